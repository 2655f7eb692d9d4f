"""reloc_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/reloc_core_host_test.cpp) run as a child process: the gates of the relocalisation matcher on their edge values (a point behind
the camera, NaN coordinates, both bounds, both distance limits) and against a restatement with the reference's casts, the serial claim
plus rotation histogram against the literal loop on random and adversarial lists, the whole host matcher against a literal loop over an
mGrid of vectors, and corrupted grids, lists and counts in heap blocks of their exact size. A clean exit is required. The sanitizer
runtimes are linked statically into the program; nothing sanitised is loaded into this process, and nothing of this runs on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reloc_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "reloc_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "reloc_core_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checksum ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
