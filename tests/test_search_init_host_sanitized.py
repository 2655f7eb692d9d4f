"""search_init_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/search_init_core_host_test.cpp) run as a child process: the sweeps of the ordered phase against the literal loop on random
candidate lists and both staircases, the pruning rule and the radix select of the scene depth (the windows, the bins and the three maxima
moved to tests/test_match_core_host_sanitized.py with their code). A clean exit is required. The sanitizer runtimes are linked statically into the program; nothing sanitised is loaded into
this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_init_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "search_init_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "search_init_core_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checksum ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
