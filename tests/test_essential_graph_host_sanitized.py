"""essential_graph_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/essential_graph_core_host_test.cpp) run as a child process: Sim3::log in every branch and with a scale at the 1e-5
thresholds, the pivoting of the 3 x 3 solve, an edge with each side fixed, a zero increment, the write-back. A clean exit is required.
The sanitizer runtimes are linked statically into the program; nothing sanitised is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_essential_graph_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "essential_graph_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "essential_graph_core_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checksum ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
