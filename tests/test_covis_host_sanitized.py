"""covis_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/covis_core_host_test.cpp) run as a child process: validate, counters, AddConnection, the target's own members, the first
connection and LoopConnections against the literal loop on more than 3000 random small streams; then every kind of broken snapshot, each
of which the validator must refuse without reading through it, and the overflow by one. The program prints how often its random set held
each situation that is easy to get wrong, and each must be there at least once. A clean exit is required. The sanitizer runtimes are
linked statically into the program; nothing sanitised is loaded into this process."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITUATIONS = ("fallback", "tie", "equal-weights", "early-return", "rebuild-pulls-sub-threshold", "first-parent", "stale", "loop-nonempty", "loop-empty")


def test_covis_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "covis_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "covis_core_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checksum ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    seen = dict(re.findall(r"(streams|%s) (\d+)" % "|".join(SITUATIONS), r.stdout))
    assert int(seen["streams"]) >= 3000 and all(int(seen[k]) >= 1 for k in SITUATIONS), seen
