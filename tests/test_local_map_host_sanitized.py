"""local_map_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/local_map_core_host_test.cpp) run as a child process: validate, votes, the voted list, the neighbour loop and the points against
the literal loop on more than 3000 random small streams (the program itself requires that they hold a case without votes, a tie for the
most votes, the break at more than 80 entries, a skipped bad neighbour and a point dropped at a later occurrence); then every kind of
broken snapshot, each of which the validator must refuse without reading through it, and both overflows by one. A clean exit is required.
The sanitizer runtimes are linked statically into the program; nothing sanitised is loaded into this process."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_local_map_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "local_map_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "local_map_core_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checksum ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    seen = dict(re.findall(r"(streams|no-votes|tie|limit-break|skipped-bad-neighbour|first-occurrence) (\d+)", r.stdout))
    assert int(seen["streams"]) >= 3000 and all(int(seen[k]) >= 1 for k in ("no-votes", "tie", "limit-break", "skipped-bad-neighbour", "first-occurrence"))
