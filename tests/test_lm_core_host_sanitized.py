"""lm_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/lm_core_host_test.cpp) run as a child process: a literal restatement of g2o's Levenberg control and the lm_core.h functions
composed as the solver loops compose them consume the same scripted trials and must agree bit for bit after every trial, for both
spellings of the cube; then 10 000 seeded random scripts. The same program drives lba_ctl.h, the control block of the window solves
(lba_lambda0 / lba_decide / lba_phase), through scripted and random windows of two optimize() calls against that restatement, again
bit for bit after every trial. A clean exit is required. The sanitizer runtimes are linked statically into
the program; nothing sanitised is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lm_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lm_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lm_core_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("lm_core: ") and "\nlba_ctl: " in r.stdout and "lm_core ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
