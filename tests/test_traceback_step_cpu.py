"""The traceback's step on the CPU -- no GPU.

tools/traceback_host_check.cpp runs the kernels' own text (csrc/traceback_step.h: the node record's packer and accessors, the
two sources of a step's candidates) under ASan and UBSan: random CSR models packed and read back, the 256-score rule from both
sides, the record source against the CSR source on every state, lane and kind of column, and five states against candidate
lists typed in from DESIGN 3.5.  The test builds and runs it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# how the program's one summary line begins when every check held (the sizes of its run follow)
HOST_CHECK_LINE = b"traceback host check: ok ("


def test_step_text_under_sanitizers(tmp_path):
    exe = str(tmp_path / "traceback_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "traceback_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and HOST_CHECK_LINE in r.stdout, (r.stdout.decode(), r.stderr.decode()[-4000:])
