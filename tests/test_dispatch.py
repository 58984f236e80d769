"""am_dispatch.h: which <FIX, GATE> and <SPC> instantiation a run-time value selects, and one occupancy cache per instantiation
(tests/helpers/dispatch_check.cc).  CPU only: the header is plain C++17 and is compiled alone, with the host compiler."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gr-air-modes_amd", "csrc")


def test_dispatch(tmp_path):
    exe = str(tmp_path / "dispatch_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "helpers", "dispatch_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
