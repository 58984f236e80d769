"""am_options.h: the four opt-in decode options as one value -- which requests each option's function stores, which it refuses,
and that a refusal leaves the value as it was (tests/helpers/options_check.cc).  CPU only: the header is plain C++17 and is
compiled alone, with the host compiler."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gr-air-modes_amd", "csrc")


def test_options(tmp_path):
    exe = str(tmp_path / "options_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "helpers", "options_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
