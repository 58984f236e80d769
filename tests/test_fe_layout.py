"""am_fe_plan / am_fe_layout (am_internal.h): the one description of the bitmap a streaming front end leaves, against the three
derivations it replaced and against what any layout must satisfy (tests/helpers/fe_layout_check.cc).  CPU only: the front ends'
sources compiled as C++ against the emulation headers, as tests/emu/Makefile does."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gr-air-modes_amd", "csrc")


def test_fe_layout(tmp_path):
    exe = str(tmp_path / "fe_layout_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas",
                           "-Wno-unused-function", "-DAM_TEST_KNOBS=1", "-I", os.path.join(HERE, "emu"), "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(HERE, "helpers", "fe_layout_check.cc"),
                           os.path.join(HERE, "emu", "hipemu.cc"), "-x", "c++", os.path.join(CSRC, "am_fe3.hip"),
                           os.path.join(CSRC, "am_fe4.hip")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
