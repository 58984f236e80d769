"""The greedy chain's block walk inside the marking launch (am_k_cblk_visit), on the CPU-fiber emulation of the kernels: against the
two-launch form on the same input (AIRMODES_WALK) and against the oracle, packets byte for byte.  The emulation runs the
workgroups of a launch one after the other; place 0 of the tickets -- the walker -- runs first and publishes every block's
entry word, so each marker finds its word at its first poll.  What the emulation cannot show (markers polling while the walker
runs, other contexts' kernels on the same CUs) is in tests/test_gpu_walk_in_mark.py.  Nothing has to be resident at once here, so the
emulated libraries' own choice is the fused form at any size (test_blocks[one_marker] checks it); the other cases force both forms.

The emulated builds cut the walk into groups of AM_CB_GROUP = 2 blocks; libairmodes_emu_rare.so also has 4-slot block heads, so
that nearly every hop of the walker lands beyond a head (AM_CB_OUT) and goes through global memory inside the fused kernel."""
import pytest

import walk_common as wc

BOTH = ("fused", "separate")


def test_no_candidate_launches_nothing(emu_lib, monkeypatch, capfd):
    wc.check_nothing(emu_lib, monkeypatch, capfd)


@pytest.mark.parametrize("case,blocks", [(wc.N_ONE, 1), (wc.N_BELOW_1, 1), (wc.N_ABOVE_1, 2), (wc.N_BELOW_2, 2), (wc.N_ABOVE_2, 3)],
                         ids=["one_marker", "below_2048", "above_2048", "below_4096", "above_4096"])
def test_blocks(emu_lib, monkeypatch, capfd, case, blocks):
    n, count = case
    modes = ("fused", "separate", None) if blocks == 1 else BOTH
    counts, visits = wc.check_both(emu_lib, monkeypatch, capfd, [wc.capture(n)], blocks=blocks, count=count, modes=modes)
    assert len(visits) == 1


def test_more_blocks_than_a_group(emu_lib, monkeypatch, capfd):
    """1.4 M samples: five blocks, three groups of two -- all three steps of the walker's two-level walk."""
    counts, visits = wc.check_both(emu_lib, monkeypatch, capfd, [wc.capture(1_400_000)], blocks=5, count=(4 * wc.CB + 1, 5 * wc.CB),
                                   modes=BOTH)
    assert len(visits) == 1


@pytest.mark.parametrize("case,blocks", [(wc.N_ONE, 1), (wc.N_ABOVE_1, 2), (wc.N_ABOVE_2, 3)], ids=["one_marker", "two", "three"])
def test_rare_branches(emu_lib_rare, monkeypatch, capfd, case, blocks):
    n, count = case
    wc.check_both(emu_lib_rare, monkeypatch, capfd, [wc.capture(n)], blocks=blocks, count=count, modes=BOTH)


@pytest.mark.parametrize("cuts", [(200_001,), (120_000, 300_003)], ids=["two_calls", "three_calls"])
@pytest.mark.parametrize("which", ["plain", "rare"])
def test_stream_in_calls(emu_lib, emu_lib_rare, monkeypatch, capfd, which, cuts):
    wc.check_stream(emu_lib if which == "plain" else emu_lib_rare, monkeypatch, capfd, 450_000, cuts, modes=BOTH)


def test_capacity_launches(emu_lib, monkeypatch, capfd):
    wc.check_capacity(emu_lib, monkeypatch, capfd, 300_000, 540_000, 300_000)
