"""Shared by tests/test_walk_in_mark.py (CPU-fiber emulation) and tests/test_gpu_walk_in_mark.py (MI355X): the greedy chain's
block walk inside the marking launch (am_k_cblk_visit) against the two-launch form (am_k_cblk_walk + am_k_cblk_mark) and the
oracle.  Every library used here is a build with the test knobs: AIRMODES_WALK=separate|fused forces a form where both are
legal, AIRMODES_TRACE_SPEC=1 makes chain_finish say on stderr which one it launched.

Inputs are prefixes of ONE 64 Msps capture at 20 000 bursts/s (about 6.4 first-stage candidates per 1 000 samples, so one
2 048-node block is about 0.33 M samples).  The lengths below were chosen from the candidate counts of that capture (counted on
the CPU with the emulated library, whose candidate records tests/test_emu_parity.py holds against the oracle's); every test asserts the count its context reports, so a change of the
capture or of the detector shows as a failed placement, not as a test that silently checks something else."""
import re

import numpy as np

import oracle
import synth
from air_modes import _capi

RATE, LAM, SEED, THR = 64e6, 20000.0, 901, 7.0
CB = 2048                                   # AM_CB: nodes per block of the greedy chain
_capture = {}

# prefix length -> (lowest, highest) candidate count it must give
N_NONE = 300_000                            # zeros
N_ONE = (88_838, (900, 1_200))              # walker + one marker
N_BELOW_1 = (210_856, (CB - 64, CB - 1))    # one block, nearly full
N_ABOVE_1 = (231_694, (CB + 1, CB + 64))    # two blocks, the second nearly empty
N_BELOW_2 = (530_674, (2 * CB - 64, 2 * CB - 1))
N_ABOVE_2 = (536_888, (2 * CB + 1, 2 * CB + 64))    # three blocks


N_CAPTURE = 1_500_000


def capture(n, size=N_CAPTURE):
    """The first n samples of the capture of `size` samples (made once per size, never changed)."""
    assert n <= size
    have = _capture.get(size)
    if have is None:
        have, _ = synth.synth_capture(RATE, size, LAM, SEED)
        have.setflags(write=False)
        _capture[size] = have
    return have[:n]


def want_of(iq):
    return oracle.demod(iq, RATE, THR, True)


def run(lib, monkeypatch, capfd, mode, pieces, flush_last=True):
    """One context, one am_process_iq call per piece under AIRMODES_WALK=mode (None: the library's own choice).
    Returns (packets of every call, candidate count of every call, [(form, blocks launched)] of every chain visit, stderr)."""
    if mode is None:
        monkeypatch.delenv("AIRMODES_WALK", raising=False)
    else:
        monkeypatch.setenv("AIRMODES_WALK", mode)
    monkeypatch.setenv("AIRMODES_TRACE_SPEC", "1")
    capfd.readouterr()
    ctx = _capi.Context(RATE, THR, True, lib=lib)
    parts, counts = [], []
    for i, x in enumerate(pieces):
        parts.append(ctx.process_iq(x, flush=(flush_last and i == len(pieces) - 1)))
        counts.append(ctx.last_num_candidates())
    ctx.close()
    err = capfd.readouterr().err
    visits = [(f, int(b)) for f, b in re.findall(r"chain visit (fused|separate), (\d+) blocks", err)]
    return parts, counts, visits, err


def check_both(lib, monkeypatch, capfd, pieces, want=None, blocks=None, count=None, modes=("fused", "separate", None)):
    """The pieces through the fused form, the two-launch form and (modes[2:]) the library's own choice: packets byte for byte equal to each other
    and to the oracle over the concatenation; every visit of a forced run took the forced form.  blocks: the number of blocks the
    LAST call's candidate count must give; count: the (lo, hi) range it must lie in.  Returns the fused run's (counts, visits)."""
    whole = np.concatenate([np.asarray(p) for p in pieces]) if len(pieces) > 1 else pieces[0]
    if want is None:
        want = want_of(whole)
    out = {}
    for mode in modes:
        parts, counts, visits, err = run(lib, monkeypatch, capfd, mode, pieces)
        got = np.concatenate(parts)
        assert got.tobytes() == want.tobytes(), "AIRMODES_WALK=%s: %d vs %d packets\n%s" % (mode, len(got), len(want), err)
        if mode is not None:
            assert all(f == mode for f, _ in visits), "AIRMODES_WALK=%s ran %r" % (mode, visits)
        out[mode] = (parts, counts, visits)
    # the same packets in the same calls, whichever form ran
    for mode in modes[1:]:
        assert [p.tobytes() for p in out[mode][0]] == [p.tobytes() for p in out["fused"][0]], "calls differ between the forms"
        assert out[mode][1] == out["fused"][1], "candidate counts differ between the forms"
    counts, visits = out["fused"][1], out["fused"][2]
    if count is not None:
        assert count[0] <= counts[-1] <= count[1], "%d candidates, meant to lie in %r" % (counts[-1], count)
    if blocks is not None:
        assert (counts[-1] + CB - 1) // CB == blocks, "%d candidates are not %d blocks" % (counts[-1], blocks)
        assert visits and visits[-1][1] >= blocks, visits       # (a capacity launch may cover more blocks than the count needs)
    return counts, visits


def check_nothing(lib, monkeypatch, capfd):
    """No candidate at all: no chain visit is launched, in either form, and nothing waits."""
    z = np.zeros(N_NONE, np.complex64)
    for mode in ("fused", "separate", None):
        parts, counts, visits, err = run(lib, monkeypatch, capfd, mode, [z])
        assert len(parts[0]) == 0 and counts == [0] and visits == [], (mode, counts, visits)
    assert len(want_of(z)) == 0


def check_stream(lib, monkeypatch, capfd, n, cuts, modes=("fused", "separate", None)):
    """One stream in len(cuts) + 1 calls (no flush between them: the resume position crosses the calls, raised by the markers and
    the walker of one launch; later calls start their scan past node 0) against the same samples in one call and the oracle."""
    iq = capture(n)
    want = want_of(iq)
    assert len(want) >= 10
    edges = [0] + list(cuts) + [n]
    pieces = [iq[a:b] for a, b in zip(edges[:-1], edges[1:])]
    counts, visits = check_both(lib, monkeypatch, capfd, pieces, want=want, modes=modes)
    assert len(visits) == len(pieces) and all(c > 0 for c in counts)
    one, _, v1, _ = run(lib, monkeypatch, capfd, "fused", [iq])
    assert one[0].tobytes() == want.tobytes() and v1 and v1[0][0] == "fused"
    return counts


def check_capacity(lib, monkeypatch, capfd, n_quiet, n_dense, n_third):
    """A sparse call, then a dense one on the same context (launched for the sparse call's density: the scan outgrows its
    capacity and is redone with the exact count), then a third call that fits.  AIRMODES_SPEC_FLOOR=0: no slack."""
    monkeypatch.setenv("AIRMODES_SPEC_FLOOR", "0")
    quiet, _ = synth.synth_capture(RATE, n_quiet, 300.0, 5)
    dense = capture(n_dense + n_third)
    pieces = [quiet, dense[:n_dense], dense[n_dense:]]
    want = want_of(np.concatenate(pieces))
    assert len(want) >= 10
    for mode in ("fused", "separate"):
        parts, counts, visits, err = run(lib, monkeypatch, capfd, mode, pieces)
        assert np.concatenate(parts).tobytes() == want.tobytes(), "AIRMODES_WALK=%s: packets differ\n%s" % (mode, err)
        assert counts[0] >= 1 and counts[1] > 4 * counts[0], "no overflow: %r" % (counts,)
        assert "scan redone" in err, err
        assert len(visits) >= 4 and all(f == mode for f, _ in visits), visits      # (the dense call visits twice)
        assert (counts[1] + CB - 1) // CB >= 2
    return counts
