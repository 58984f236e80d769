"""The greedy chain's block walk inside the marking launch (am_k_cblk_visit) on a real MI355X: markers poll for their block's
entry word while the walker of the same launch runs, workgroups land on whatever CU and XCD the hardware picks.  Every case
compares the packets byte for byte with the oracle and with the two-launch form on the same input (AIRMODES_WALK, read by the
builds with the test knobs only), and asserts from the candidate count its context reports that it sits where it is meant to
(tests/walk_common.py).  Which form ran is read from the knobs builds' trace (AIRMODES_TRACE_SPEC), never from timing; the product
library, which reads nothing from the environment, runs the same inputs against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import walk_common as wc
from air_modes import _capi

pytestmark = pytest.mark.gpu

N_BIG = 6_400_000                            # about 20 blocks: more than AM_CB_GROUP = 16 of the device builds


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hip_lib


@pytest.fixture(scope="module")
def klib(hip_knobs_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hip_knobs_lib


@pytest.fixture(scope="module")
def rare():
    """4-slot block heads, groups of two blocks (gr-air-modes_amd/csrc/Makefile, target `rare`): every hop of the walker takes the
    AM_CB_OUT / global-hop branches.  Built the way tests/test_gpu_parity.py builds it."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_variants", "libairmodes_hip_rare.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(path), "..", "..", "gr-air-modes_amd", "csrc"), "rare"])
    return _capi.Library(path)


def product(lib, pieces):
    """The product library's own choice on the same calls: packets of every call."""
    ctx = _capi.Context(wc.RATE, wc.THR, True, lib=lib)
    parts = [ctx.process_iq(x, flush=(i == len(pieces) - 1)) for i, x in enumerate(pieces)]
    ctx.close()
    return np.concatenate(parts)


def test_no_candidate_launches_nothing(lib, klib, monkeypatch, capfd):
    wc.check_nothing(klib, monkeypatch, capfd)
    assert len(product(lib, [np.zeros(wc.N_NONE, np.complex64)])) == 0


@pytest.mark.parametrize("case,blocks", [(wc.N_ONE, 1), (wc.N_BELOW_1, 1), (wc.N_ABOVE_1, 2), (wc.N_BELOW_2, 2), (wc.N_ABOVE_2, 3)],
                         ids=["one_marker", "below_2048", "above_2048", "below_4096", "above_4096"])
def test_blocks(lib, klib, monkeypatch, capfd, case, blocks):
    n, count = case
    iq = wc.capture(n)
    want = wc.want_of(iq)
    counts, visits = wc.check_both(klib, monkeypatch, capfd, [iq], want=want, blocks=blocks, count=count)
    assert len(visits) == 1
    assert product(lib, [iq]).tobytes() == want.tobytes()


def test_more_blocks_than_a_group(lib, klib, monkeypatch, capfd):
    """About 20 blocks: the walker's group table (step 1), its group-to-group lane (2) and the entries inside the groups (3)."""
    iq = wc.capture(N_BIG, size=N_BIG)
    want = wc.want_of(iq)
    counts, visits = wc.check_both(klib, monkeypatch, capfd, [iq], want=want, count=(16 * wc.CB + 1, 30 * wc.CB))
    assert len(visits) == 1 and visits[0][1] > 16
    _, _, own, _ = wc.run(klib, monkeypatch, capfd, None, [iq])
    assert own == [("fused", visits[0][1])], own              # (a plain scan of a few dozen blocks: the library's own choice)
    assert product(lib, [iq]).tobytes() == want.tobytes()


@pytest.mark.parametrize("case,blocks", [(wc.N_ONE, 1), (wc.N_ABOVE_1, 2), (wc.N_ABOVE_2, 3)], ids=["one_marker", "two", "three"])
def test_rare_branches(rare, monkeypatch, capfd, case, blocks):
    n, count = case
    wc.check_both(rare, monkeypatch, capfd, [wc.capture(n)], blocks=blocks, count=count)


def test_rare_branches_many_blocks(rare, monkeypatch, capfd):
    wc.check_both(rare, monkeypatch, capfd, [wc.capture(1_400_000)], blocks=5, count=(4 * wc.CB + 1, 5 * wc.CB))


@pytest.mark.parametrize("cuts", [(500_001,), (300_000, 900_003)], ids=["two_calls", "three_calls"])
def test_stream_in_calls(lib, klib, rare, monkeypatch, capfd, cuts):
    n = 1_400_000
    wc.check_stream(klib, monkeypatch, capfd, n, cuts)
    wc.check_stream(rare, monkeypatch, capfd, n, cuts)
    iq = wc.capture(n)
    edges = [0] + list(cuts) + [n]
    assert product(lib, [iq[a:b] for a, b in zip(edges[:-1], edges[1:])]).tobytes() == wc.want_of(iq).tobytes()


def test_capacity_launches(klib, monkeypatch, capfd):
    wc.check_capacity(klib, monkeypatch, capfd, 300_000, 900_000, 500_000)


@pytest.mark.timeout(180)
def test_pipe_of_four(klib, monkeypatch, capfd):
    """am_pipe of depth 4 over six batches of about a million samples, fused form forced (a deferred tail takes the two launches by
    itself: it was measured slower fused, not wrong): up to four contexts' front ends, refinements and fused visits compete for the
    CUs while a fused launch's markers wait for their walker.  Packets equal the synchronous calls.  (The wait is bounded: a design
    error would come back as AM_EHIP from a collect, not as a stall -- and this test has a time limit besides.)"""
    import torch
    monkeypatch.delenv("AIRMODES_WALK", raising=False)
    monkeypatch.setenv("AIRMODES_TRACE_SPEC", "1")
    iq = wc.capture(N_BIG, size=N_BIG)
    edges = [0, 1_000_000, 2_100_000, 3_000_001, 4_200_000, 5_300_000, N_BIG]
    batches = [iq[a:b] for a, b in zip(edges[:-1], edges[1:])]
    ctx = _capi.Context(wc.RATE, wc.THR, True, lib=klib)
    want = [ctx.process_iq(b, flush=True) for b in batches]
    ctx.close()
    for b, w in zip(batches, want):
        assert w.tobytes() == wc.want_of(b).tobytes() and len(w) >= 10
    dev = [torch.from_numpy(np.ascontiguousarray(b).view(np.float32).copy()).cuda() for b in batches]
    torch.cuda.synchronize()
    for mode, form, other in (("fused", "chain visit fused", "chain visit separate"), (None, "chain visit separate", "chain visit fused")):
        if mode:
            monkeypatch.setenv("AIRMODES_WALK", mode)
        else:
            monkeypatch.delenv("AIRMODES_WALK", raising=False)
        capfd.readouterr()
        pipe = _capi.Pipe(wc.RATE, wc.THR, True, device=0, depth=4, lib=klib)
        got = []
        for d, b in zip(dev, batches):
            if pipe.in_flight() == pipe.depth():
                got.append(pipe.collect())
            pipe.submit_device(d.data_ptr(), len(b))
        while pipe.in_flight():
            got.append(pipe.collect())
        pipe.close()
        err = capfd.readouterr().err
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.tobytes() == w.tobytes(), "AIRMODES_WALK=%s, batch %d: %d vs %d packets" % (mode, k, len(g), len(w))
        assert err.count(form) >= len(batches) and other not in err, err


def test_more_blocks_than_cus_takes_two_launches(klib, monkeypatch, capfd):
    """A scan of more blocks than the device has CUs: the fused kernel's workgroups (1 024 threads, the walk's tables in LDS: one
    per CU) would no longer be resident in one round, so the library takes the two-launch form by itself.  About 90 M samples at
    64 Msps for 256 CUs: eight copies of an 11.25 M sample capture, one behind the other (one stream; the oracle is the witness).
    Forced, the fused form still gives the same packets: places go by ticket, whoever is not resident yet waits for a CU, not
    for a word."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    part = wc.capture(11_250_000, size=11_250_000)
    reps = max(1, -(-(cus + 8) * wc.CB // 70_000))           # (about 72 000 candidates per copy; a few blocks to spare)
    iq = np.tile(part, reps)
    want = wc.want_of(iq)
    assert len(want) >= 100 * reps
    parts, counts, visits, err = wc.run(klib, monkeypatch, capfd, None, [iq])
    blocks = (counts[0] + wc.CB - 1) // wc.CB
    assert blocks + 1 > cus, "%d candidates = %d blocks do not outnumber %d CUs" % (counts[0], blocks, cus)
    assert parts[0].tobytes() == want.tobytes()
    assert visits and all(f == "separate" for f, _ in visits), visits
    parts, counts2, visits, err = wc.run(klib, monkeypatch, capfd, "fused", [iq])
    assert parts[0].tobytes() == want.tobytes() and counts2 == counts
    assert visits and all(f == "fused" for f, _ in visits), visits
