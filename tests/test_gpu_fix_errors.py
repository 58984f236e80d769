"""Opt-in repair of DF11 / DF17 replies with one or two wrong bits (am_set_fix_errors) on the device: every kernel that
slices -- am_k_slice, am_k_extract_slice_iq<SPC>, am_k_extract_slice -- through the C ABI, byte for byte against the numpy
definition in tests/fix_common.py (which tests/test_fix_errors.py pins to the reference's own slicer)."""
import numpy as np
import pytest

import fix_common as fx
import oracle
import parity_common as pc
import synth
from air_modes import _capi

pytestmark = pytest.mark.gpu

# low-SNR seeded captures (4-14 dB), sizes the streaming front end serves: (rate, samples, bursts per second, seed)
CAPTURES = {2: (2e6, 2_000_000, 4000.0, 81), 4: (4e6, 2_000_000, 4000.0, 82), 20: (20e6, 12_000_000, 8000.0, 83),
            64: (64e6, 32_000_000, 6000.0, 84), 5: (5e6, 2_000_000, 5000.0, 85)}
_cache = {}


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    oracle.build()
    return hip_lib


def capture(msps):
    """(iq, {max_bits: expected packets}); the expected list must hold tens of one-bit and of two-bit repairs BEFORE the
    library is asked."""
    if msps not in _cache:
        rate, n, lam, seed = CAPTURES[msps]
        iq, _ = fx.low_snr_capture(rate, n, seed, lam=lam)
        want = {mb: fx.expected_from_capture(iq, rate, mb) for mb in (0, 1, 2)}
        n11, n17, n2 = fx.repaired_counts(want[2])
        print("capture %g Msps: %d / %d / %d packets, repairs DF11 %d DF17 %d two-bit %d"
              % (msps, len(want[0]), len(want[1]), len(want[2]), n11, n17, n2))
        assert n11 + n17 >= 20 and n2 >= 20 and fx.repaired_counts(want[1]) == (n11, n17, 0)
        assert want[0].tobytes() == oracle.demod(iq, rate).tobytes()
        _cache[msps] = (iq, want)
    return _cache[msps]


def uneven_cuts(n):
    return [0, n // 7 + 1, n // 7 + 2, n // 2 + 13, n - n // 5, n - 333, n]


def test_slicer_kernel_repairs_as_defined(lib):
    """am_slicer_work -> am_k_slice<FIX> on 120 000 damaged bursts and the edge vectors."""
    b, t, _ = fx.damaged_bursts(120_000, 12)
    eb, et = pc.edge_bursts(4000, 3)
    ctx = _capi.Context(4e6, 7.0, True, lib=lib)
    for mb in (0, 1, 2):
        want = fx.slice_fix(b, t, mb)[0]
        n11, n17, n2 = fx.repaired_counts(want)
        print("max_bits %d: %d packets, repairs DF11 %d DF17 %d two-bit %d" % (mb, len(want), n11, n17, n2))
        if mb:
            assert n11 >= 200 * 20 and n17 >= 800 * 20 and (mb == 1 or n2 >= 800 * 20)       # (20 x the floors for 6 000 bursts)
        ctx.set_fix_errors(mb)
        got = ctx.slicer_work(b, t)
        assert got.tobytes() == want.tobytes(), "max_bits %d: %d vs %d packets" % (mb, len(got), len(want))
        ewant = fx.slice_fix(eb, et, mb)[0]
        egot = ctx.slicer_work(eb, et)
        assert egot.tobytes() == ewant.tobytes()
        if mb == 0:
            assert got.tobytes() == oracle.slice_bursts(b, t).tobytes()                      # the unchanged contract
            assert egot.tobytes() == oracle.slice_bursts(eb, et).tobytes()
    ctx.close()


@pytest.mark.parametrize("msps", [2, 4, 20, 64])
def test_production_path_repairs_as_defined(lib, msps):
    """am_k_extract_slice_iq<SPC, FIX> behind the streaming front end: one call, and uneven chunks with a flush."""
    iq, want = capture(msps)
    rate, n = CAPTURES[msps][0], len(iq)
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    for mb in (0, 1, 2):
        ctx.set_fix_errors(mb)
        got = ctx.process_iq(iq, flush=True)
        assert ctx.last_frontend() == 3
        assert got.tobytes() == want[mb].tobytes(), "max_bits %d: %d vs %d packets" % (mb, len(got), len(want[mb]))
        assert lib.format_messages(got, True) == oracle.format_messages(want[mb])
        cuts = uneven_cuts(n)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == want[mb].tobytes()
    ctx.close()


def test_pipes_repair_as_defined(lib):
    """am_pipe (whole batches in flight) and am_spipe (one stream, chunks in flight) at 64 Msps."""
    import torch
    iq, want = capture(64)
    rate, n = CAPTURES[64][0], len(iq)
    pipe = _capi.Pipe(rate, 7.0, True, depth=3, lib=lib)
    half = iq[:n // 2 + 5]
    want_half = {mb: fx.expected_from_capture(half, rate, mb) for mb in (0, 2)}
    for mb in (2, 0):
        pipe.set_fix_errors(mb)
        assert pipe.get_fix_errors() == mb
        pipe.submit(iq)
        pipe.submit(half)
        pipe.submit(iq)
        assert pipe.collect().tobytes() == want[mb].tobytes()
        assert pipe.collect().tobytes() == want_half[mb].tobytes()
        assert pipe.collect().tobytes() == want[mb].tobytes()
    pipe.close()
    sp = _capi.StreamPipe(rate, 7.0, True, depth=3, lib=lib)
    base = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
    torch.cuda.synchronize()
    cuts = [0, 5_000_001, 9_000_000, 17_777_777, 26_000_000, n]
    chunks = [(base.data_ptr() + 8 * a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    for mb in (1, 2, 0):
        sp.set_fix_errors(mb)
        assert sp.get_fix_errors() == mb
        got = np.concatenate(sp.run(chunks))
        assert got.tobytes() == want[mb].tobytes(), "stream pipe, max_bits %d: %d vs %d packets" % (mb, len(got), len(want[mb]))
    sp.close()
    del base


def test_fractional_rate_and_generic_kernels(lib, hip_knobs_lib, monkeypatch):
    """5 Msps (2.5 samples per chip: the rate-generic kernels, am_k_extract_slice<FIX> with the chip table), and the same
    kernel at whole rates in the test build that can be told to use the generic kernels only."""
    iq, want = capture(5)
    ctx = _capi.Context(5e6, 7.0, True, lib=lib)
    n = len(iq)
    for mb in (0, 1, 2):
        ctx.set_fix_errors(mb)
        assert ctx.process_iq(iq, flush=True).tobytes() == want[mb].tobytes()
        assert ctx.last_frontend() == 1
        cuts = uneven_cuts(n)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == want[mb].tobytes()
    ctx.close()
    monkeypatch.setenv("AIRMODES_GENERIC", "1")
    for msps in (4, 20):
        iq, want = capture(msps)
        ctx = _capi.Context(CAPTURES[msps][0], 7.0, True, lib=hip_knobs_lib)
        for mb in (0, 1, 2):
            ctx.set_fix_errors(mb)
            assert ctx.process_iq(iq, flush=True).tobytes() == want[mb].tobytes()
            assert ctx.last_frontend() == 1
        ctx.close()


def test_bank_of_three_receivers(lib):
    """rx_path_bank (am_process_multi): receiver j's queue == its own rx_path(fix_errors=2)."""
    import air_modes
    iq = capture(20)[0]
    rate = CAPTURES[20][0]
    caps = [iq[:4_000_000], iq[4_000_000:9_000_001], iq[6_000_000:]]
    qs = [air_modes.msg_queue() for _ in caps]
    bank = air_modes.rx_path_bank(rate, 7.0, qs, use_pmf=True, device=0, lib=lib, fix_errors=2)
    per = bank.work(caps)
    assert sum(int(np.count_nonzero(p["reserved"][:, 1])) for p in per) >= 30
    for q, cap in zip(qs, caps):
        got = []
        while not q.empty_p():
            got.append(q.delete_head().to_string())
        q1 = air_modes.msg_queue()
        rx = air_modes.rx_path(rate, 7.0, q1, use_pmf=True, device=0, lib=lib, fix_errors=2)
        rx.work(cap, flush=True)
        own = []
        while not q1.empty_p():
            own.append(q1.delete_head().to_string())
        assert got == own and rx.repaired > 0
        assert got == oracle.format_messages(fx.expected_from_capture(cap, rate, 2))


def test_off_means_off(lib):
    """The 64 Msps stress capture of the benchmark's configuration: a context that had the repair on and then off returns
    what a fresh context returns, which is what the oracle returns."""
    rate, (iq, _) = synth.config_capture("64msps")
    want = oracle.demod(iq, rate)
    fresh = _capi.Context(rate, 7.0, True, lib=lib)
    a = fresh.process_iq(iq, flush=True)
    fresh.close()
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_fix_errors(2)
    on = ctx.process_iq(iq, flush=True)
    assert on.tobytes() == fx.expected_from_capture(iq, rate, 2).tobytes() and np.count_nonzero(on["reserved"][:, 1]) >= 100
    ctx.set_fix_errors(0)
    b = ctx.process_iq(iq, flush=True)
    ctx.close()
    assert a.tobytes() == b.tobytes() == want.tobytes() and len(want) > 1000
