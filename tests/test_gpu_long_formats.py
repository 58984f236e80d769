"""Opt-in 112-bit slicing and parity check of DF18 / DF19 squitters (am_set_long_formats) on the device: every kernel that
slices -- am_k_slice, am_k_extract_slice_iq<SPC> (direct and staged loads), am_k_extract_slice -- through the C ABI, byte for byte
against the numpy definition in tests/longfmt_common.py (which tests/test_long_formats.py pins to the reference's own slicer),
never against the library itself."""
import numpy as np
import pytest

import gate_common as gc
import longfmt_common as lf
import oracle
import parity_common as pc
import synth
from air_modes import _capi

pytestmark = pytest.mark.gpu

# seeded captures at SNR 6-14 dB, the smallest the streaming front ends take whole steps of: (rate, samples, bursts / s, seed)
CAPTURES = {2: (2e6, 400_000, 3000.0, 41), 4: (4e6, 800_000, 6000.0, 33), 20: (20e6, 2_000_000, 10000.0, 43),
            64: (64e6, 4_000_000, 12000.0, 44), 5: (5e6, 1_000_000, 5000.0, 45)}
SETTINGS = ((3, 0), (3, 2), (1, 2), (0, 0))           # (mask, fix_errors)
EARLY = 0                                              # 64 Msps: a DF18 burst starts at this sample of the stream
TTL_S = 60.0
_cache = {}


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    oracle.build()
    return hip_lib


def capture(msps):
    """(iq, what the oracle's scan hands the slicer, {(mask, fix): expected packets}); the expected lists hold DF18 and DF19
    packets, clean and repaired, BEFORE the library is asked."""
    if msps not in _cache:
        rate, n, lam, seed = CAPTURES[msps]
        iq, _ = lf.capture(rate, n, lam, seed)
        early = None
        if msps == 64:
            # a burst at the very start of the stream.  The matched filter looks back over 32 samples, so the hit lies 31 samples
            # behind the burst's own first one (and its tag 2 * 32 - 1 behind that): its window begins before the source,
            # its loads are not all inside it, and it takes am_k_extract_slice_iq's direct path, not the staged one of every
            # other hit here -- both must form chips 128..239 of a DF18.  (One sample later the hit is staged again.)
            early = lf.frame(np.random.default_rng(7), 18)
            iq = lf.add_burst(iq, rate, EARLY, early)
        sc = lf.scan(iq, rate)
        want = {s: lf.expected(sc, s[1], s[0]) for s in SETTINGS}
        c18, c19, r18, r19 = lf.counts(want[(3, 2)])
        print("capture %g Msps: %s packets, DF18 %d DF19 %d clean, %d %d repaired"
              % (msps, [len(want[s]) for s in SETTINGS], c18, c19, r18, r19))
        assert c18 >= 20 and c19 >= 10 and r18 + r19 >= 5
        assert lf.counts(want[(1, 2)])[1::2] == (0, 0) and lf.counts(want[(0, 0)]) == (0, 0, 0, 0)
        assert want[(0, 0)].tobytes() == oracle.demod(iq, rate).tobytes()
        assert len(set(w.tobytes() for w in want.values())) == len(SETTINGS)
        if early is not None:
            first = want[(3, 0)][0]
            assert bytes(first["data"][:14]) == early and first["nbytes"] == 14
            assert int(first["sample"]) - (2 * 32 - 1) < 32         # the hit's own sample: the kernel's `inside` fails below 32
        _cache[msps] = (iq, sc, want)
    return _cache[msps]


def uneven_cuts(n):
    return [0, n // 7 + 1, n // 7 + 2, n // 2 + 13, n - n // 5, n - 333, n]


def test_slicer_kernel_as_defined(lib):
    """am_slicer_work -> am_k_slice<FIX, 0, LF> on 8 000 constructed bursts and the edge vectors: every mask x fix 0 / 2."""
    b, t, _ = lf.long_bursts(8000, 22)
    eb, et = pc.edge_bursts(4000, 3)
    ctx = _capi.Context(4e6, 7.0, True, lib=lib)
    seen = set()
    for mask in (0, 1, 2, 3):
        for mb in (0, 2):
            want = lf.slice_long(b, t, mb, mask)[0]
            c18, c19, r18, r19 = lf.counts(want)
            print("mask %d fix %d: %d packets, DF18 %d DF19 %d clean, %d %d repaired" % (mask, mb, len(want), c18, c19, r18, r19))
            assert (c18 >= 500) == bool(mask & 1) and (c19 >= 500) == bool(mask & 2)
            assert (r18 >= 500) == bool(mask & 1 and mb) and (r19 >= 500) == bool(mask & 2 and mb)
            seen.add(want.tobytes())
            ctx.set_fix_errors(mb)
            ctx.set_long_formats(mask)
            got = ctx.slicer_work(b, t)
            assert got.tobytes() == want.tobytes(), "mask %d fix %d: %d vs %d packets" % (mask, mb, len(got), len(want))
            assert ctx.slicer_work(eb, et).tobytes() == lf.slice_long(eb, et, mb, mask)[0].tobytes()
            if mask == 0 and mb == 0:
                assert got.tobytes() == oracle.slice_bursts(b, t).tobytes()                  # the unchanged contract
    assert len(seen) == 8
    ctx.close()


@pytest.mark.parametrize("msps", [2, 4, 20, 64])
def test_production_path_as_defined(lib, msps):
    """am_k_extract_slice_iq<SPC, FIX, 0, LF> behind the streaming front end: one call, and uneven chunks with a flush."""
    iq, _, want = capture(msps)
    rate, n = CAPTURES[msps][0], len(iq)
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    for (mask, mb), w in want.items():
        ctx.set_fix_errors(mb)
        ctx.set_long_formats(mask)
        got = ctx.process_iq(iq, flush=True)
        assert ctx.last_frontend() == 3
        assert got.tobytes() == w.tobytes(), "mask %d fix %d: %d vs %d packets" % (mask, mb, len(got), len(w))
        assert lib.format_messages(got, True) == oracle.format_messages(w)
        cuts = uneven_cuts(n)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == w.tobytes()
    ctx.close()


def test_fractional_rate_and_generic_kernels(lib, hip_knobs_lib, monkeypatch):
    """5 Msps (2.5 samples per chip: am_k_extract_slice<FIX, 0, LF> with the chip table), and the same kernel at 4 Msps in the
    test build that can be told to use the generic kernels only."""
    iq, _, want = capture(5)
    n = len(iq)
    ctx = _capi.Context(5e6, 7.0, True, lib=lib)
    for (mask, mb), w in want.items():
        ctx.set_fix_errors(mb)
        ctx.set_long_formats(mask)
        assert ctx.process_iq(iq, flush=True).tobytes() == w.tobytes()
        assert ctx.last_frontend() == 1
        cuts = uneven_cuts(n)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == w.tobytes()
    ctx.close()
    monkeypatch.setenv("AIRMODES_GENERIC", "1")
    iq, _, want = capture(4)
    ctx = _capi.Context(4e6, 7.0, True, lib=hip_knobs_lib)
    for (mask, mb), w in want.items():
        ctx.set_fix_errors(mb)
        ctx.set_long_formats(mask)
        assert ctx.process_iq(iq, flush=True).tobytes() == w.tobytes()
        assert ctx.last_frontend() == 1
    ctx.close()


def test_pipes_as_defined(lib):
    """am_pipe at depth 3 (whole batches in flight) and am_spipe with four chunks of one stream, at 64 Msps."""
    import torch
    iq, _, want = capture(64)
    rate, n = CAPTURES[64][0], len(iq)
    half = iq[:n // 2 + 5]
    half_sc = lf.scan(half, rate)
    pipe = _capi.Pipe(rate, 7.0, True, depth=3, lib=lib)
    for mask, mb in ((3, 2), (0, 0), (1, 2)):
        pipe.set_fix_errors(mb)
        pipe.set_long_formats(mask)
        assert pipe.get_long_formats() == mask
        pipe.submit(iq)
        pipe.submit(half)
        pipe.submit(iq)
        with pytest.raises(_capi.AirModesError):
            pipe.set_long_formats(0)                                    # batches in flight
        assert pipe.collect().tobytes() == want[(mask, mb)].tobytes()
        assert pipe.collect().tobytes() == lf.expected(half_sc, mb, mask).tobytes()
        assert pipe.collect().tobytes() == want[(mask, mb)].tobytes()
    pipe.close()
    sp = _capi.StreamPipe(rate, 7.0, True, depth=3, lib=lib)
    base = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
    torch.cuda.synchronize()
    cuts = [0, 900_001, 1_700_000, 3_111_111, n]
    chunks = [(base.data_ptr() + 8 * a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    for mask, mb in SETTINGS:
        sp.set_fix_errors(mb)
        sp.set_long_formats(mask)
        assert sp.get_long_formats() == mask
        got = np.concatenate(sp.run(chunks))
        w = want[(mask, mb)]
        assert got.tobytes() == w.tobytes(), "stream pipe, mask %d fix %d: %d vs %d packets" % (mask, mb, len(got), len(w))
    sp.close()
    del base


def test_bank_of_three_receivers(lib):
    """rx_path_bank (am_process_multi) at 20 Msps: receiver j's queue is the definition on its own capture."""
    import air_modes
    iq = capture(20)[0]
    rate = CAPTURES[20][0]
    caps = [iq[:700_000], iq[700_000:1_400_001], iq[1_000_000:]]
    qs = [air_modes.msg_queue() for _ in caps]
    bank = air_modes.rx_path_bank(rate, 7.0, qs, use_pmf=True, device=0, lib=lib, fix_errors=2, long_formats=[18, 19])
    per = bank.work(caps)
    for q, cap, pk in zip(qs, caps, per):
        got = []
        while not q.empty_p():
            got.append(q.delete_head().to_string())
        w = lf.expected(lf.scan(cap, rate), 2, 3)
        assert lf.counts(w)[0] >= 5 and lf.counts(w)[1] >= 3
        assert pk.tobytes() == w.tobytes() and got == oracle.format_messages(w)


def test_gate_interplay_and_time_shards(lib):
    """The address gate in mode 2 with DF18 alone enabled: DF18 kept although it is no DF11 / DF17, DF19 an "other" and dropped,
    everything else as gate_common says.  And the time shards (am_shard_scan / am_shard_resolve, two chunks on one device), which
    the gate does not cover but the option does."""
    iq, sc, want = capture(4)
    rate, n = CAPTURES[4][0], len(iq)
    ttl = gc.ttl_samples(TTL_S, rate)
    w = lf.expected(sc, 2, 1, 2, ttl)
    assert lf.counts(w)[0] >= 20 and lf.counts(w)[2] >= 10 and set(np.unique(w["df"])) <= {11, 17, 18}
    w1 = lf.expected(sc, 2, 1, 1, ttl)                                   # mode 1 keeps the "others": DF19 as a 56-bit fragment
    assert len(w1) > len(w)
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_fix_errors(2)
    ctx.set_long_formats(1)
    for mode, ww in ((2, w), (1, w1)):
        ctx.set_address_gate(mode, TTL_S)
        assert ctx.process_iq(iq, flush=True).tobytes() == ww.tobytes()
        cuts = uneven_cuts(n)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == ww.tobytes()
    ctx.close()
    ctxs = [_capi.Context(rate, 7.0, True, lib=lib) for _ in range(2)]
    for c in ctxs:
        c.set_fix_errors(2)
        c.set_long_formats(3)
    pc.check_sharded(lib, rate, iq, 2, want=want[(3, 2)], ctxs=ctxs)
    for c in ctxs:
        c.close()


def test_off_means_off(lib):
    """A capture of the edge formats as tools/synth.py makes them (DF_MIX_EDGE, address overlay on DF18 / DF19): a context that had
    the option on and then off returns what a fresh context returns, which is what the oracle returns."""
    rate, n = 64e6, 4_000_000
    iq, _ = synth.synth_capture(rate, n, 12000.0, 46, df_mix=synth.DF_MIX_EDGE)
    want = oracle.demod(iq, rate)
    fresh = _capi.Context(rate, 7.0, True, lib=lib)
    a = fresh.process_iq(iq, flush=True)
    fresh.close()
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_long_formats(3)
    on = ctx.process_iq(iq, flush=True)
    assert on.tobytes() == lf.expected(lf.scan(iq, rate), 0, 3).tobytes() and on.tobytes() != want.tobytes()
    ctx.set_long_formats(0)
    b = ctx.process_iq(iq, flush=True)
    ctx.close()
    assert a.tobytes() == b.tobytes() == want.tobytes() and len(want) > 100 and (want["df"] == 18).any()
