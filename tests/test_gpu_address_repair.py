"""Opt-in repair of one wrong bit in an address/parity reply (am_set_address_repair) on the device: the slicing kernels' <FIX, 2>
instantiations, am_k_gate_test<1> and am_k_gate_repair behind them (am_gate.inc) and every covered call of the C ABI, byte for
byte against the numpy definition in tests/aprepair_common.py applied to the oracle's packets."""
import numpy as np
import pytest

import aprepair_common as ar
import gate_common as gc
import oracle
from air_modes import _capi

pytestmark = pytest.mark.gpu

AP = gc.AP
# fleet captures: (rate, samples, bursts per second, seed, fleet, SNR), how many of its samples are used, and what the definition
# repairs of the oracle's packets: {ttl in seconds: repaired}
CAPTURES = {64: ((64e6, 16_000_000, 20000.0, 24, 30, (6.0, 30.0)), 16_000_000, {60.0: 8, 0.01: 1}),
            20: ((20e6, 20_000_000, 5000.0, 23, 60, (6.0, 30.0)), 8_000_000, {60.0: 4}),
            5: ((5e6, 3_000_000, 3000.0, 27, 30, (4.0, 14.0)), 3_000_000, {60.0: 25})}
_cache = {}


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    oracle.build()
    return hip_lib


def capture(msps):
    """(iq, truth, the oracle's packets); the definition's own counts are pinned BEFORE the library is asked."""
    if msps not in _cache:
        args, n, repaired = CAPTURES[msps]
        iq, truth, _ = gc.fleet_capture(*args)
        iq = np.ascontiguousarray(iq[:n])
        pk = oracle.demod(iq, args[0], 7.0)
        for ttl_s, want in repaired.items():
            out, keep, fixed, amb = ar.repair(pk, 1, gc.ttl_samples(ttl_s, args[0]))
            rep = out[out["reserved"][:, 1] != 0]
            print("capture %g Msps, ttl %g s: %d packets, %d kept, %d repaired (%d transmitted), %d ambiguous"
                  % (msps, ttl_s, len(pk), keep.sum(), len(rep), gc.transmitted(rep, truth).sum(), amb))
            assert len(rep) == want and want >= 1 and amb == 0 and gc.transmitted(rep, truth).all()
        _cache[msps] = (iq, truth, pk)
    return _cache[msps]


def uneven_cuts(n):
    return [0, n // 7 + 1, n // 7 + 2, n // 2 + 13, n - n // 5, n - 333, n]


def drain(q):
    got = []
    while not q.empty_p():
        got.append(q.delete_head().to_string())
    return got


def repair_ctx(lib, rate, mode=1, ttl_s=60.0, on=1):
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_address_gate(mode, ttl_s)
    ctx.set_address_repair(on)
    return ctx


@pytest.mark.parametrize("msps", [64, 20])
def test_production_path_as_defined(lib, msps):
    """am_k_extract_slice_iq<SPC, FIX, 2> + the gate and repair kernels behind the streaming front end: one call, uneven chunks
    with a flush, device input, and the counters."""
    import torch
    iq, truth, pk = capture(msps)
    args, _, repaired = CAPTURES[msps]
    rate, n = args[0], len(iq)
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_address_repair(1)
    dev = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
    torch.cuda.synchronize()
    gstat = dict(taught=0, passed=0, dropped=0, not_learned=0)
    rstat = dict(repaired=0, ambiguous=0)
    for mode in (1, 2):
        for ttl_s in repaired:
            want, keep, fixed, amb = ar.repair(pk, mode, gc.ttl_samples(ttl_s, rate))
            assert int((fixed >= 0).sum()) == repaired[ttl_s]
            ctx.set_address_gate(mode, ttl_s)
            got = ctx.process_iq(iq, flush=True)
            assert ctx.last_frontend() == 3
            assert got.tobytes() == want.tobytes(), "mode %d ttl %g: %d vs %d packets" % (mode, ttl_s, len(got), len(want))
            assert lib.format_messages(got, True) == oracle.format_messages(want)
            cuts = uneven_cuts(n)
            parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.concatenate(parts).tobytes() == want.tobytes()
            parts = [ctx.process_iq_device(dev.data_ptr() + 8 * a, b - a, flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.concatenate(parts).tobytes() == want.tobytes()
            c = ar.counts(pk, keep, fixed)
            for key, v in zip(("taught", "passed", "dropped"), c[:3]):
                gstat[key] += 3 * v
            rstat["repaired"] += 3 * c[3]
            assert ctx.address_gate_stats() == gstat and ctx.address_repair_stats() == rstat
    ctx.close()
    del dev


def test_fractional_rate(lib):
    """5 Msps, SNR 4-14 dB: the rate-generic kernels, am_k_extract_slice<FIX, 2>.  25 repaired."""
    iq, truth, pk = capture(5)
    n = len(iq)
    ctx = repair_ctx(lib, 5e6)
    want, keep, fixed, amb = ar.repair(pk, 1, gc.ttl_samples(60.0, 5e6))
    assert int((fixed >= 0).sum()) == 25
    assert ctx.process_iq(iq, flush=True).tobytes() == want.tobytes()
    assert ctx.last_frontend() == 1
    cuts = uneven_cuts(n)
    parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts).tobytes() == want.tobytes()
    assert ctx.address_repair_stats() == dict(repaired=50, ambiguous=0)
    ctx.close()


def test_slicer_block_alone(lib):
    """am_slicer_work -> am_k_slice<FIX, 2>: the map carries across two calls, and the second call's replies are repaired from
    what the first one taught."""
    iq, truth, pk = capture(20)
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, 10, True), 10, 7.0, 20e6)
    assert oracle.slice_bursts(bursts, tags).tobytes() == pk.tobytes()
    ctx = repair_ctx(lib, 20e6)
    for mode, ttl_s in ((1, 60.0), (2, 60.0)):
        want, keep, fixed, amb = ar.repair(pk, mode, gc.ttl_samples(ttl_s, 20e6))
        ctx.set_address_gate(mode, ttl_s)
        ctx.reset()
        assert ctx.slicer_work(bursts, tags).tobytes() == want.tobytes()
        ctx.reset()
        h = len(tags) // 3
        assert int((fixed >= 0).sum()) == 4 and (fixed[pk["sample"] >= tags["sample"][h]] >= 0).any()
        got = np.concatenate([ctx.slicer_work(bursts[:h], tags[:h]), ctx.slicer_work(bursts[h:], tags[h:])])
        assert got.tobytes() == want.tobytes()
    assert ctx.address_repair_stats() == dict(repaired=16, ambiguous=0)
    ctx.close()


def test_pipe(lib):
    """am_pipe at 64 Msps: every batch is a whole stream with a map of its own."""
    iq, truth, pk = capture(64)
    rate, n = 64e6, len(iq)
    half = iq[:n // 2 + 5]
    pk_half = oracle.demod(half, rate, 7.0)
    pipe = _capi.Pipe(rate, 7.0, True, depth=3, lib=lib)
    pipe.set_address_repair(1)
    for mode, ttl_s, n_half in ((1, 60.0, 6), (2, 0.01, 1)):
        ttl = gc.ttl_samples(ttl_s, rate)
        pipe.set_address_gate(mode, ttl_s)
        want = ar.repair(pk, mode, ttl)[0]
        want_half, _, fixed_half, _ = ar.repair(pk_half, mode, ttl)
        assert int((fixed_half >= 0).sum()) == n_half
        pipe.submit(iq)
        with pytest.raises(_capi.AirModesError):
            pipe.set_address_repair(0)
        pipe.submit(half)
        pipe.submit(iq)
        assert pipe.collect().tobytes() == want.tobytes()
        assert pipe.collect().tobytes() == want_half.tobytes()
        assert pipe.collect().tobytes() == want.tobytes()
    pipe.close()


def test_streams_of_one_scan_search_their_own_map(lib):
    """am_process_multi / am_submit_multi at 20 Msps: three captures of ONE fleet at SNR 4-14 dB; B holds only address/parity
    frames and must repair none of them, whatever A and C teach in the same scan."""
    rate = 20e6
    snr = (4.0, 14.0)
    iq_a, _, fleet = gc.fleet_capture(rate, 3_000_000, 5000.0, 41, 20, snr)
    only_ap = tuple((d, 1.0) for d in (0, 4, 5, 20, 21))
    iq_b = gc.fleet_capture(rate, 2_000_001, 5000.0, 42, 20, snr, fleet=fleet, mix=only_ap)[0]
    iq_c = gc.fleet_capture(rate, 2_500_000, 5000.0, 43, 20, snr, fleet=fleet)[0]
    caps = [iq_a, iq_b, iq_c]
    pks = [oracle.demod(x, rate, 7.0) for x in caps]
    assert int(np.isin(pks[1]["df"], AP).sum()) > 200
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_address_repair(1)
    buf, lens = ctx.multi_pack(caps)
    for mode, ttl_s, n_rep in ((1, 60.0, [6, 0, 3]), (2, 0.02, [5, 0, 3])):
        ttl = gc.ttl_samples(ttl_s, rate)
        ctx.set_address_gate(mode, ttl_s)
        exp = [ar.repair(p, mode, ttl) for p in pks]
        assert [int((e[2] >= 0).sum()) for e in exp] == n_rep
        assert not np.isin(exp[1][0]["df"], AP).any()
        before = ctx.address_repair_stats()
        for got in (ctx.process_multi(buf, lens), (ctx.submit_multi(buf, lens), ctx.collect_multi())[1]):
            for g, e in zip(got, exp):
                assert g.tobytes() == e[0].tobytes(), (mode, ttl_s)
        after = ctx.address_repair_stats()
        assert after["repaired"] - before["repaired"] == 2 * sum(n_rep) and after["ambiguous"] == 0
    ctx.close()


def test_rx_path_on_cu8_chunks(lib):
    """4 Msps through rx_path on an RTL-SDR's bytes at SNR 4-14 dB, in chunks: message texts, rx.repaired and rx.gated."""
    import air_modes
    from air_modes import formats
    iq, truth, _ = gc.fleet_capture(4e6, 4_000_000, 3000.0, 26, 40, (4.0, 14.0), sigma=0.02)
    raw = np.clip(np.round(iq.view(np.float32) * 127.5 / 2.0 + 127.5), 0, 255).astype(np.uint8)
    pk = oracle.demod(formats.to_cf32(raw, "cu8"), 4e6, 7.0)
    for mode, ttl_s, n_rep in ((1, 60.0, 43), (2, 0.05, 15)):
        want, keep, fixed, amb = ar.repair(pk, mode, gc.ttl_samples(ttl_s, 4e6))
        assert int((fixed >= 0).sum()) == n_rep and gc.transmitted(want[want["reserved"][:, 1] != 0], truth).all()
        q = air_modes.msg_queue()
        rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, device=0, lib=lib, address_gate=mode, address_ttl=ttl_s,
                               address_repair=1)
        cuts = [0, 2 * 700_001, 2 * 700_002, 2 * 2_500_000, raw.size]
        for a, b in zip(cuts[:-1], cuts[1:]):
            rx.work(raw[a:b], flush=(b == raw.size))
        assert drain(q) == oracle.format_messages(want)
        assert rx.packets == len(want) and rx.repaired == n_rep and rx.gated == int((~keep).sum())


def test_off_means_off(lib):
    """A context that had the repair on and then has it off returns what a fresh gate-only context returns."""
    iq, truth, pk = capture(64)
    fresh = _capi.Context(64e6, 7.0, True, lib=lib)
    fresh.set_address_gate(1, 60.0)
    a = fresh.process_iq(iq, flush=True)
    fresh.close()
    ctx = repair_ctx(lib, 64e6)
    on = ctx.process_iq(iq, flush=True)
    assert len(on) == len(a) + 8
    ctx.set_address_repair(0)
    b = ctx.process_iq(iq, flush=True)
    assert ctx.address_repair_stats() == dict(repaired=8, ambiguous=0)
    ctx.set_address_repair(1)
    ctx.set_address_gate(0, 60.0)
    c = ctx.process_iq(iq, flush=True)
    ctx.close()
    assert a.tobytes() == b.tobytes() == pk[gc.gate(pk, 1, gc.ttl_samples(60.0, 64e6))].tobytes()
    assert c.tobytes() == pk.tobytes()
