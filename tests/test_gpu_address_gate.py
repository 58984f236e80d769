"""Opt-in address gate for address/parity replies (am_set_address_gate) on the device: the slicing kernels' <FIX, 1>
instantiations, the gate kernels behind them (am_gate.inc) and every covered call of the C ABI, byte for byte against the numpy
definition in tests/gate_common.py applied to the oracle's packets."""
import numpy as np
import pytest

import fix_common as fx
import gate_common as gc
import oracle
from air_modes import _capi

pytestmark = pytest.mark.gpu

AP = gc.AP
# fleet captures: (rate, samples, bursts per second, seed, fleet, SNR), the two windows in seconds, and what the definition keeps of
# the oracle's packets: {ttl: (mode 1, mode 2)}
CAPTURES = {64: ((64e6, 16_000_000, 20000.0, 24, 30, (6.0, 30.0)), (60.0, 0.01), 549, {60.0: (369, 361), 0.01: (235, 227)}),
            20: ((20e6, 20_000_000, 5000.0, 23, 60, (6.0, 30.0)), (60.0, 0.02), 2339, {60.0: (2107, 2104), 0.02: (1399, 1396)}),
            4: ((4e6, 4_000_000, 3000.0, 26, 40, (10.0, 35.0)), (60.0, 0.05), None, None)}
_cache = {}


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    oracle.build()
    return hip_lib


def capture(msps):
    """(iq, truth, the oracle's packets); the pinned counts are checked BEFORE the library is asked."""
    if msps not in _cache:
        args, ttls, n_pk, kept = CAPTURES[msps]
        iq, truth, _ = gc.fleet_capture(*args)
        pk = oracle.demod(iq, args[0], 7.0)
        true = gc.transmitted(pk, truth)
        isap = np.isin(pk["df"], AP)
        for ttl_s in ttls:
            k1, k2 = (gc.gate(pk, m, gc.ttl_samples(ttl_s, args[0])) for m in (1, 2))
            print("capture %g Msps, ttl %g s: %d packets -> %d / %d; false AP %d -> %d" % (msps, ttl_s, len(pk), k1.sum(), k2.sum(),
                                                                                        (isap & ~true).sum(), (k1 & isap & ~true).sum()))
            assert not (k1 & isap & ~true).any() and 0 < k2.sum() < k1.sum() < len(pk)
            if kept:
                assert len(pk) == n_pk and (int(k1.sum()), int(k2.sum())) == kept[ttl_s]
        _cache[msps] = (iq, truth, pk)
    return _cache[msps]


def uneven_cuts(n):
    return [0, n // 7 + 1, n // 7 + 2, n // 2 + 13, n - n // 5, n - 333, n]


def drain(q):
    got = []
    while not q.empty_p():
        got.append(q.delete_head().to_string())
    return got


@pytest.mark.parametrize("msps", [64, 20])
def test_production_path_as_defined(lib, msps):
    """am_k_extract_slice_iq<SPC, FIX, 1> + the gate kernels behind the streaming front end: one call, uneven chunks with a
    flush, device input, and the counters."""
    import torch
    iq, truth, pk = capture(msps)
    args, ttls = CAPTURES[msps][:2]
    rate, n = args[0], len(iq)
    if msps == 64:
        assert int((np.isin(pk["df"], AP) & ~gc.transmitted(pk, truth)).sum()) == 143
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    dev = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
    torch.cuda.synchronize()
    stat = dict(taught=0, passed=0, dropped=0, not_learned=0)
    for mode in (0, 1, 2):
        for ttl_s in ttls:
            k = gc.gate(pk, mode, gc.ttl_samples(ttl_s, rate))
            want = pk[k]
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
            if mode:
                for key, v in zip(("taught", "passed", "dropped"), gc.counts(pk, k)):
                    stat[key] += 3 * v
            assert ctx.address_gate_stats() == stat
    ctx.close()
    del dev


def test_with_the_repair_on(lib):
    """<2, 1>: a repaired DF11 / DF17 reply is kept and teaches nothing."""
    iq = capture(20)[0][:8_000_000]
    rate = 20e6
    pk = fx.expected_from_capture(iq, rate, 2)
    assert int(np.count_nonzero(pk["reserved"][:, 1])) >= 20
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_fix_errors(2)
    for mode, ttl_s in ((1, 60.0), (2, 0.02)):
        k = gc.gate(pk, mode, gc.ttl_samples(ttl_s, rate))
        assert k[pk["reserved"][:, 1] > 0].all() and 0 < (~k).sum()
        ctx.set_address_gate(mode, ttl_s)
        assert ctx.process_iq(iq, flush=True).tobytes() == pk[k].tobytes()
        parts = [ctx.process_iq(iq[:3_000_001]), ctx.process_iq(iq[3_000_001:], flush=True)]
        assert np.concatenate(parts).tobytes() == pk[k].tobytes()
    ctx.close()


def test_rx_path_on_cu8_chunks(lib):
    """4 Msps through rx_path on an RTL-SDR's bytes, in chunks: message texts and rx.gated."""
    import air_modes
    from air_modes import formats
    args = CAPTURES[4][0]
    iq, truth, _ = gc.fleet_capture(*args, sigma=0.02)
    raw = np.clip(np.round(iq.view(np.float32) * 127.5 / 2.0 + 127.5), 0, 255).astype(np.uint8)
    pk = oracle.demod(formats.to_cf32(raw, "cu8"), 4e6, 7.0)
    assert len(pk) > 1000
    for mode, ttl_s in ((0, 60.0), (1, 60.0), (2, 0.05)):
        k = gc.gate(pk, mode, gc.ttl_samples(ttl_s, 4e6))
        assert mode == 0 or 0 < (~k).sum() < len(pk)
        q = air_modes.msg_queue()
        rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, device=0, lib=lib, address_gate=mode, address_ttl=ttl_s)
        cuts = [0, 2 * 700_001, 2 * 700_002, 2 * 2_500_000, raw.size]
        for a, b in zip(cuts[:-1], cuts[1:]):
            rx.work(raw[a:b], flush=(b == raw.size))
        assert drain(q) == oracle.format_messages(pk[k])
        assert rx.packets == int(k.sum()) and rx.gated == int((~k).sum())


def test_slicer_block_alone(lib):
    """am_slicer_work -> am_k_slice<FIX, 1>: the map carries over from call to call until am_reset."""
    iq = capture(20)[0][:8_000_000]
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, 10, True), 10, 7.0, 20e6)
    want = oracle.slice_bursts(bursts, tags)
    ctx = _capi.Context(20e6, 7.0, True, lib=lib)
    for mode, ttl_s in ((0, 60.0), (1, 60.0), (2, 0.02), (1, 0.002)):
        k = gc.gate(want, mode, gc.ttl_samples(ttl_s, 20e6))
        ctx.set_address_gate(mode, ttl_s)
        ctx.reset()
        assert ctx.slicer_work(bursts, tags).tobytes() == want[k].tobytes()
        ctx.reset()
        h = len(tags) // 3
        got = np.concatenate([ctx.slicer_work(bursts[:h], tags[:h]), ctx.slicer_work(bursts[h:], tags[h:])])
        assert got.tobytes() == want[k].tobytes()
    ctx.close()


def test_pipe(lib):
    """am_pipe at 64 Msps: every batch is a whole stream with a map of its own."""
    iq, truth, pk = capture(64)
    rate, n = 64e6, len(iq)
    half = iq[:n // 2 + 5]
    pk_half = oracle.demod(half, rate, 7.0)
    pipe = _capi.Pipe(rate, 7.0, True, depth=3, lib=lib)
    for mode, ttl_s in ((2, 0.01), (1, 60.0), (0, 60.0)):
        ttl = gc.ttl_samples(ttl_s, rate)
        pipe.set_address_gate(mode, ttl_s)
        assert pipe.get_address_gate() == (mode, ttl_s)
        pipe.submit(iq)
        with pytest.raises(_capi.AirModesError):
            pipe.set_address_gate(1, 1.0)
        pipe.submit(half)
        pipe.submit(iq)
        want = pk[gc.gate(pk, mode, ttl)]
        assert pipe.collect().tobytes() == want.tobytes()
        assert pipe.collect().tobytes() == pk_half[gc.gate(pk_half, mode, ttl)].tobytes()
        assert pipe.collect().tobytes() == want.tobytes()
    pipe.close()


def test_streams_of_one_scan_do_not_share_aircraft(lib):
    """am_process_multi / am_submit_multi / rx_path_bank at 20 Msps: three captures of ONE fleet; B holds only address/parity
    frames and must keep none of them, whatever A and C teach in the same scan."""
    import air_modes
    rate = 20e6
    iq_a, _, fleet = gc.fleet_capture(rate, 5_000_000, 5000.0, 41, 20)
    only_ap = tuple((d, 1.0) for d in (0, 4, 5, 20, 21))
    iq_b = gc.fleet_capture(rate, 4_000_001, 5000.0, 42, 20, fleet=fleet, mix=only_ap)[0]
    iq_c = gc.fleet_capture(rate, 4_500_000, 5000.0, 43, 20, fleet=fleet)[0]
    caps = [iq_a, iq_b, iq_c]
    pks = [oracle.demod(x, rate, 7.0) for x in caps]
    assert int(np.isin(pks[1]["df"], AP).sum()) > 300
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    buf, lens = ctx.multi_pack(caps)
    for mode, ttl_s in ((0, 60.0), (1, 60.0), (2, 0.02)):
        ttl = gc.ttl_samples(ttl_s, rate)
        ctx.set_address_gate(mode, ttl_s)
        keeps = [gc.gate(p, mode, ttl) for p in pks]
        if mode:
            assert not np.isin(pks[1][keeps[1]]["df"], AP).any() and keeps[0].sum() > 300
        before = ctx.address_gate_stats()
        for got in (ctx.process_multi(buf, lens), (ctx.submit_multi(buf, lens), ctx.collect_multi())[1]):
            for g, p, k in zip(got, pks, keeps):
                assert g.tobytes() == p[k].tobytes(), (mode, ttl_s)
        after = ctx.address_gate_stats()
        if mode:
            tot = np.sum([gc.counts(p, k) for p, k in zip(pks, keeps)], axis=0)
            assert [after[x] - before[x] for x in ("taught", "passed", "dropped")] == [2 * int(v) for v in tot]
    ctx.close()
    qs = [air_modes.msg_queue() for _ in caps]
    air_modes.rx_path_bank(rate, 7.0, qs, use_pmf=True, device=0, lib=lib, address_gate=1, address_ttl=0.02).work(caps)
    for q, p in zip(qs, pks):
        assert drain(q) == oracle.format_messages(p[gc.gate(p, 1, gc.ttl_samples(0.02, rate))])


def test_fractional_rate(lib):
    """5 Msps: the rate-generic kernels, am_k_extract_slice<FIX, 1>."""
    iq, truth, _ = gc.fleet_capture(5e6, 3_000_000, 3000.0, 27, 30)
    pk = oracle.demod(iq, 5e6, 7.0)
    ctx = _capi.Context(5e6, 7.0, True, lib=lib)
    for mode, ttl_s in ((1, 60.0), (2, 0.03)):
        k = gc.gate(pk, mode, gc.ttl_samples(ttl_s, 5e6))
        assert 0 < (~k).sum() < len(pk)
        ctx.set_address_gate(mode, ttl_s)
        assert ctx.process_iq(iq, flush=True).tobytes() == pk[k].tobytes()
        assert ctx.last_frontend() == 1
        n = len(iq)
        cuts = uneven_cuts(n)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == pk[k].tobytes()
    ctx.close()


def test_off_means_off(lib):
    """A context that had the gate on and then off returns what a fresh context returns, which is what the oracle returns."""
    iq, truth, pk = capture(64)
    fresh = _capi.Context(64e6, 7.0, True, lib=lib)
    a = fresh.process_iq(iq, flush=True)
    fresh.close()
    ctx = _capi.Context(64e6, 7.0, True, lib=lib)
    ctx.set_address_gate(2, 0.01)
    on = ctx.process_iq(iq, flush=True)
    assert len(on) == 227
    ctx.set_address_gate(0, 0.01)
    b = ctx.process_iq(iq, flush=True)
    ctx.close()
    assert a.tobytes() == b.tobytes() == pk.tobytes()
