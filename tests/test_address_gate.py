"""Opt-in address gate for address/parity replies (am_set_address_gate), without a GPU: the definition (tests/gate_common.py)
against the oracle, what the gate is for, expiry, and the library -- the product sources under the CPU emulation -- against the
definition: every slicing path, byte for byte."""
import numpy as np
import pytest

import fix_common as fx
import gate_common as gc
import oracle
import synth
from air_modes import _capi

AP = gc.AP


@pytest.fixture(scope="module")
def cap_a():
    """4 Msps, 2 s, 3 000 bursts/s of a fleet of 40, SNR 10-35 dB."""
    oracle.build()
    iq, truth, fleet = gc.fleet_capture(4e6, 8_000_000, 3000.0, 21, 40)
    return iq, truth, oracle.demod(iq, 4e6, 7.0)


@pytest.fixture(scope="module")
def cap_b():
    """The same at SNR 4-14 dB, 4 000 bursts/s."""
    oracle.build()
    iq, truth, fleet = gc.fleet_capture(4e6, 8_000_000, 4000.0, 22, 40, (4.0, 14.0))
    return iq, truth, oracle.demod(iq, 4e6, 7.0)


@pytest.fixture(scope="module")
def small():
    """4 Msps, 0.5 s of the fleet: what the emulated library is run on.  (iq, truth, the oracle's packets)"""
    oracle.build()
    iq, truth, fleet = gc.fleet_capture(4e6, 2_000_000, 3000.0, 21, 40)
    return iq, truth, oracle.demod(iq, 4e6, 7.0)


def expected(iq, rate, mode, ttl_s, fix=0):
    pk = fx.expected_from_capture(iq, rate, fix) if fix else oracle.demod(iq, rate, 7.0)
    keep = gc.gate(pk, mode, gc.ttl_samples(ttl_s, rate))
    return pk, keep


def drain(q):
    got = []
    while not q.empty_p():
        got.append(q.delete_head().to_string())
    return got


# ---- 1. the definition against the oracle ----------------------------------------------------------------------------------
def test_definition_against_the_oracle(small):
    iq, truth, pk = small
    assert len(pk) == 929
    assert gc.gate(pk, 0, 1).all()
    for ttl in (gc.ttl_samples(60.0, 4e6), 200_000, 20_000, 1):
        k1, k2 = gc.gate(pk, 1, ttl), gc.gate(pk, 2, ttl)
        for k in (k1, k2):
            assert gc.is_subsequence(pk[k], pk)
            assert gc.brute_force_ok(pk, k, ttl)                     # no kept AP packet without a teach inside the window
        assert not (k2 & ~k1).any()                                  # mode 2 only drops more
        assert np.isin(pk[k2]["df"], (0, 4, 5, 11, 16, 17, 20, 21)).all()
        assert (k1 == k2)[np.isin(pk["df"], (11, 17) + AP)].all()
    assert gc.gate(pk, 1, 1).sum() < gc.gate(pk, 1, 20_000).sum() < gc.gate(pk, 1, 200_000).sum() < len(pk)


# ---- 2. what it is for ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,n_pk,n_ap,n_false,n_true,kept_true,kept1,kept2",
                         [("a", 3622, 1839, 155, 1684, 1652, 3435, 3431), ("b", 2176, 1266, 432, 834, 806, 1716, 1693)])
def test_false_replies_go_true_ones_stay(cap_a, cap_b, which, n_pk, n_ap, n_false, n_true, kept_true, kept1, kept2):
    iq, truth, pk = cap_a if which == "a" else cap_b
    true = gc.transmitted(pk, truth)
    isap = np.isin(pk["df"], AP)
    assert (len(pk), int(isap.sum()), int((isap & ~true).sum()), int((isap & true).sum())) == (n_pk, n_ap, n_false, n_true)
    assert not (~true & np.isin(pk["df"], (11, 17))).any()          # 24-bit parity: DF11 / DF17 never make a false frame
    ttl = gc.ttl_samples(60.0, 4e6)
    for mode, kept in ((1, kept1), (2, kept2)):
        k = gc.gate(pk, mode, ttl)
        assert not (k & isap & ~true).any()                          # no kept AP packet is a frame that was not transmitted
        assert (k & isap & true).sum() >= 0.95 * (isap & true).sum()
        assert int((k & isap & true).sum()) == kept_true and int(k.sum()) == kept
    assert np.isin(pk[gc.gate(pk, 2, ttl)]["df"], (0, 4, 5, 11, 16, 17, 20, 21)).all()


def test_noise_alone():
    """No transmission at all, 5 dB threshold (the GUI default): what comes out with the gate off is all fiction."""
    oracle.build()
    iq, truth, _ = gc.fleet_capture(4e6, 8_000_000, 0.0, 3, 40)
    pk = oracle.demod(iq, 4e6, 5.0)
    assert len(truth) == 0 and len(pk) == 118 and int(np.isin(pk["df"], AP).sum()) == 46
    ttl = gc.ttl_samples(60.0, 4e6)
    k1, k2 = gc.gate(pk, 1, ttl), gc.gate(pk, 2, ttl)
    assert int(k1.sum()) == 72 and not np.isin(pk[k1]["df"], AP).any()
    assert int(k2.sum()) == 0


# ---- 3. expiry -------------------------------------------------------------------------------------------------------------------
def test_expiry(cap_a, cap_b):
    for (iq, truth, pk), kept in ((cap_a, 1103), (cap_b, 328)):
        true = gc.transmitted(pk, truth)
        isap = np.isin(pk["df"], AP)
        k = gc.gate(pk, 1, gc.ttl_samples(0.05, 4e6))
        assert gc.ttl_samples(0.05, 4e6) == 200_000
        assert int((k & isap & true).sum()) == kept and not (k & isap & ~true).any()


def test_expiry_20msps():
    oracle.build()
    iq, truth, _ = gc.fleet_capture(20e6, 20_000_000, 5000.0, 23, 60, (6.0, 30.0))
    pk = oracle.demod(iq, 20e6, 7.0)
    true = gc.transmitted(pk, truth)
    isap = np.isin(pk["df"], AP)
    assert len(pk) == 2339
    k = gc.gate(pk, 1, gc.ttl_samples(0.02, 20e6))
    assert int((k & isap & true).sum()) == 325 and not (k & isap & ~true).any() and int(k.sum()) == 1399
    assert int(gc.gate(pk, 1, gc.ttl_samples(60.0, 20e6)).sum()) == 2107


def hand_made(samples_and_frames):
    """Clean bursts (chips 0 / 1) of the given frames at the given item counts."""
    b = np.zeros((len(samples_and_frames), 240), np.float32)
    t = np.zeros(len(samples_and_frames), oracle.TAG_DTYPE)
    for i, (s, frame) in enumerate(samples_and_frames):
        chips = synth.frame_chips(frame)
        b[i, :chips.size] = chips
        t[i]["sample"] = s
    return b, t


def test_window_edge_through_slicer_work(emu_lib):
    """Teach / test pairs exactly ttl_samples and ttl_samples + 1 apart, in one call and across calls."""
    oracle.build()
    rng = np.random.default_rng(5)
    a1, a2, a3 = 0x4840D6, 0xABCDEF, 0x000001
    ttl_s, rate = 0.001, 4e6
    T = gc.ttl_samples(ttl_s, rate)
    assert T == 4000
    seq = [(1000, gc.fleet_frame(rng, 17, a1)), (1000 + T, gc.fleet_frame(rng, 20, a1)),          # exactly ttl: kept
           (1500, gc.fleet_frame(rng, 11, a2)), (1500 + T + 1, gc.fleet_frame(rng, 4, a2)),      # one more: dropped
           (9000, gc.fleet_frame(rng, 0, a3)),                                                   # never taught: dropped
           (9500, gc.fleet_frame(rng, 17, a3)), (9600, gc.fleet_frame(rng, 5, a3)),              # taught in front of it: kept
           (9700, gc.fleet_frame(rng, 21, a1)),                                                  # a1 is too old by now
           (9800, gc.fleet_frame(rng, 18, a1))]                                                  # neither: mode 2 drops it
    seq.sort(key=lambda x: x[0])
    b, t = hand_made(seq)
    pk = oracle.slice_bursts(b, t)
    assert len(pk) == len(seq) and sorted(pk["df"].tolist()) == [0, 4, 5, 11, 17, 17, 18, 20, 21]
    ctx = _capi.Context(rate, 7.0, True, lib=emu_lib)
    for mode in (1, 2):
        ctx.set_address_gate(mode, ttl_s)
        k = gc.gate(pk, mode, T)
        assert pk[k]["df"].tolist() == [17, 11, 20, 17, 5] + ([18] if mode == 1 else [])
        ctx.reset()
        assert ctx.slicer_work(b, t).tobytes() == pk[k].tobytes()
        # the map carries over from call to call ...
        ctx.reset()
        for cut in (1, 2, 3, 6):
            ctx.reset()
            got = np.concatenate([ctx.slicer_work(b[:cut], t[:cut]), ctx.slicer_work(b[cut:], t[cut:])])
            assert got.tobytes() == pk[k].tobytes(), cut
        # ... until am_reset
        ctx.reset()
        ctx.slicer_work(b[:1], t[:1])
        ctx.reset()
        assert 20 not in ctx.slicer_work(b[1:], t[1:])["df"].tolist()
    ctx.close()


# ---- 4. library == definition ----------------------------------------------------------------------------------------------------
def test_slicer_work_on_a_capture(emu_lib, small):
    iq, truth, pk = small
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, 2, True), 2, 7.0, 4e6)
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    for fix in (0, 2):
        want = fx.slice_fix(bursts, tags, fix)[0]
        if not fix:
            assert want.tobytes() == pk.tobytes()
        ctx.set_fix_errors(fix)
        for mode in (0, 1, 2):
            for ttl_s in (60.0, 0.005):
                ctx.set_address_gate(mode, ttl_s)
                ctx.reset()
                k = gc.gate(want, mode, gc.ttl_samples(ttl_s, 4e6))
                assert ctx.slicer_work(bursts, tags).tobytes() == want[k].tobytes(), (fix, mode, ttl_s)
    ctx.close()


def test_whole_path_as_defined(emu_lib, small):
    """One call; uneven chunks with a flush (many windows in one call, one window across several calls); a second stream
    behind the flush starts with an empty map; the counters."""
    iq, truth, pk0 = small
    n = len(iq)
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    stat = dict(taught=0, passed=0, dropped=0, not_learned=0)
    assert ctx.address_gate_stats() == stat
    for fix in (0, 2):
        ctx.set_fix_errors(fix)
        for mode in (0, 1, 2):
            for ttl_s in ((60.0, 0.05, 0.002) if not fix else (0.002,)):
                pk, k = expected(iq, 4e6, mode, ttl_s, fix)
                want = pk[k]
                if mode == 0:
                    assert len(want) == len(pk) and (fix or want.tobytes() == pk0.tobytes())
                else:
                    assert 0 < len(want) < len(pk)
                ctx.set_address_gate(mode, ttl_s)
                assert ctx.process_iq(iq, flush=True).tobytes() == want.tobytes(), (fix, mode, ttl_s)
                for cuts in ([0, 70_001, 70_002, 811_117, 1_500_000, n - 333, n], [0, 1_000_000, 1_003_000, 1_009_000, 1_011_111, n]):
                    parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
                    assert np.concatenate(parts).tobytes() == want.tobytes(), (fix, mode, ttl_s, cuts)
                if mode:
                    for key, v in zip(("taught", "passed", "dropped"), gc.counts(pk, k)):
                        stat[key] += 3 * v
                assert ctx.address_gate_stats() == stat
    ctx.close()


def test_small_capacity_and_fetch(emu_lib, small):
    iq, truth, pk = small
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    ctx.set_address_gate(2, 0.05)
    want = pk[gc.gate(pk, 2, 200_000)]
    assert ctx.process_iq(iq, flush=True, capacity=8).tobytes() == want.tobytes()      # AM_ECAPACITY + am_fetch_packets
    ctx.close()


def test_native_samples(emu_lib):
    """process_samples on cu8, as an RTL-SDR delivers them: the oracle on the widened samples, then the definition."""
    from air_modes import formats
    oracle.build()
    iq, truth, fleet = gc.fleet_capture(4e6, 1_000_000, 3000.0, 25, 20, sigma=0.02)
    raw = np.clip(np.round(iq.view(np.float32) * 127.5 / 2.0 + 127.5), 0, 255).astype(np.uint8)
    plain = oracle.demod(formats.to_cf32(raw, "cu8"), 4e6, 7.0)
    assert len(plain) > 100
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    for mode in (0, 1, 2):
        ctx.set_address_gate(mode, 0.05)
        k = gc.gate(plain, mode, 200_000)
        assert mode == 0 or 0 < k.sum() < len(plain)
        assert ctx.process_samples(raw, flush=True).tobytes() == plain[k].tobytes()
        parts = [ctx.process_samples(raw[:2 * 400_001]), ctx.process_samples(raw[2 * 400_001:], flush=True)]
        assert np.concatenate(parts).tobytes() == plain[k].tobytes()
    ctx.close()


def test_fractional_rate(emu_lib):
    """5 Msps, 2.5 samples per chip: the rate-generic kernels (am_k_extract_slice<FIX, 1>, chip table) and the generator's
    area-sampled chips."""
    oracle.build()
    iq, truth, _ = gc.fleet_capture(5e6, 1_500_000, 3000.0, 27, 30)
    pk = oracle.demod(iq, 5e6, 7.0)
    assert len(pk) > 300
    ctx = _capi.Context(5e6, 7.0, True, lib=emu_lib)
    for mode, ttl_s in ((1, 60.0), (2, 0.03)):
        k = gc.gate(pk, mode, gc.ttl_samples(ttl_s, 5e6))
        assert 0 < (~k).sum() < len(pk)
        ctx.set_address_gate(mode, ttl_s)
        assert ctx.process_iq(iq, flush=True).tobytes() == pk[k].tobytes()
        assert ctx.last_frontend() == 1
        parts = [ctx.process_iq(iq[:600_001]), ctx.process_iq(iq[600_001:], flush=True)]
        assert np.concatenate(parts).tobytes() == pk[k].tobytes()
    ctx.close()


def test_what_empties_the_map(emu_lib, small):
    """A second stream behind a flush, am_reset and am_set_rate start with an empty map; am_set_address_gate keeps it."""
    iq, truth, pk = small
    half = len(iq) // 2
    ttl = gc.ttl_samples(60.0, 4e6)
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    ctx.set_address_gate(1, 60.0)
    first = oracle.demod(iq[:half], 4e6, 7.0)
    second = oracle.demod(iq[half:], 4e6, 7.0)
    want2 = second[gc.gate(second, 1, ttl)]
    # carried over inside a stream: the second half knows the first half's aircraft
    whole = np.concatenate([ctx.process_iq(iq[:half]), ctx.process_iq(iq[half:], flush=True)])
    assert whole.tobytes() == pk[gc.gate(pk, 1, ttl)].tobytes()
    n_second_in_stream = int((whole["sample"] >= half + 2).sum())
    assert n_second_in_stream > len(want2)                            # (the test has teeth: an empty map keeps fewer)
    # flush
    ctx.process_iq(iq[:half], flush=True)
    assert ctx.process_iq(iq[half:], flush=True).tobytes() == want2.tobytes()
    # am_reset
    ctx.process_iq(iq[:half])
    ctx.reset()
    assert ctx.process_iq(iq[half:], flush=True).tobytes() == want2.tobytes()
    # am_set_rate
    ctx.process_iq(iq[:half])
    ctx.set_rate(4e6)
    assert ctx.get_address_gate() == (1, 60.0)
    assert ctx.process_iq(iq[half:], flush=True).tobytes() == want2.tobytes()
    # am_set_address_gate in the middle of a stream keeps the map
    a = ctx.process_iq(iq[:half])
    ctx.set_address_gate(2, 30.0)
    ctx.set_address_gate(1, 60.0)
    b = ctx.process_iq(iq[half:], flush=True)
    assert np.concatenate([a, b]).tobytes() == whole.tobytes()
    ctx.close()


def test_rx_path_texts_and_counters(emu_lib, small):
    """Message texts == format_messages(kept), also when the stream's first packet is gated out: the first message POSTED is
    the first one formatted (six significant digits, then ten)."""
    import air_modes
    iq, truth, pk = small
    for mode, ttl_s in ((0, 60.0), (1, 60.0), (2, 0.05)):
        k = gc.gate(pk, mode, gc.ttl_samples(ttl_s, 4e6))
        q = air_modes.msg_queue()
        rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, lib=emu_lib, address_gate=mode, address_ttl=ttl_s)
        assert rx.get_address_gate() == (mode, ttl_s)
        rx.work(iq[:900_001])
        rx.work(iq[900_001:], flush=True)
        assert drain(q) == oracle.format_messages(pk[k])
        assert rx.packets == int(k.sum()) and rx.gated == int((~k).sum())
    # a stream whose first packet is an address/parity reply of an unknown aircraft
    for i in np.flatnonzero(np.isin(pk["df"], AP))[:20]:
        sub = np.ascontiguousarray(iq[int(pk[i]["sample"]) - 2000:])
        want = oracle.demod(sub, 4e6, 7.0)
        if int(want[0]["df"]) in AP:
            break
    k = gc.gate(want, 1, gc.ttl_samples(60.0, 4e6))
    assert int(want[0]["df"]) in AP and not k[0] and k.sum() > 10
    q = air_modes.msg_queue()
    rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, lib=emu_lib)
    rx.set_address_gate(1)
    rx.work(sub, flush=True)
    assert drain(q) == oracle.format_messages(want[k])


# ---- 5. a repeated scan does not teach ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8e6, 64e6])
def test_repeated_scan_does_not_teach(emu_lib, monkeypatch, rate):
    """AIRMODES_SPEC_FLOOR=0, a quiet stretch and then a dense one: the dense scan overflows the capacity it was launched for
    and is redone.  What its first, incomplete try sliced is not the stream's: packets == definition, and the
    non-speculative path agrees."""
    monkeypatch.setenv("AIRMODES_SPEC_FLOOR", "0")
    oracle.build()
    fleet = gc.fleet_capture(rate, 1000, 0.0, 610, 12)[2]
    quiet = gc.fleet_capture(rate, 600_000, 40.0 * rate / 8e6, 611, 12, fleet=fleet)[0]
    busy = gc.fleet_capture(rate, 900_000, 20000.0 * (1.0 if rate == 8e6 else 1.5), 612, 12, fleet=fleet)[0]
    iq = np.concatenate([quiet, busy])
    pk = oracle.demod(iq, rate, 7.0, True)
    ttl_s = 20_000 / 8e6
    k = gc.gate(pk, 1, gc.ttl_samples(ttl_s, rate))
    assert 0 < (~k).sum() and k.sum() > (40 if rate == 8e6 else 8)
    assert (k & np.isin(pk["df"], AP)).sum() > 0
    ctx = _capi.Context(rate, 7.0, True, lib=emu_lib)
    ctx.set_address_gate(1, ttl_s)
    got = [ctx.process_iq(iq[:300000]), ctx.process_iq(iq[300000:600000])]
    m_quiet = ctx.last_num_candidates()
    got.append(ctx.process_iq(iq[600000:1100000]))
    m_busy = ctx.last_num_candidates()
    got.append(ctx.process_iq(iq[1100000:], flush=True))
    assert m_busy > 4 * max(m_quiet, 1)                      # the capacity (1.25 x extrapolation) was exceeded
    assert np.concatenate(got).tobytes() == pk[k].tobytes()
    st = ctx.address_gate_stats()
    assert (st["taught"], st["passed"], st["dropped"]) == gc.counts(pk, k)       # the repeated scan counted once
    ctx.close()
    monkeypatch.setenv("AIRMODES_NO_SPEC", "1")
    ctx = _capi.Context(rate, 7.0, True, lib=emu_lib)
    ctx.set_address_gate(1, ttl_s)
    got = [ctx.process_iq(iq[:700001]), ctx.process_iq(iq[700001:], flush=True)]
    ctx.close()
    assert np.concatenate(got).tobytes() == pk[k].tobytes()


# ---- 6. pipes and bank ------------------------------------------------------------------------------------------------------------
def test_pipe(emu_lib, small):
    iq = small[0][:600_000]
    pk = oracle.demod(iq, 4e6, 7.0)
    want = pk[gc.gate(pk, 2, gc.ttl_samples(0.05, 4e6))]
    assert 0 < len(want) < len(pk)
    pipe = _capi.Pipe(4e6, 7.0, True, depth=2, lib=emu_lib)
    assert pipe.get_address_gate() == (0, 60.0)
    pipe.set_address_gate(2, 0.05)
    assert pipe.get_address_gate() == (2, 0.05)
    pipe.submit(iq)
    with pytest.raises(_capi.AirModesError):
        pipe.set_address_gate(1, 0.05)                                  # a batch is in flight
    pipe.submit(iq)
    # every batch is a whole stream with a map of its own: the same capture twice gives the same packets twice
    assert pipe.collect().tobytes() == want.tobytes() and pipe.collect().tobytes() == want.tobytes()
    pipe.submit(iq)
    assert pipe.collect().tobytes() == want.tobytes()
    for bad in ((3, 60.0), (1, 0.0), (1, float("nan"))):
        with pytest.raises(_capi.AirModesError):
            pipe.set_address_gate(*bad)
    assert pipe.get_address_gate() == (2, 0.05)
    pipe.close()


def test_streams_of_one_scan_do_not_share_aircraft(emu_lib):
    """am_process_multi, three captures of ONE fleet: B holds only address/parity frames -- alone it keeps none, and it must
    not see the aircraft A and C teach in the same scan.  rx_path_bank: the same through the queues."""
    import air_modes
    oracle.build()
    rate = 4e6
    iq_a, _, fleet = gc.fleet_capture(rate, 700_000, 3000.0, 31, 10)
    only_ap = tuple((d, 1.0) for d in (0, 4, 5, 20, 21))
    iq_b = gc.fleet_capture(rate, 500_001, 3000.0, 32, 10, fleet=fleet, mix=only_ap)[0]
    iq_c = gc.fleet_capture(rate, 600_000, 3000.0, 33, 10, fleet=fleet)[0]
    caps = [iq_a, iq_b, iq_c]
    pks = [oracle.demod(x, rate, 7.0) for x in caps]
    assert int(np.isin(pks[1]["df"], AP).sum()) > 100
    ctx = _capi.Context(rate, 7.0, True, lib=emu_lib)
    buf, lens = ctx.multi_pack(caps)
    for mode, ttl_s in ((0, 60.0), (1, 60.0), (2, 60.0), (1, 0.01)):
        ttl = gc.ttl_samples(ttl_s, rate)
        ctx.set_address_gate(mode, ttl_s)
        keeps = [gc.gate(p, mode, ttl) for p in pks]
        if mode:
            assert not np.isin(pks[1][keeps[1]]["df"], AP).any() and keeps[0].sum() > 100
        before = ctx.address_gate_stats()
        got = ctx.process_multi(buf, lens)
        for g, p, k in zip(got, pks, keeps):
            assert g.tobytes() == p[k].tobytes(), (mode, ttl_s)
        ctx.submit_multi(buf, lens)
        got = ctx.collect_multi()
        for g, p, k in zip(got, pks, keeps):
            assert g.tobytes() == p[k].tobytes(), (mode, ttl_s)
        after = ctx.address_gate_stats()
        if mode:
            tot = np.sum([gc.counts(p, k) for p, k in zip(pks, keeps)], axis=0)
            assert [after[x] - before[x] for x in ("taught", "passed", "dropped")] == [2 * int(v) for v in tot]
    ctx.close()
    qs = [air_modes.msg_queue() for _ in caps]
    air_modes.rx_path_bank(rate, 7.0, qs, use_pmf=True, lib=emu_lib, address_gate=2, address_ttl=0.01).work(caps)
    for q, p in zip(qs, pks):
        assert drain(q) == oracle.format_messages(p[gc.gate(p, 2, gc.ttl_samples(0.01, rate))])


# ---- 7. setters ---------------------------------------------------------------------------------------------------------------------
def test_setters(emu_lib, small):
    L = emu_lib.L
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    assert ctx.get_address_gate() == (0, 60.0)
    for bad in ((-1, 60.0), (3, 60.0), (1, 0.0), (1, -1.0), (1, float("inf")), (1, float("nan"))):
        with pytest.raises(_capi.AirModesError) as e:
            ctx.set_address_gate(*bad)
        assert e.value.code == _capi.AM_EINVAL and ctx.get_address_gate() == (0, 60.0)
    for v in ((2, 1.5), (1, 60.0), (0, 3.0), (2, 0.25)):
        ctx.set_address_gate(*v)
        assert ctx.get_address_gate() == v
    ctx.reset()
    assert ctx.get_address_gate() == (2, 0.25)
    ctx.set_rate(8e6)
    assert ctx.get_address_gate() == (2, 0.25)
    ctx.set_rate(4e6)
    assert L.am_set_address_gate(None, 1, 60.0) == _capi.AM_EINVAL
    assert L.am_get_address_gate(None, None, None) == _capi.AM_EINVAL
    assert L.am_get_address_gate_stats(None, None, None, None, None) == _capi.AM_EINVAL
    assert L.am_pipe_set_address_gate(None, 1, 60.0) == _capi.AM_EINVAL
    assert L.am_pipe_get_address_gate(None, None, None) == _capi.AM_EINVAL
    assert L.am_get_address_gate(ctx._h, None, None) == _capi.AM_OK
    # the time shards refuse the gate and are what they were without it
    iq = small[0][:400_000]
    left, right = ctx.shard_halo()
    assert left >= 0 and right >= 0
    with pytest.raises(_capi.AirModesError) as e:
        ctx.shard_scan(iq, 0, len(iq), len(iq))
    assert e.value.code == _capi.AM_ENOTSUP
    with pytest.raises(_capi.AirModesError) as e:
        ctx.shard_resolve(0)
    assert e.value.code == _capi.AM_ENOTSUP
    ctx.set_address_gate(0, 60.0)
    ctx.shard_scan(iq, 0, len(iq), len(iq))
    assert ctx.shard_resolve(0).tobytes() == oracle.demod(iq, 4e6, 7.0).tobytes()
    ctx.close()
    import air_modes
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, 2, True), 2, 7.0, 4e6)
    want = oracle.slice_bursts(bursts, tags)
    sl = air_modes.slicer(air_modes.msg_queue(), lib=emu_lib, address_gate=2, address_ttl=0.01)
    assert sl.work(bursts, tags).tobytes() == want[gc.gate(want, 2, 40_000)].tobytes()


def test_modes_rx_options_parse():
    from air_modes import modes_rx
    ap = modes_rx.build_parser()
    a = ap.parse_args(["-s", "x.cf32"])
    assert a.address_gate == 0 and a.address_ttl == 60.0
    a = ap.parse_args(["-s", "x.cf32", "--address-gate", "2", "--address-ttl", "12.5"])
    assert a.address_gate == 2 and a.address_ttl == 12.5
    with pytest.raises(SystemExit):
        ap.parse_args(["-s", "x.cf32", "--address-gate", "3"])
