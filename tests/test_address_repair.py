"""Opt-in repair of one wrong bit in an address/parity reply (am_set_address_repair), without a GPU: the definition
(tests/aprepair_common.py) on the captures of the address gate's tests, hand-made bursts on every edge of the candidate range and
of the window, the library -- the product sources under the CPU emulation -- against the definition, byte for byte and text for
text, and the reference's slicer on the repaired bursts with the chips of the repaired bit exchanged."""
import numpy as np
import pytest

import aprepair_common as ar
import fix_common as fx
import gate_common as gc
import oracle
import synth
from air_modes import _capi

AP = gc.AP
TTL60 = gc.ttl_samples(60.0, 4e6)


@pytest.fixture(scope="module")
def low():
    """4 Msps, 0.5 s, 4 000 bursts/s of a fleet of 40 at SNR 4-14 dB: what the emulated library is run on.
    (iq, truth, the oracle's packets)"""
    oracle.build()
    iq, truth, _ = gc.fleet_capture(4e6, 2_000_000, 4000.0, 22, 40, (4.0, 14.0))
    return iq, truth, oracle.demod(iq, 4e6, 7.0)


def expected(pk, mode, ttl_s, rate=4e6, on=1):
    return ar.repair(pk, mode, gc.ttl_samples(ttl_s, rate), on)


def drain(q):
    got = []
    while not q.empty_p():
        got.append(q.delete_head().to_string())
    return got


def repair_ctx(lib, rate=4e6, mode=1, ttl_s=60.0, on=1):
    ctx = _capi.Context(rate, 7.0, True, lib=lib)
    ctx.set_address_gate(mode, ttl_s)
    ctx.set_address_repair(on)
    return ctx


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------
def check_definition(pk, truth, ttl, n_repaired):
    out, keep, fixed, ambiguous = ar.repair(pk, 1, ttl)
    rep = out[out["reserved"][:, 1] != 0]
    true = gc.transmitted(rep, truth)
    print("packets %d, kept %d, repaired %d (transmitted %d), ambiguous %d" % (len(pk), keep.sum(), len(rep), true.sum(), ambiguous))
    assert (len(rep), int((~true).sum()), ambiguous) == (n_repaired, 0, 0)
    assert (rep["crc"] != pk[fixed >= 0]["crc"]).all() and np.isin(rep["df"], AP).all()
    assert (fixed[fixed >= 0] >= 5).all() and (fixed[fixed >= 0] < 8 * pk[fixed >= 0]["nbytes"]).all()
    # every field but data, crc and reserved[1] is as sliced; data differs in exactly the one bit
    was = pk[fixed >= 0]
    for name in ("nbytes", "df", "numlowconf", "ref", "sample", "secs", "frac"):
        assert (rep[name] == was[name]).all()
    flipped = np.unpackbits(rep["data"] ^ was["data"], axis=1)
    assert (flipped.sum(axis=1) == 1).all() and (flipped.argmax(axis=1) == fixed[fixed >= 0]).all()
    # the independent O(n^2) search
    bf = ar.brute_force(pk, ttl)
    k0 = gc.gate(pk, 1, ttl)
    assert sorted(bf) == np.flatnonzero(np.isin(pk["df"], AP) & ~k0).tolist()
    assert {i: js[0] for i, js in bf.items() if len(js) == 1} == {int(i): int(fixed[i]) for i in np.flatnonzero(fixed >= 0)}
    assert sum(1 for js in bf.values() if len(js) > 1) == ambiguous
    # off is a subsequence of on, up to the repaired ones; mode 2 repairs the same packets; off is the gate
    assert ar.off_is_subsequence_of_on(pk, k0, keep, fixed)
    out0, keep0, fixed0, amb0 = ar.repair(pk, 1, ttl, on=0)
    assert out0.tobytes() == pk[k0].tobytes() and (fixed0 < 0).all() and amb0 == 0
    out2, keep2, fixed2, _ = ar.repair(pk, 2, ttl)
    assert (fixed2 == fixed).all() and not (keep2 & ~keep).any()
    assert ar.repair(pk, 0, ttl)[0].tobytes() == pk.tobytes()
    return out, keep, fixed


@pytest.mark.parametrize("which,args,thr,n_repaired",
                         [("cap_a", (4e6, 8_000_000, 3000.0, 21, 40), 7.0, 21),
                          ("cap_b", (4e6, 8_000_000, 4000.0, 22, 40, (4.0, 14.0)), 7.0, 101),
                          ("noise", (4e6, 8_000_000, 0.0, 3, 40), 5.0, 0),
                          ("low", (4e6, 2_000_000, 4000.0, 22, 40, (4.0, 14.0)), 7.0, 11)])
def test_definition_on_the_gates_captures(which, args, thr, n_repaired):
    oracle.build()
    iq, truth, _ = gc.fleet_capture(*args)
    pk = oracle.demod(iq, 4e6, thr)
    check_definition(pk, truth, TTL60, n_repaired)


# ---- 2. hand-made bursts through am_slicer_work ---------------------------------------------------------------------------------
def hand_made(samples_and_frames):
    """Clean bursts (chips 0 / 1) of the given frames at the given item counts."""
    b = np.zeros((len(samples_and_frames), 240), np.float32)
    t = np.zeros(len(samples_and_frames), oracle.TAG_DTYPE)
    for i, (s, frame) in enumerate(samples_and_frames):
        chips = synth.frame_chips(frame)
        b[i, :chips.size] = chips
        t[i]["sample"] = s
    return b, t


def flip(frame, *bits):
    f = bytearray(frame)
    for j in bits:
        f[j >> 3] ^= 0x80 >> (j & 7)
    return bytes(f)


def run_hand_made(emu_lib, seq, ttl_s=0.001, rate=4e6):
    """-> (packets of am_slicer_work with the repair on, the repair's stats); checked against the definition, with the repair
    off against the gate alone, and across two calls at every cut."""
    seq = sorted(seq, key=lambda x: x[0])
    b, t = hand_made(seq)
    pk = oracle.slice_bursts(b, t)
    assert len(pk) == len(seq)
    T = gc.ttl_samples(ttl_s, rate)
    want, keep, fixed, ambiguous = ar.repair(pk, 1, T)
    ctx = repair_ctx(emu_lib, rate, 1, ttl_s)
    got = ctx.slicer_work(b, t)
    st = ctx.address_repair_stats()
    assert got.tobytes() == want.tobytes()
    assert emu_lib.format_messages(got, True) == oracle.format_messages(want)
    assert st == dict(repaired=int((fixed >= 0).sum()), ambiguous=ambiguous)
    gs = ctx.address_gate_stats()
    assert (gs["taught"], gs["passed"], gs["dropped"]) == ar.counts(pk, keep, fixed)[:3]
    for cut in range(1, len(seq)):
        ctx.reset()
        two = np.concatenate([ctx.slicer_work(b[:cut], t[:cut]), ctx.slicer_work(b[cut:], t[cut:])])
        assert two.tobytes() == want.tobytes(), cut
    ctx.set_address_repair(0)
    ctx.reset()
    assert ctx.slicer_work(b, t).tobytes() == pk[gc.gate(pk, 1, T)].tobytes()
    # (the stats are the context's: the first run and one more for every cut; the run with the repair off added nothing)
    assert ctx.address_repair_stats() == dict(repaired=st["repaired"] * len(seq), ambiguous=st["ambiguous"] * len(seq))
    ctx.close()
    return got, st


@pytest.mark.parametrize("df", [4, 20])
def test_every_edge_of_the_candidate_range(emu_lib, df):
    """A wrong bit at j = 5, nbits - 25 (the last message bit), nbits - 24 (the first parity bit) and nbits - 1, for a short and
    for a long reply: repaired into the transmitted frame, crc = the address.  A wrong bit among the five DF bits (DF4 <-> DF5,
    DF20 <-> DF21: still an address/parity reply of the same length) is no candidate."""
    oracle.build()
    rng = np.random.default_rng(7)
    a1, a2 = 0x4840D6, 0xABCDEF
    nbits = 112 if df == 20 else 56
    frames = [gc.fleet_frame(rng, df, a1) for _ in range(5)]
    js = [5, nbits - 25, nbits - 24, nbits - 1]
    seq = [(1000, gc.fleet_frame(rng, 17, a1)), (1100, gc.fleet_frame(rng, 11, a2))]
    seq += [(2000 + 100 * k, flip(frames[k], j)) for k, j in enumerate(js)]
    seq += [(2500, flip(frames[4], 4))]
    got, st = run_hand_made(emu_lib, seq)
    assert st == dict(repaired=4, ambiguous=0) and len(got) == 6
    for k, j in enumerate(js):
        p = got[2 + k]
        assert bytes(p["data"][:nbits // 8]) == frames[k] and int(p["crc"]) == a1 and p["reserved"].tolist() == [0, 1, 0]
        assert int(p["df"]) == df and int(p["sample"]) == 2000 + 100 * k


def test_window_edges_and_order(emu_lib):
    """A teach exactly ttl before the damaged reply and one ttl + 1 before it; a teach behind the reply is not used."""
    oracle.build()
    rng = np.random.default_rng(8)
    a1, a2, a3 = 0x4840D6, 0xABCDEF, 0x000001
    T = gc.ttl_samples(0.001, 4e6)
    assert T == 4000
    f1, f2, f3 = gc.fleet_frame(rng, 20, a1), gc.fleet_frame(rng, 4, a2), gc.fleet_frame(rng, 21, a3)
    seq = [(1000, gc.fleet_frame(rng, 17, a1)), (1000 + T, flip(f1, 40)),            # exactly ttl: repaired
           (1500, gc.fleet_frame(rng, 11, a2)), (1500 + T + 1, flip(f2, 9)),         # one more: dropped
           (9000, flip(f3, 77)), (9100, gc.fleet_frame(rng, 17, a3)),                # taught behind it: dropped
           (9200, flip(f3, 77))]                                                     # the same reply behind the teach: repaired
    got, st = run_hand_made(emu_lib, seq)
    assert st == dict(repaired=2, ambiguous=0)
    assert [(int(p["sample"]), int(p["df"]), int(p["reserved"][1])) for p in got] == \
        [(1000, 17, 0), (1500, 11, 0), (1000 + T, 20, 1), (9100, 17, 0), (9200, 21, 1)]
    assert bytes(got[2]["data"]) == f1 and bytes(got[4]["data"]) == f3


def test_ambiguous_pair_and_two_wrong_bits(emu_lib):
    """Fleet addresses A and B = A ^ syn(j1) ^ syn(j2): a reply of A with bit j1 wrong is as well a reply of B with bit j2 wrong --
    dropped, and counted.  A reply with two wrong bits is not repaired."""
    oracle.build()
    rng = np.random.default_rng(9)
    A = 0x4840D6
    j1, j2 = 17, 60
    B = A ^ int(fx.SYN[112][j1]) ^ int(fx.SYN[112][j2])
    assert 0 < B < (1 << 24) and B != A
    fa = gc.fleet_frame(rng, 20, A)
    seq = [(1000, gc.fleet_frame(rng, 17, A)), (1100, gc.fleet_frame(rng, 17, B)),
           (2000, flip(fa, j1)),                                                         # A's with j1 wrong, or B's with j2 wrong
           (2100, flip(fa, 30, 31)),                                                     # two wrong bits
           (2200, flip(fa, j2 + 1))]                                                     # one wrong bit elsewhere: repaired
    got, st = run_hand_made(emu_lib, seq)
    assert st == dict(repaired=1, ambiguous=1)
    assert got["sample"].tolist() == [1000, 1100, 2200] and bytes(got[2]["data"]) == fa and int(got[2]["crc"]) == A
    # with B unknown the same reply is A's
    got, st = run_hand_made(emu_lib, [seq[0], seq[2]])
    assert st == dict(repaired=1, ambiguous=0) and bytes(got[1]["data"]) == fa


# ---- 3. the emulated library against the definition -----------------------------------------------------------------------------
def test_whole_path_as_defined(emu_lib, low):
    """One call, uneven cuts with a flush, a small capacity followed by am_fetch_packets; the counters."""
    iq, truth, pk = low
    n = len(iq)
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    ctx.set_address_repair(1)
    gstat = dict(taught=0, passed=0, dropped=0, not_learned=0)
    rstat = dict(repaired=0, ambiguous=0)
    assert ctx.process_iq(iq, flush=True).tobytes() == pk.tobytes()      # inert while the gate is off
    for mode, ttl_s in ((1, 60.0), (2, 60.0), (1, 0.05)):
        want, keep, fixed, amb = expected(pk, mode, ttl_s)
        assert int((fixed >= 0).sum()) == {60.0: 11, 0.05: 5}[ttl_s]
        ctx.set_address_gate(mode, ttl_s)
        got = ctx.process_iq(iq, flush=True)
        assert got.tobytes() == want.tobytes(), (mode, ttl_s)
        assert emu_lib.format_messages(got, True) == oracle.format_messages(want)
        for cuts in ([0, 70_001, 70_002, 811_117, 1_500_000, n - 333, n], [0, 1_000_000, 1_003_000, 1_009_000, 1_011_111, n]):
            parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.concatenate(parts).tobytes() == want.tobytes(), (mode, ttl_s, cuts)
        assert ctx.process_iq(iq, flush=True, capacity=8).tobytes() == want.tobytes()      # AM_ECAPACITY + am_fetch_packets
        c = ar.counts(pk, keep, fixed)
        for key, v in zip(("taught", "passed", "dropped"), c[:3]):
            gstat[key] += 4 * v
        rstat["repaired"] += 4 * c[3]
        rstat["ambiguous"] += 4 * amb
        assert ctx.address_gate_stats() == gstat and ctx.address_repair_stats() == rstat
    ctx.close()


def test_with_fix_errors_on(emu_lib, low):
    """fix_errors = 2: a repaired DF11 / DF17 reply teaches nothing, the address/parity repair sees the same map."""
    iq, truth, pk0 = low
    pk = fx.expected_from_capture(iq, 4e6, 2)
    assert int(np.count_nonzero(pk["reserved"][:, 1])) > 20
    want, keep, fixed, amb = expected(pk, 1, 60.0)
    assert int((fixed >= 0).sum()) == 11
    ctx = repair_ctx(emu_lib)
    ctx.set_fix_errors(2)
    assert ctx.process_iq(iq, flush=True).tobytes() == want.tobytes()
    parts = [ctx.process_iq(iq[:900_001]), ctx.process_iq(iq[900_001:], flush=True)]
    assert np.concatenate(parts).tobytes() == want.tobytes()
    ctx.close()


def test_pipe(emu_lib, low):
    """am_pipe_submit / am_pipe_collect (am_submit_iq / am_collect on the pipe's contexts): every batch is a whole stream."""
    iq, truth, pk = low
    want = expected(pk, 1, 60.0)[0]
    pipe = _capi.Pipe(4e6, 7.0, True, depth=2, lib=emu_lib)
    assert pipe.get_address_repair() == 0
    pipe.set_address_gate(1, 60.0)
    pipe.set_address_repair(1)
    assert pipe.get_address_repair() == 1
    pipe.submit(iq)
    with pytest.raises(_capi.AirModesError) as e:
        pipe.set_address_repair(0)                                       # a batch is in flight
    assert e.value.code == _capi.AM_EINVAL
    pipe.submit(iq)
    assert pipe.collect().tobytes() == want.tobytes() and pipe.collect().tobytes() == want.tobytes()
    with pytest.raises(_capi.AirModesError):
        pipe.set_address_repair(2)
    assert pipe.get_address_repair() == 1
    pipe.set_address_repair(0)
    pipe.submit(iq)
    assert pipe.collect().tobytes() == pk[gc.gate(pk, 1, TTL60)].tobytes()
    pipe.close()


def test_streams_of_one_scan_search_their_own_map(emu_lib):
    """am_process_multi / am_submit_multi / rx_path_bank, three captures of ONE fleet: B holds only address/parity frames -- it
    repairs nothing, whatever A and C teach in the same scan."""
    import air_modes
    oracle.build()
    rate = 4e6
    snr = (4.0, 14.0)
    iq_a, _, fleet = gc.fleet_capture(rate, 900_000, 4000.0, 31, 10, snr)
    only_ap = tuple((d, 1.0) for d in (0, 4, 5, 20, 21))
    iq_b = gc.fleet_capture(rate, 500_001, 4000.0, 32, 10, snr, fleet=fleet, mix=only_ap)[0]
    iq_c = gc.fleet_capture(rate, 800_000, 4000.0, 33, 10, snr, fleet=fleet)[0]
    caps = [iq_a, iq_b, iq_c]
    pks = [oracle.demod(x, rate, 7.0) for x in caps]
    assert int(np.isin(pks[1]["df"], AP).sum()) > 50
    ctx = _capi.Context(rate, 7.0, True, lib=emu_lib)
    ctx.set_address_repair(1)
    buf, lens = ctx.multi_pack(caps)
    for mode, ttl_s in ((1, 60.0), (2, 0.05)):
        ttl = gc.ttl_samples(ttl_s, rate)
        ctx.set_address_gate(mode, ttl_s)
        exp = [ar.repair(p, mode, ttl) for p in pks]
        n_rep = [int((e[2] >= 0).sum()) for e in exp]
        print("repaired per stream:", n_rep)
        assert n_rep[0] > 0 and n_rep[2] > 0 and n_rep[1] == 0
        assert not np.isin(exp[1][0]["df"], AP).any()
        before = ctx.address_repair_stats()
        got = ctx.process_multi(buf, lens)
        for g, e in zip(got, exp):
            assert g.tobytes() == e[0].tobytes(), (mode, ttl_s)
        ctx.submit_multi(buf, lens)
        for g, e in zip(ctx.collect_multi(), exp):
            assert g.tobytes() == e[0].tobytes(), (mode, ttl_s)
        after = ctx.address_repair_stats()
        assert after["repaired"] - before["repaired"] == 2 * sum(n_rep) and after["ambiguous"] == before["ambiguous"]
    ctx.close()
    qs = [air_modes.msg_queue() for _ in caps]
    bank = air_modes.rx_path_bank(rate, 7.0, qs, use_pmf=True, lib=emu_lib, address_gate=1, address_ttl=60.0, address_repair=1)
    bank.work(caps)
    for q, p in zip(qs, pks):
        assert drain(q) == oracle.format_messages(ar.repair(p, 1, TTL60)[0])
    qs = [air_modes.msg_queue() for _ in caps]
    bank = air_modes.rx_path_bank(rate, 7.0, qs, use_pmf=True, lib=emu_lib, address_gate=1, address_ttl=60.0, address_repair=1)
    bank.set_address_repair(0)
    bank.work(caps)
    for q, p in zip(qs, pks):
        assert drain(q) == oracle.format_messages(p[gc.gate(p, 1, TTL60)])


def test_repeated_scan_counts_once(emu_lib, monkeypatch):
    """AIRMODES_SPEC_FLOOR=0, a quiet stretch and then a dense one: the dense scan overflows the capacity it was launched for
    and is redone (AM_RETRY_EXACT).  Packets == definition, and the repair's stats are added once."""
    monkeypatch.setenv("AIRMODES_SPEC_FLOOR", "0")
    oracle.build()
    rate = 8e6
    fleet = gc.fleet_capture(rate, 1000, 0.0, 610, 12)[2]
    quiet = gc.fleet_capture(rate, 600_000, 40.0, 611, 12, (4.0, 14.0), fleet=fleet)[0]
    busy = gc.fleet_capture(rate, 900_000, 20000.0, 612, 12, (4.0, 14.0), fleet=fleet)[0]
    iq = np.concatenate([quiet, busy])
    pk = oracle.demod(iq, rate, 7.0, True)
    ttl_s = 0.01
    want, keep, fixed, amb = expected(pk, 1, ttl_s, rate)
    print("repaired %d, ambiguous %d of %d packets" % ((fixed >= 0).sum(), amb, len(pk)))
    assert (fixed >= 0).sum() > 0
    ctx = repair_ctx(emu_lib, rate, 1, ttl_s)
    got = [ctx.process_iq(iq[:300000]), ctx.process_iq(iq[300000:600000])]
    m_quiet = ctx.last_num_candidates()
    got.append(ctx.process_iq(iq[600000:1100000]))
    m_busy = ctx.last_num_candidates()
    got.append(ctx.process_iq(iq[1100000:], flush=True))
    assert m_busy > 4 * max(m_quiet, 1)                      # the capacity (1.25 x extrapolation) was exceeded
    assert np.concatenate(got).tobytes() == want.tobytes()
    assert ctx.address_repair_stats() == dict(repaired=int((fixed >= 0).sum()), ambiguous=amb)
    gs = ctx.address_gate_stats()
    assert (gs["taught"], gs["passed"], gs["dropped"]) == ar.counts(pk, keep, fixed)[:3]
    ctx.close()


def test_rx_path_texts_and_counters(emu_lib, low):
    import air_modes
    iq, truth, pk = low
    for mode, ttl_s, on in ((1, 60.0, 1), (2, 0.05, 1), (1, 60.0, 0), (0, 60.0, 1)):
        want, keep, fixed, amb = expected(pk, mode, ttl_s, on=on)
        q = air_modes.msg_queue()
        rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, lib=emu_lib, address_gate=mode, address_ttl=ttl_s, address_repair=on)
        assert rx.get_address_repair() == on
        rx.work(iq[:900_001])
        rx.work(iq[900_001:], flush=True)
        assert drain(q) == oracle.format_messages(want)
        assert rx.packets == len(want) and rx.repaired == int((fixed >= 0).sum()) and rx.gated == int((~keep).sum())
        if mode and on:
            assert rx.repaired > 0
    q = air_modes.msg_queue()
    rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, lib=emu_lib, address_gate=1)
    rx.set_address_repair(1)
    rx.work(iq, flush=True)
    assert drain(q) == oracle.format_messages(expected(pk, 1, 60.0)[0])


def test_slicer_block(emu_lib, low):
    import air_modes
    iq, truth, pk = low
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, 2, True), 2, 7.0, 4e6)
    want = oracle.slice_bursts(bursts, tags)
    assert want.tobytes() == pk.tobytes()
    sl = air_modes.slicer(air_modes.msg_queue(), lib=emu_lib, address_gate=1, address_ttl=60.0, address_repair=1)
    assert sl.work(bursts, tags).tobytes() == expected(pk, 1, 60.0)[0].tobytes()


def test_off_means_off(emu_lib, low):
    """Setting 0, or the gate off, returns exactly the packets of the library as it is without the setting."""
    iq, truth, pk = low
    plain = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    plain.set_address_gate(1, 60.0)
    gated = plain.process_iq(iq, flush=True)
    plain.close()
    assert gated.tobytes() == pk[gc.gate(pk, 1, TTL60)].tobytes()
    ctx = repair_ctx(emu_lib)
    on = ctx.process_iq(iq, flush=True)
    assert len(on) == len(gated) + 11
    ctx.set_address_repair(0)
    assert ctx.process_iq(iq, flush=True).tobytes() == gated.tobytes()
    ctx.set_address_repair(1)
    ctx.set_address_gate(0, 60.0)
    assert ctx.process_iq(iq, flush=True).tobytes() == pk.tobytes()
    assert ctx.address_repair_stats() == dict(repaired=11, ambiguous=0)
    ctx.close()


# ---- 4. setters -----------------------------------------------------------------------------------------------------------------
def test_setters(emu_lib):
    L = emu_lib.L
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    assert ctx.get_address_repair() == 0 and ctx.address_repair_stats() == dict(repaired=0, ambiguous=0)
    for bad in (-1, 2, 3):
        with pytest.raises(_capi.AirModesError) as e:
            ctx.set_address_repair(bad)
        assert e.value.code == _capi.AM_EINVAL and ctx.get_address_repair() == 0
    ctx.set_address_repair(1)
    assert ctx.get_address_repair() == 1
    ctx.reset()
    assert ctx.get_address_repair() == 1
    ctx.set_rate(8e6)
    assert ctx.get_address_repair() == 1
    ctx.set_address_gate(2, 1.0)
    ctx.set_address_gate(0, 1.0)
    assert ctx.get_address_repair() == 1
    ctx.set_address_repair(0)
    assert ctx.get_address_repair() == 0
    assert L.am_set_address_repair(None, 1) == _capi.AM_EINVAL
    assert L.am_get_address_repair(None) == _capi.AM_EINVAL
    assert L.am_get_address_repair_stats(None, None, None) == _capi.AM_EINVAL
    assert L.am_get_address_repair_stats(ctx._h, None, None) == _capi.AM_OK
    assert L.am_pipe_set_address_repair(None, 1) == _capi.AM_EINVAL
    assert L.am_pipe_get_address_repair(None) == _capi.AM_EINVAL
    assert L.am_abi_version() == 5
    ctx.close()


def test_modes_rx_option_parses():
    from air_modes import modes_rx
    ap = modes_rx.build_parser()
    assert ap.parse_args(["-s", "x.cf32"]).address_repair == 0
    a = ap.parse_args(["-s", "x.cf32", "--address-gate", "1", "--address-repair", "1"])
    assert a.address_gate == 1 and a.address_repair == 1
    with pytest.raises(SystemExit):
        ap.parse_args(["-s", "x.cf32", "--address-repair", "2"])


# ---- 5. pinned to the reference -------------------------------------------------------------------------------------------------
def test_the_reference_slicer_on_chip_exchanged_bursts():
    """Exchanging the two chips of bit j flips the decision and keeps the confidence (slicer_impl.cc:74-98), so the reference's
    own slicer, given the burst with that chip pair exchanged, emits the repaired packet with crc = A_j -- for every repaired
    burst of the 8 000 000-sample low-SNR capture."""
    oracle.build()
    iq, truth, _ = gc.fleet_capture(4e6, 8_000_000, 4000.0, 22, 40, (4.0, 14.0))
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, 2, True), 2, 7.0, 4e6)
    pk, idx, _ = fx.slice_fix(bursts, tags, 0)
    assert pk.tobytes() == oracle.slice_bursts(bursts, tags).tobytes()
    out, keep, fixed, amb = ar.repair(pk, 1, TTL60)
    assert int((fixed >= 0).sum()) == 101
    full = pk.copy()
    full[keep] = out
    sw, ti, want, left_out = fx.exchange_chips(bursts, full, idx)
    assert left_out == 0 and len(want) == 101 and want.tobytes() == out[out["reserved"][:, 1] != 0].tobytes()
    plain = want.copy()
    plain["reserved"] = 0
    got = oracle.slice_bursts(sw, tags[ti])
    assert got.tobytes() == plain.tobytes()
    assert gc.transmitted(got, truth).all()
    if oracle.have_ref():
        texts, acc = oracle.ref_slice_bursts(sw, tags[ti])
        assert acc.all() and texts == oracle.format_messages(plain)
