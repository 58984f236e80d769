"""Opt-in repair of DF11 / DF17 replies with one or two wrong bits (am_set_fix_errors), without a GPU: the uniqueness the
definition rests on, the definition (tests/fix_common.py) against the reference's own slicer, and the library -- the product
sources under the CPU emulation -- against the definition."""
import itertools

import numpy as np
import pytest

import fix_common as fx
import oracle
import parity_common as pc
from air_modes import _capi


@pytest.fixture(scope="module")
def damaged():
    oracle.build()
    return fx.damaged_bursts(6000, 11)


@pytest.fixture(scope="module")
def edge():
    oracle.build()
    return pc.edge_bursts(4000, 3)


@pytest.fixture(scope="module")
def capture():
    oracle.build()
    return fx.low_snr_capture(4e6, 2_000_000, 77)


def test_syndromes_of_one_and_two_wrong_bits_are_unique():
    """For 56 and for 112 bits, over ALL positions: the syndromes of the one-bit and the two-bit patterns are non-zero,
    distinct and disjoint from each other, and no three-bit pattern has one of them -- a repair is unique when it exists, and
    three wrong bits are never repaired into another frame."""
    for nbits in (56, 112):
        syn = fx.SYN[nbits]
        # the table is the syndrome of a unit frame, and syndromes add (the CRC is linear): one random frame through both
        rng = np.random.default_rng(nbits)
        bits = rng.integers(0, 2, nbits)
        assert fx.crc_serial(bits) == int(np.bitwise_xor.reduce(syn[bits == 1]))
        one = set(int(s) for s in syn)
        two = [int(syn[a] ^ syn[b]) for a, b in itertools.combinations(range(nbits), 2)]
        assert len(one) == nbits and 0 not in one
        assert len(set(two)) == len(two) == nbits * (nbits - 1) // 2 and 0 not in two
        assert not one & set(two)
        low = np.array(sorted(one | set(two)), np.int64)
        a, b, c = np.array(list(itertools.combinations(range(nbits), 3))).T
        three = syn[a] ^ syn[b] ^ syn[c]
        assert len(three) == nbits * (nbits - 1) * (nbits - 2) // 6
        assert not np.isin(three, low).any() and (three != 0).all()


def test_definition_without_repair_is_the_reference_slicer(damaged, edge):
    """fix_common proves itself: with max_bits = 0 its packets are the oracle's, byte for byte."""
    b, t = edge
    want = oracle.slice_bursts(b, t)
    assert len(want) == 1757
    assert fx.slice_fix(b, t, 0)[0].tobytes() == want.tobytes()
    b, t, _ = damaged
    want = oracle.slice_bursts(b, t)
    assert len(want) == 1342
    assert fx.slice_fix(b, t, 0)[0].tobytes() == want.tobytes()


def test_definition_against_the_reference_slicer_with_chips_exchanged(damaged):
    """The reference's own slicer, given the burst with the two chips of every repaired bit exchanged, emits exactly the
    repaired packet (slicer_impl.cc:74-98: the decision flips, the confidence stays).  Every repaired frame is the transmitted
    one, and no burst with three wrong bits is repaired."""
    b, t, meta = damaged
    pk1, _, _ = fx.slice_fix(b, t, 1)
    assert len(pk1) == 2497 and fx.repaired_counts(pk1) == (245, 910, 0)
    pk, idx, searched = fx.slice_fix(b, t, 2)
    n11, n17, n2 = fx.repaired_counts(pk)
    assert len(pk) == 3426 and (n11, n17, n2) == (245, 910, 929)
    assert n11 >= 200 and n17 >= 800 and n2 >= 800                      # (the floors: hundreds of each)
    # one-bit repairs do not depend on max_bits
    assert pk[pk["reserved"][:, 1] != 2].tobytes() == pk1.tobytes()
    for p, i in zip(pk, idx):
        df, nerr, style, frame = meta[i]
        if p["reserved"][1]:                                            # (so none of the three-error bursts is among them)
            assert bytes(p["data"][:len(frame)]) == frame and nerr == p["reserved"][1] and p["crc"] == 0
    assert sum(1 for m in meta if m[1] == 3) > 1000
    sw, ti, want, left_out = fx.exchange_chips(b, pk, idx)
    assert left_out <= 0.01 * (n11 + n17 + n2)
    got = oracle.slice_bursts(sw, t[ti])
    plain = want.copy()
    plain["reserved"] = 0
    assert len(got) == len(want) and got.tobytes() == plain.tobytes()
    if oracle.have_ref():
        texts, acc = oracle.ref_slice_bursts(sw, t[ti])
        assert acc.all() and texts == oracle.format_messages(plain)


def test_slicer_work_repairs_as_defined(emu_lib, damaged, edge):
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    for max_bits in (0, 1, 2):
        ctx.set_fix_errors(max_bits)
        for b, t in (damaged[:2], edge):
            got = ctx.slicer_work(b, t)
            want = fx.slice_fix(b, t, max_bits)[0]
            assert got.tobytes() == want.tobytes(), "max_bits %d: %d vs %d packets" % (max_bits, len(got), len(want))
            if max_bits == 0:
                assert got.tobytes() == oracle.slice_bursts(b, t).tobytes()          # the unchanged contract
            assert emu_lib.format_messages(got, True) == oracle.format_messages(want)
    ctx.close()


def test_whole_path_repairs_as_defined(emu_lib, capture):
    """4 Msps, SNR 4-14 dB: one call, uneven chunks with a flush, and rx_path (message texts, rx.repaired)."""
    import air_modes
    iq, truth = capture
    n = len(iq)
    frames = set(x["frame"] for x in truth)
    want = {mb: fx.expected_from_capture(iq, 4e6, mb) for mb in (0, 1, 2)}
    assert len(want[0]) == 482 and want[0].tobytes() == oracle.demod(iq, 4e6).tobytes()
    n11, n17, n2 = fx.repaired_counts(want[2])
    assert n11 + n17 >= 60 and n2 >= 25 and (n11 + n17, n2) == (64, 28)
    assert fx.repaired_counts(want[1]) == (n11, n17, 0) and len(want[1]) == 546 and len(want[2]) == 574
    for p in want[2][want[2]["reserved"][:, 1] > 0]:
        assert bytes(p["data"][:p["nbytes"]]).hex() in frames
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    for mb in (0, 1, 2):
        ctx.set_fix_errors(mb)
        assert ctx.process_iq(iq, flush=True).tobytes() == want[mb].tobytes()
        cuts = [0, 70_001, 70_002, 811_117, 1_500_000, n - 333, n]
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == want[mb].tobytes()
        q = air_modes.msg_queue()
        rx = air_modes.rx_path(4e6, 7.0, q, use_pmf=True, lib=emu_lib, fix_errors=mb)
        assert rx.get_fix_errors() == mb
        rx.work(iq[:900_001])
        rx.work(iq[900_001:], flush=True)
        got = []
        while not q.empty_p():
            got.append(q.delete_head().to_string())
        assert got == oracle.format_messages(want[mb])
        assert rx.packets == len(want[mb]) and rx.repaired == sum(fx.repaired_counts(want[mb]))
    ctx.close()


def test_pipes_and_bank_forward_the_setting(emu_lib, capture):
    import air_modes
    iq = capture[0][:600_000]
    want = fx.expected_from_capture(iq, 4e6, 2)
    assert sum(fx.repaired_counts(want)) > 10
    pipe = _capi.Pipe(4e6, 7.0, True, depth=2, lib=emu_lib)
    assert pipe.get_fix_errors() == 0
    pipe.set_fix_errors(2)
    assert pipe.get_fix_errors() == 2
    pipe.submit(iq)
    with pytest.raises(_capi.AirModesError):
        pipe.set_fix_errors(1)                                          # a batch is in flight
    pipe.submit(iq)
    assert pipe.collect().tobytes() == want.tobytes() and pipe.collect().tobytes() == want.tobytes()
    with pytest.raises(_capi.AirModesError):
        pipe.set_fix_errors(3)
    pipe.close()
    sp = _capi.StreamPipe(4e6, 7.0, True, depth=2, lib=emu_lib)
    assert sp.get_fix_errors() == 0
    sp.set_fix_errors(2)
    assert sp.get_fix_errors() == 2
    with pytest.raises(_capi.AirModesError):
        sp.set_fix_errors(-1)
    base = np.ascontiguousarray(iq.view(np.float32))
    cuts = [0, 200_001, 410_000, len(iq)]
    got = sp.run([(base.ctypes.data + 8 * a, b - a) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.concatenate(got).tobytes() == want.tobytes()
    sp.close()
    caps = [iq[:300_000], iq[300_000:], iq[100_000:450_001]]
    qs = [air_modes.msg_queue() for _ in caps]
    air_modes.rx_path_bank(4e6, 7.0, qs, use_pmf=True, lib=emu_lib, fix_errors=2).work(caps)
    for q, cap in zip(qs, caps):
        got = []
        while not q.empty_p():
            got.append(q.delete_head().to_string())
        assert got == oracle.format_messages(fx.expected_from_capture(cap, 4e6, 2)) and got


def test_setters(emu_lib, damaged):
    ctx = _capi.Context(4e6, 7.0, True, lib=emu_lib)
    assert ctx.get_fix_errors() == 0
    for bad in (-1, 3, 17):
        with pytest.raises(_capi.AirModesError) as e:
            ctx.set_fix_errors(bad)
        assert e.value.code == _capi.AM_EINVAL and ctx.get_fix_errors() == 0
    for v in (2, 1, 0, 2):
        ctx.set_fix_errors(v)
        assert ctx.get_fix_errors() == v
    ctx.reset()
    assert ctx.get_fix_errors() == 2
    ctx.set_rate(8e6)
    assert ctx.get_fix_errors() == 2
    b, t, _ = damaged
    assert ctx.slicer_work(b[:500], t[:500]).tobytes() == fx.slice_fix(b[:500], t[:500], 2)[0].tobytes()
    ctx.close()
    assert emu_lib.L.am_get_fix_errors(None) == _capi.AM_EINVAL and emu_lib.L.am_set_fix_errors(None, 1) == _capi.AM_EINVAL
    import air_modes
    sl = air_modes.slicer(air_modes.msg_queue(), lib=emu_lib, fix_errors=1)
    assert sl.work(b[:500], t[:500]).tobytes() == fx.slice_fix(b[:500], t[:500], 1)[0].tobytes()


def test_modes_rx_option_parses():
    from air_modes import modes_rx
    ap = modes_rx.build_parser()
    assert ap.parse_args(["-s", "x.cf32"]).fix_errors == 0
    assert ap.parse_args(["-s", "x.cf32", "--fix-errors", "2"]).fix_errors == 2
    with pytest.raises(SystemExit):
        ap.parse_args(["-s", "x.cf32", "--fix-errors", "3"])
