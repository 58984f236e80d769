"""Opt-in 112-bit slicing and parity check of DF18 / DF19 squitters (am_set_long_formats), without a GPU: the definition
(tests/longfmt_common.py) with the option off against the oracle, with it on against the reference's own slicer, and the
library -- the product sources under the CPU emulation -- against the definition.

The two definition tests below run tests/longfmt_common.py, the oracle and the reference's slicer only, no code of the library:
they pin the definition and pass wherever that file exists.  Every other test here calls am_set_long_formats or the parser's
long_formats argument, and fails where those do not exist."""
import numpy as np
import pytest

import fix_common as fx
import gate_common as gc
import longfmt_common as lf
import oracle
import parity_common as pc
import synth
from air_modes import _capi

RATE = 4e6
CAPTURE = (RATE, 800_000, 6000.0, 33)            # 0.2 s at 4 Msps, SNR 6-14 dB
TTL_S = 60.0


@pytest.fixture(scope="module")
def bursts():
    oracle.build()
    return lf.long_bursts(6000, 21)


@pytest.fixture(scope="module")
def capture():
    """(iq, truth, what the oracle's scan hands the slicer)"""
    oracle.build()
    iq, truth = lf.capture(*CAPTURE)
    return iq, truth, lf.scan(iq, RATE)


def test_definition_with_the_option_off_is_the_reference_slicer(bursts):
    """The unchanged contract: mask 0 equals oracle.slice_bursts byte for byte, and equals fix_common with the repair on."""
    b, t, meta = bursts
    dfs = np.array([m[0] for m in meta])
    assert all((dfs == df).sum() >= 200 for df in lf.BURST_DFS)
    want = oracle.slice_bursts(b, t)
    assert len(want) > 1000
    assert lf.slice_long(b, t, 0, 0)[0].tobytes() == want.tobytes()
    for mb in (1, 2):
        assert lf.slice_long(b, t, mb, 0)[0].tobytes() == fx.slice_fix(b, t, mb)[0].tobytes()
    eb, et = pc.edge_bursts(4000, 3)
    assert lf.slice_long(eb, et, 0, 0)[0].tobytes() == oracle.slice_bursts(eb, et).tobytes()
    # clean-PI frames: every undamaged DF18 / DF19 burst has syndrome 0 over 112 bits
    raw = lf.slice_raw(b, 3)
    clean = np.array([m[0] in (18, 19) and m[1] == 0 for m in meta])
    assert clean.sum() > 500 and (raw["synd"][clean] == 0).all() and (raw["nbits"][clean] == 112).all()


def test_definition_against_the_reference_slicer_with_header_chips_exchanged(bursts):
    """A DF18 burst with the two chips of bit 3 exchanged, a DF19 burst with those of bits 3 and 4: the header reads 16, which
    the reference takes for a long address/parity reply -- no parity test, 112 bits out.  Its data are our 112 decisions with
    those bits flipped, numlowconf and ref ours, its crc our syndrome XOR syn(3) (XOR syn(4)): for the bursts we accept and for
    those we drop.  None is left out (long_bursts: all chips finite, no pair equal).
    The reference's own slicer hands out message texts (data, crc, ref, time), which carry no numlowconf: data, crc and ref are
    pinned to the reference itself, numlowconf only through oracle.slice_bursts, the project's restatement of the
    reference's slicer in C."""
    b, t, _ = bursts
    raw = lf.slice_raw(b, 3)
    sel = np.nonzero(np.isin(raw["hdr"], (18, 19)))[0]
    kept = set(lf.slice_long(b, t, 0, 3)[1])
    n_acc = sum(1 for i in sel if i in kept)
    assert len(sel) > 2500 and n_acc > 500 and len(sel) - n_acc > 500
    assert all((raw["synd"][i] == 0) == (i in kept) for i in sel)          # (long, not DF11, header bits set: only :182 drops one)
    sw, flipped = lf.as_df16(b[sel], raw["hdr"][sel])
    assert np.isfinite(sw).all() and (sw[:, 16::2] != sw[:, 17::2]).all() and len(sw) == len(sel)      # none left out
    want = np.zeros(len(sel), lf.PK)
    dec = raw["dec"][sel].copy()
    crc = raw["synd"][sel].copy()
    for k, js in enumerate(flipped):
        for j in js:
            dec[k, j] ^= 1
            crc[k] ^= fx.SYN[112][j]
    want["data"] = np.packbits(dec, axis=1)
    want["nbytes"] = 14
    want["df"] = 16
    want["numlowconf"] = raw["nlow"][sel]
    want["crc"] = crc
    want["ref"] = raw["ref"][sel]
    for k in ("sample", "secs", "frac"):
        want[k] = t[k][sel]
    assert (want["data"][:, 0] >> 3 == 16).all()
    # accepted by us <=> our syndrome is 0 <=> the reference's "address" is syn(3) (^ syn(4))
    for k, i in enumerate(sel):
        base = int(np.bitwise_xor.reduce(fx.SYN[112][list(flipped[k])]))
        if i in kept:
            assert int(want["crc"][k]) == base
    got = oracle.slice_bursts(sw, t[sel])
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    if oracle.have_ref():
        texts, acc = oracle.ref_slice_bursts(sw, t[sel])
        assert acc.all() and texts == oracle.format_messages(want)


def test_slicer_work_as_defined(emu_lib, bursts):
    """am_slicer_work -> am_k_slice<FIX, 0, LF> under the emulation: bytes and message texts, every mask x fix 0 / 2."""
    b, t, _ = bursts
    eb, et = pc.edge_bursts(4000, 3)
    ctx = _capi.Context(RATE, 7.0, True, lib=emu_lib)
    seen = set()
    for mask in (0, 1, 2, 3):
        for mb in (0, 2):
            want = lf.slice_long(b, t, mb, mask)[0]
            c18, c19, r18, r19 = lf.counts(want)
            assert (c18 >= 400) == bool(mask & 1) and (c19 >= 400) == bool(mask & 2)
            assert (r18 >= 400) == bool(mask & 1 and mb) and (r19 >= 400) == bool(mask & 2 and mb)
            seen.add(want.tobytes())
            ctx.set_fix_errors(mb)
            ctx.set_long_formats(mask)
            got = ctx.slicer_work(b, t)
            assert got.tobytes() == want.tobytes(), "mask %d fix %d: %d vs %d packets" % (mask, mb, len(got), len(want))
            assert emu_lib.format_messages(got, True) == oracle.format_messages(want)
            if (mask, mb) in ((0, 0), (3, 2)):          # the edge vectors: every format, non-finite chips, ties
                assert ctx.slicer_work(eb, et).tobytes() == lf.slice_long(eb, et, mb, mask)[0].tobytes()
            if mask == 0 and mb == 0:
                assert got.tobytes() == oracle.slice_bursts(b, t).tobytes()
    assert len(seen) == 8                                   # eight expectations, no two alike
    ctx.close()


def test_whole_path_as_defined(emu_lib, capture):
    """4 Msps, 0.2 s: one call, uneven chunks with a flush, and the same with the address gate in mode 2."""
    import air_modes
    iq, truth, sc = capture
    n = len(iq)
    ttl = gc.ttl_samples(TTL_S, RATE)
    want = {(mask, mb): lf.expected(sc, mb, mask) for mask in (0, 3) for mb in (0, 2)}
    c18, c19, r18, r19 = lf.counts(want[(3, 2)])
    assert c18 >= 20 and c19 >= 20 and r18 >= 20, (c18, c19, r18, r19)
    assert want[(0, 0)].tobytes() == oracle.demod(iq, RATE).tobytes()
    assert lf.counts(want[(0, 2)]) == (0, 0, 0, 0)
    # the packets of every other format are what they are with the option off
    for mb in (0, 2):
        on, off = want[(3, mb)], want[(0, mb)]
        assert on[~np.isin(on["df"], (18, 19))].tobytes() == off[~np.isin(off["df"], (18, 19))].tobytes()
    frames = set(x["frame"] for x in truth)
    for p in want[(3, 2)][np.isin(want[(3, 2)]["df"], (18, 19))]:
        assert bytes(p["data"][:14]).hex() in frames and p["crc"] == 0 and p["nbytes"] == 14
    gated = lf.expected(sc, 2, 3, 2, ttl)
    assert lf.counts(gated) == (c18, c19, r18, r19) and len(gated) < len(want[(3, 2)])
    assert set(np.unique(gated["df"])) <= {11, 17, 18, 19}
    gated1 = lf.expected(sc, 2, 1, 2, ttl)                   # DF19 not enabled: an "other", dropped in mode 2
    assert not (gated1["df"] == 19).any() and lf.counts(gated1)[0] == c18
    ctx = _capi.Context(RATE, 7.0, True, lib=emu_lib)
    cuts = [0, 70_001, 70_002, 311_117, 600_000, n - 333, n]
    for (mask, mb), w in want.items():
        if (mask, mb) == (0, 2):                  # (the repair alone: tests/test_fix_errors.py)
            continue
        ctx.set_fix_errors(mb)
        ctx.set_long_formats(mask)
        got = ctx.process_iq(iq, flush=True)
        assert got.tobytes() == w.tobytes(), "mask %d fix %d: %d vs %d packets" % (mask, mb, len(got), len(w))
        assert emu_lib.format_messages(got, True) == oracle.format_messages(w)
        parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.concatenate(parts).tobytes() == w.tobytes()
    ctx.set_address_gate(2, TTL_S)
    for mask, w in ((3, gated), (1, gated1)):
        ctx.set_long_formats(mask)
        assert ctx.process_iq(iq, flush=True).tobytes() == w.tobytes()
        if mask == 3:
            parts = [ctx.process_iq(iq[a:b], flush=(b == n)) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.concatenate(parts).tobytes() == w.tobytes()
    ctx.close()
    q = air_modes.msg_queue()
    rx = air_modes.rx_path(RATE, 7.0, q, use_pmf=True, lib=emu_lib, fix_errors=2, long_formats=(18, 19))
    assert rx.get_long_formats() == 3
    rx.work(iq[:300_001])
    rx.work(iq[300_001:], flush=True)
    got = []
    while not q.empty_p():
        got.append(q.delete_head().to_string())
    assert got == oracle.format_messages(want[(3, 2)])


def test_pipes_and_bank_forward_the_setting(emu_lib, capture):
    import air_modes
    iq, _, sc = capture
    want = lf.expected(sc, 0, 3)
    assert lf.counts(want)[0] >= 20
    pipe = _capi.Pipe(RATE, 7.0, True, depth=2, lib=emu_lib)
    assert pipe.get_long_formats() == 0
    pipe.set_long_formats([18, 19])
    assert pipe.get_long_formats() == 3
    pipe.submit(iq)
    with pytest.raises(_capi.AirModesError) as e:
        pipe.set_long_formats(1)                                        # a batch is in flight
    assert e.value.code == _capi.AM_EINVAL and pipe.get_long_formats() == 3
    pipe.submit(iq)
    assert pipe.collect().tobytes() == want.tobytes() and pipe.collect().tobytes() == want.tobytes()
    with pytest.raises(_capi.AirModesError):
        pipe.set_long_formats(4)
    pipe.close()
    sp = _capi.StreamPipe(RATE, 7.0, True, depth=2, lib=emu_lib)
    assert sp.get_long_formats() == 0
    with pytest.raises(_capi.AirModesError):
        sp.set_long_formats(-1)
    sp.set_long_formats(3)
    assert sp.get_long_formats() == 3
    base = np.ascontiguousarray(iq.view(np.float32))
    cuts = [0, 200_001, 410_000, len(iq)]
    got = sp.run([(base.ctypes.data + 8 * a, b - a) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.concatenate(got).tobytes() == want.tobytes()
    sp.close()
    caps = [iq[:300_000], iq[300_000:], iq[100_000:450_001]]
    qs = [air_modes.msg_queue() for _ in caps]
    air_modes.rx_path_bank(RATE, 7.0, qs, use_pmf=True, lib=emu_lib, long_formats=3).work(caps)
    for q, cap in zip(qs, caps):
        got = []
        while not q.empty_p():
            got.append(q.delete_head().to_string())
        w = lf.expected(lf.scan(cap, RATE), 0, 3)
        assert got == oracle.format_messages(w) and (w["df"] == 18).any()


def test_stream_pipe_refuses_a_new_setting_with_chunks_in_flight(emu_lib, capture):
    iq = capture[0]
    sp = _capi.StreamPipe(RATE, 7.0, True, depth=2, lib=emu_lib)
    base = np.ascontiguousarray(iq.view(np.float32))
    sp.submit_device(base.ctypes.data, 400_000)
    with pytest.raises(_capi.AirModesError) as e:
        sp.set_long_formats(3)
    assert e.value.code == _capi.AM_EINVAL and sp.get_long_formats() == 0
    sp.submit_device(base.ctypes.data + 8 * 400_000, len(iq) - 400_000, flush=True)
    got = np.concatenate([sp.collect(), sp.collect()])
    assert got.tobytes() == oracle.demod(iq, RATE).tobytes()
    sp.set_long_formats(3)
    sp.close()


def test_setters(emu_lib, bursts):
    b, t, _ = bursts
    b, t = b[:800], t[:800]
    ctx = _capi.Context(RATE, 7.0, True, lib=emu_lib)
    assert ctx.get_long_formats() == 0
    for bad in (-1, 4, 18):
        with pytest.raises(_capi.AirModesError) as e:
            ctx.set_long_formats(bad)
        assert e.value.code == _capi.AM_EINVAL and ctx.get_long_formats() == 0
    with pytest.raises(ValueError):
        ctx.set_long_formats([17])
    for v, m in ((3, 3), ([18], 1), ((19,), 2), (0, 0), ([19, 18], 3)):
        ctx.set_long_formats(v)
        assert ctx.get_long_formats() == m
    ctx.reset()
    assert ctx.get_long_formats() == 3
    ctx.set_rate(8e6)
    assert ctx.get_long_formats() == 3
    assert ctx.slicer_work(b, t).tobytes() == lf.slice_long(b, t, 0, 3)[0].tobytes()
    # on, then off, equals fresh; and a new mask takes effect with the next call
    for mask in (1, 0, 2, 0):
        ctx.set_long_formats(mask)
        assert ctx.slicer_work(b, t).tobytes() == lf.slice_long(b, t, 0, mask)[0].tobytes()
    fresh = _capi.Context(RATE, 7.0, True, lib=emu_lib)
    assert fresh.slicer_work(b, t).tobytes() == ctx.slicer_work(b, t).tobytes() == oracle.slice_bursts(b, t).tobytes()
    fresh.close()
    ctx.close()
    assert emu_lib.L.am_get_long_formats(None) == _capi.AM_EINVAL and emu_lib.L.am_set_long_formats(None, 1) == _capi.AM_EINVAL


def _lines(messages, long_formats=3, location=(37.7, -122.4)):
    from air_modes import cpr, msprint, parse
    from air_modes.pubsub import pubsub
    pub = pubsub()
    lines = []
    msprint.output_print(cpr.cpr_decoder(list(location)), pub, callback=lines.append)
    feed = parse.make_parser(pub, long_formats=long_formats)
    for m in messages:
        feed(m)
    return lines


def _squitter(df, field, aa, me):
    body = bytes([(df << 3) | field]) + aa.to_bytes(3, "big") + me.to_bytes(7, "big")
    return body + synth._crc24(body).to_bytes(3, "big")


def test_parser_and_printer():
    from air_modes import parse
    from air_modes.exceptions import NoHandlerError
    ident = (4 << 51) | (3 << 48) | int("".join("%06d" % int(bin(c)[2:]) for c in (1, 2, 3, 49, 50, 51, 32, 32)), 2)
    velocity = (19 << 51) | (1 << 48) | (0 << 42) | (100 << 32) | (1 << 31) | (200 << 21) | (10 << 10)
    msgs = []
    for df, name in ((17, "ca"), (18, "cf"), (19, "af")):
        for me in (ident, velocity):
            fr = _squitter(df, 0, 0xABCDEF, me)
            r = parse.modes_reply(int(fr.hex(), 16), long_formats=3)
            assert r["df"] == df and r[name] == 0 and r["aa"] == 0xABCDEF
            assert r["pi"] == (int(fr.hex(), 16) >> 1) & 0xFFFFFF       # (pi:88:24, as the reference lays out DF17)
            assert r["me"].get_type() == (0x08 if me == ident else 0x09)
            msgs.append("%s 000000 0.5 0 0.25" % fr.hex())
    lines = _lines(msgs)
    assert len(lines) == 6
    assert lines[0].endswith("Type 17 BDS0,8 (ident) from abcdef type LARGE ident ABC123  ")
    assert "Type 17 BDS0,9-1 (track report) from abcdef with velocity" in lines[1]
    for k, df in ((2, 18), (4, 19)):
        assert lines[k] == lines[0].replace("Type 17", "Type %d" % df)
        assert lines[k + 1] == lines[1].replace("Type 17", "Type %d" % df)
    # every control field that carries an extended squitter; the others, and DF19's other application fields, in one line
    for cf in range(8):
        fr = _squitter(18, cf, 0x123456, ident)
        out = _lines(["%s 000000 0.5 0 0.25" % fr.hex()])
        if cf in (0, 1, 2, 5, 6):
            assert out == [lines[0].replace("Type 17", "Type 18").replace("abcdef", "123456")]
        else:
            assert len(out) == 1 and out[0].endswith("Type 18 with CF=%d from 123456 not implemented" % cf)
    for af in range(1, 8):
        fr = _squitter(19, af, 0x00BEEF, velocity)
        r = parse.modes_reply(int(fr.hex(), 16), long_formats=2)
        assert r["af"] == af and "aa" not in r.fields and "me" not in r.fields
        out = _lines(["%s 000000 0.5 0 0.25" % fr.hex()])
        assert len(out) == 1 and out[0].endswith("Type 19 with AF=%d from beef not implemented" % af)
    # the parser's tables are opt-in like the slicing, format by format: without the option a 112-bit DF18 / DF19 message is
    # what it is to the reference's parser (no table, nothing printed), and DF17 does not depend on it
    assert _lines(msgs, long_formats=0) == lines[:2]
    assert _lines(msgs, long_formats=[18]) == lines[:4] and _lines(msgs, long_formats=2) == lines[:2] + lines[4:]
    for df, other in ((18, 2), (19, 1)):
        for mask in (0, other):
            with pytest.raises(NoHandlerError):
                parse.modes_reply(int(_squitter(df, 0, 0xABCDEF, ident).hex(), 16), long_formats=mask)
        with pytest.raises(NoHandlerError):
            parse.modes_reply(int(_squitter(df, 0, 0xABCDEF, ident).hex(), 16))
    with pytest.raises(ValueError):
        parse.make_parser(None, long_formats=4)
    with pytest.raises(ValueError):
        parse.make_parser(None, long_formats=[17])
    # a 56-bit DF18 / DF19 message is what it was with any mask: no table, nothing printed
    for df in (18, 19):
        short = int(_squitter(df, 0, 0xABCDEF, ident)[:7].hex(), 16)
        for mask in (0, 3):
            with pytest.raises(NoHandlerError):
                parse.modes_reply(short, long_formats=mask)
            assert _lines(["%014x 000000 0.5 0 0.25" % short], long_formats=mask) == []


def test_modes_rx_option_parses():
    from air_modes import modes_rx
    ap = modes_rx.build_parser()
    assert ap.parse_args(["-s", "x.cf32"]).long_formats == ()
    assert ap.parse_args(["-s", "x.cf32", "--long-formats", "18,19"]).long_formats == (18, 19)
    assert ap.parse_args(["-s", "x.cf32", "--long-formats", "19"]).long_formats == (19,)
    for bad in ("17", "18,20", "x", ""):
        with pytest.raises(SystemExit):
            ap.parse_args(["-s", "x.cf32", "--long-formats", bad])
    assert _capi.long_formats_mask((18, 19)) == 3 and _capi.long_formats_mask(()) == 0
