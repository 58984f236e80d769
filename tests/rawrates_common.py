"""Shared checks of the raw front end at 2 .. 40 Msps (am_set_raw_front_end level 2): a stream of sc16 / cs8 / cu8
samples scanned as it is (am_k_fe4<SPC, G, NW, FMT>, am_k_extract_slice_iq<SPC, ..., 1>) against the same stream widened first
(levels 1 and 0) and against the oracle on to_cf32(raw).  The same assertions run on the real GPU (tests/test_gpu_raw_rates.py:
every rate, format, offset and chunk length, 14 s) and against the CPU emulation of the kernels (tests/test_raw_rates.py: every
check and every rate, with fewer formats, offsets and lengths at the rates that are slow to emulate -- the whole matrix takes 21
minutes there, nine seconds a scan at 40 Msps).  All comparisons are exact."""
import functools

import numpy as np

import oracle
import air_modes
from air_modes import _capi, formats
from air_modes.formats import to_cf32

import formats_common as fc
import rawfe_common as rc

RATES = (2, 4, 8, 10, 16, 20, 32, 40)            # Msps: the rates am_k_fe4 serves
SOME_RATES = (2, 10, 20, 40)                     # SPC = 1, both odd-R layouts (30 samples per unit), LU = 48
STEP = {2: 3072, 4: 3072, 8: 3072, 10: 3840, 16: 3072, 20: 3840, 32: 3072, 40: 1920}   # samples per front-end step
NOISE_RATES = (20, 40)


def spc_of(msps):
    return msps // 2


def pmf_of(msps):
    return spc_of(msps) > 1


def key_of(msps):
    spc = spc_of(msps)
    n = (200_000 if spc <= 4 else 100_000) * spc
    assert n >= 65 * STEP[msps]                  # interior unguarded steps, a ring-rebuild step and a guarded last step per workgroup
    return (msps * 1e6, n, 2500.0)


@functools.lru_cache(maxsize=None)
def capture(msps, fmt, drop=0):
    """(raw, iq, the oracle's packets on to_cf32(raw), their texts) of the rate's capture without its last `drop` samples:
    computed once, never written to."""
    rate, raw = fc.raw_capture(key_of(msps), fmt)
    assert rate == msps * 1e6
    if drop:
        raw = raw[:raw.size - 2 * drop].copy()
    iq = to_cf32(raw, fmt)
    want = oracle.demod(iq, rate, 7.0, pmf_of(msps))
    assert len(want) >= 50, "only %d packets in the converted capture" % len(want)
    for a in (raw, iq, want):
        a.setflags(write=False)
    return raw, iq, want, tuple(oracle.format_messages(want))


def context(lib, level, msps, **kw):
    ctx = _capi.Context(msps * 1e6, 7.0, pmf_of(msps), lib=lib, **kw)
    assert ctx.raw_front_end_level() == 1 and ctx.get_raw_front_end() is True        # the default
    ctx.set_raw_front_end(level)
    assert ctx.raw_front_end_level() == level and ctx.get_raw_front_end() is bool(level)
    return ctx


def receiver(lib, level, msps, **kw):
    q = air_modes.msg_queue()
    rx = air_modes.rx_path(msps * 1e6, 7.0, q, use_pmf=pmf_of(msps), lib=lib, raw_front_end=level, **kw)
    assert rx.context().raw_front_end_level() == level
    return rx, q


def read_at(level, fmt):
    return formats.code(fmt) if level == 2 else formats.CF32


# ---- 1. the native route is taken, and only where promised ---------------------------------------------------------------
def check_route(lib):
    n = 12_000                                   # 3 to 6 front-end steps at every rate: which kernels run does not depend on more
    for fmt in fc.RAW_FORMATS:
        raw = fc.random_raw(fmt, n, 5)
        code = formats.code(fmt)
        assert code != formats.CF32
        for msps in RATES + (64,):
            for level in (2, 1):
                ctx = context(lib, level, msps)
                want = code if (level == 2 or msps == 64) else formats.CF32
                ctx.process_samples(raw, flush=True)
                assert ctx.last_scan_format() == want, (fmt, msps, level)
                ctx.process_iq(to_cf32(raw, fmt), flush=True)    # float input
                assert ctx.last_scan_format() == formats.CF32
                ctx.process_samples(raw, flush=True)
                assert ctx.last_scan_format() == want, (fmt, msps, level)
                ctx.close()
        # a fractional number of samples per chip (the rate-generic kernels), the DC blocker: widened first at every level
        ctx = _capi.Context(5e6, 7.0, True, lib=lib)
        ctx.set_raw_front_end(2)
        ctx.process_samples(raw, flush=True)
        assert ctx.raw_front_end_level() == 2 and ctx.last_scan_format() == formats.CF32
        ctx.close()
        ctx = context(lib, 2, 20, use_dcblock=True)
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == formats.CF32
        ctx.close()
    # the levels: 0 / 1 / 2 round-trip; every other non-zero value means 1, as before the levels
    ctx = _capi.Context(20e6, 7.0, True, lib=lib)
    for level in (0, 1, 2, 0, 2, 1):
        ctx.set_raw_front_end(level)
        assert ctx.raw_front_end_level() == level and ctx.get_raw_front_end() is bool(level)
    for on, level in ((True, 1), (False, 0)):
        ctx.set_raw_front_end(on)
        assert ctx.raw_front_end_level() == level
    for other in (7, 3, -1, -2):
        ctx.set_raw_front_end(2)
        assert lib.L.am_set_raw_front_end(ctx._h, other) == 0
        assert lib.L.am_get_raw_front_end(ctx._h) == 1 and ctx.raw_front_end_level() == 1
    assert lib.L.am_abi_version() == 5
    # the level survives am_reset and am_set_rate ...
    raw = fc.random_raw("sc16", n, 6)
    ctx.set_raw_front_end(2)
    ctx.reset()
    assert ctx.raw_front_end_level() == 2
    ctx.set_rate(10e6)
    assert ctx.raw_front_end_level() == 2
    ctx.process_samples(raw, flush=True)
    assert ctx.last_scan_format() == formats.SC16
    ctx.set_rate(20e6)
    # ... and takes effect with the next stream, not in mid-stream
    half = n // 2 + 1
    for first, then in ((1, 2), (2, 1), (2, 0), (0, 2)):
        ctx.set_raw_front_end(first)
        now = read_at(first, "sc16")
        ctx.process_samples(raw[:2 * half])
        assert ctx.last_scan_format() == now
        ctx.set_raw_front_end(then)
        assert ctx.raw_front_end_level() == then
        ctx.process_samples(raw[2 * half:], flush=True)
        assert ctx.last_scan_format() == now, (first, then)
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == read_at(then, "sc16"), (first, then)
    ctx.close()
    # rx_path: None leaves the library's default, 0 / 1 / 2 set the level
    q = air_modes.msg_queue()
    assert air_modes.rx_path(20e6, 7.0, q, use_pmf=True, lib=lib).context().raw_front_end_level() == 1
    for level in (0, 1, 2):
        rx = air_modes.rx_path(20e6, 7.0, q, use_pmf=True, lib=lib, raw_front_end=level)
        assert rx.context().raw_front_end_level() == level
    rx.work(raw, flush=True)
    assert rx.context().last_scan_format() == formats.SC16


# ---- 2. packets: level 2 == level 1 == oracle, host and device input, uneven chunks --------------------------------------------
def check_packets(lib, msps, fmt, seed, device):
    raw, _, want, want_texts = capture(msps, fmt)
    n = raw.size // 2
    edges = [0] + fc.cut_points(n, seed) + [n]
    dev = rc.DeviceCopy(lib, raw) if device else None
    for level in (2, 1):
        rx, q = receiver(lib, level, msps)
        got, read = rc.feed(rx, raw, fmt, edges, dev)
        what = "%d Msps, %s, level %d, %s input" % (msps, fmt, level, "device" if device else "host")
        rc.same_packets(got, want, what)
        assert tuple(fc.drain(q)) == want_texts, what
        assert set(read) <= {read_at(level, fmt), formats.CF32}, what
        assert read[-1] == read_at(level, fmt), what
        assert rx.samples == n and rx.packets == len(want)
    return len(want)


# ---- 3. stage level: every candidate record --------------------------------------------------------------------------------
def candidates(lib, msps, raw, fmt, level):
    ctx = context(lib, level, msps)
    pk = ctx.process_samples(raw, fmt, flush=True)
    assert ctx.last_scan_format() == read_at(level, fmt)
    pos, ref, val, iav = ctx.fetch_candidates()
    ctx.close()
    return pk, pos, ref, val, fc.u32(iav)


def check_stage(lib, msps, raw, fmt, at_least):
    on, off = candidates(lib, msps, raw, fmt, 2), candidates(lib, msps, raw, fmt, 0)
    print("%d Msps, %s: %d candidate records" % (msps, fmt, len(off[1])))
    assert len(off[1]) >= at_least, "only %d candidates in the widened scan" % len(off[1])
    for a, b, name in zip(on, off, ("packets", "pos", "refined", "valid", "inavg")):
        assert np.array_equal(a, b), "%d Msps, %s: %s differs between the raw and the widened scan" % (msps, fmt, name)
    return len(on[1])


# ---- 4. extraction: bursts and tags ----------------------------------------------------------------------------------------
def check_extraction(lib, msps, fmt):
    raw, _, want, _ = capture(msps, fmt)
    n = raw.size // 2
    cut = n // 2 + 7
    res = []
    for level in (2, 0):
        ctx = context(lib, level, msps)
        calls = []
        for a, b in ((0, cut), (cut, n)):
            pk = ctx.process_samples(raw[2 * a:2 * b], fmt, flush=(b == n), keep_tags=True)
            bursts, tags = ctx.fetch_tags()
            calls.append((pk, fc.u32(bursts), tags))
        assert ctx.last_scan_format() == read_at(level, fmt)
        ctx.close()
        res.append(calls)
    total = 0
    for (pa, ba, ta), (pb, bb, tb) in zip(*res):
        assert len(ta) >= len(pa) and ba.shape == (len(ta), 240)
        assert np.array_equal(pa, pb) and np.array_equal(ba, bb) and ta.tobytes() == tb.tobytes(), (msps, fmt)
        total += len(pa)
    assert total == len(want)
    rc.same_packets(np.concatenate([c[0] for c in res[0]]), want, "%d Msps, %s" % (msps, fmt))


# ---- 5. alignment ------------------------------------------------------------------------------------------------------
def check_alignment(lib, msps, fmt, offsets=None, odd_sources=("device", "host")):
    """A whole stream in one flushing call from a device buffer at every byte offset, and one of odd length: the source ends in
    half a pair.  (offsets, odd_sources: the emulated twin runs fewer of them at the rates that are slow to emulate.)"""
    raw, _, want, _ = capture(msps, fmt)
    n = raw.size // 2
    for off in (rc.offsets_of(fmt) if offsets is None else offsets):
        dev = rc.DeviceCopy(lib, raw, off)
        ctx = context(lib, 2, msps)
        got = ctx.process_samples_device(dev.ptr, n, fmt, flush=True)
        assert ctx.last_scan_format() == formats.code(fmt)
        ctx.close()
        rc.same_packets(got, want, "%d Msps, %s at byte offset %d" % (msps, fmt, off))
    assert (n - 1) % 2 == 1
    raw1, _, want1, _ = capture(msps, fmt, 1)
    dev = rc.DeviceCopy(lib, raw1)
    ctx = context(lib, 2, msps)
    for source in odd_sources:
        if source == "device":
            got = ctx.process_samples_device(dev.ptr, n - 1, fmt, flush=True)
        else:
            got = ctx.process_samples(raw1, fmt, flush=True)
        assert ctx.last_scan_format() == formats.code(fmt)
        rc.same_packets(got, want1, "%d Msps, %s, %d samples from the %s" % (msps, fmt, n - 1, source))
    ctx.close()


# ---- 6. short first chunks: the second call's view starts at the rounded-down start of the carried tail ---------------------------
def first_chunks(msps):
    spc, T = spc_of(msps), STEP[msps]
    return (1, 7, 49 * spc - 1, 49 * spc + 1, T - 1, T + 1)


def check_first_chunk(lib, msps, fmt, device, lengths=None):
    raw, _, want, _ = capture(msps, fmt)
    n = raw.size // 2
    dev = rc.DeviceCopy(lib, raw) if device else None
    for k in (first_chunks(msps) if lengths is None else lengths):
        rx, _ = receiver(lib, 2, msps)
        got, read = rc.feed(rx, raw, fmt, [0, k, n], dev)
        assert read[-1] == formats.code(fmt)
        rc.same_packets(got, want, "%d Msps, %s, first chunk of %d samples" % (msps, fmt, k))


def check_short_streams(lib, msps, fmt):
    """Whole streams shorter than one front-end step: no error, and the oracle's packets -- none at all in 1 and 31 samples; a step
    less one sample is 1.5 ms of the capture at 2 Msps and may hold a reply."""
    raw = capture(msps, fmt)[0]
    for k in (1, 31, STEP[msps] - 1):
        piece = raw[:2 * k]
        want = oracle.demod(to_cf32(piece, fmt), msps * 1e6, 7.0, pmf_of(msps))
        assert len(want) == 0 or k > 31, (msps, fmt, k)
        ctx = context(lib, 2, msps)
        got = ctx.process_samples(piece, fmt, flush=True)
        rc.same_packets(got, want, "%d Msps, %s, a stream of %d samples from the host" % (msps, fmt, k))
        dev = rc.DeviceCopy(lib, piece)
        got = ctx.process_samples_device(dev.ptr, k, fmt, flush=True)
        rc.same_packets(got, want, "%d Msps, %s, a stream of %d samples from the device" % (msps, fmt, k))
        ctx.close()


# ---- 7. the decode options ride along ---------------------------------------------------------------------------------------
def check_options(lib, seed):
    msps, fmt = 20, "sc16"
    raw, _, plain, _ = capture(msps, fmt)
    n = raw.size // 2
    edges = [0] + fc.cut_points(n, seed) + [n]
    tag = (100_003, 1_600_000_000, 0.625)
    res = []
    for level in (2, 1):
        rx, q = receiver(lib, level, msps, fix_errors=2, long_formats=(18, 19), address_gate=1, address_repair=1)
        got, read = rc.feed(rx, raw, fmt, edges, rx_time=(tag,))
        assert read[-1] == read_at(level, fmt)
        ctx = rx.context()
        res.append((got, tuple(fc.drain(q)), ctx.address_gate_stats(), ctx.address_repair_stats(), rx.repaired, rx.gated))
    on, off = res
    assert len(on[0]) >= 50 and np.array_equal(on[0], off[0]) and on[0].tobytes() == off[0].tobytes()
    assert on[1:] == off[1:], (on[2:], off[2:])
    assert on[2]["taught"] > 0 and on[2]["passed"] + on[2]["dropped"] > 0          # the gate saw both kinds of reply
    return len(on[0]), len(plain)


# ---- 8. format change in the middle of a stream --------------------------------------------------------------------------------
def check_changes(lib):
    msps, fmt = 20, "sc16"
    raw, iq, want, want_texts = capture(msps, fmt)
    n = raw.size // 2
    a, b, c = n // 4 + 1, n // 2 + 3, 3 * (n // 4)
    rx, q = receiver(lib, 2, msps)
    ctx = rx.context()
    parts = [rx.work(raw[:2 * a])]
    assert ctx.last_scan_format() == formats.SC16
    parts.append(rx.work(iq[a:b]))                           # a float32 chunk: the rest of the stream is widened
    assert ctx.last_scan_format() == formats.CF32
    parts.append(rx.work(raw[2 * b:2 * c]))
    assert ctx.last_scan_format() == formats.CF32
    parts.append(rx.work(raw[2 * c:], flush=True))
    assert ctx.last_scan_format() == formats.CF32
    rc.same_packets(np.concatenate(parts), want, "sc16, float32, sc16")
    assert tuple(fc.drain(q)) == want_texts
    rc.same_packets(rx.work(raw, flush=True), want, "the stream after it")
    assert ctx.last_scan_format() == formats.SC16
