"""Shared checks of the raw front end at 64 Msps (am_set_raw_front_end): a stream of sc16 / cs8 / cu8 samples
scanned as it is (am_k_fe3<FMT>, am_k_refine_seg<PMF, FMT>, am_k_extract_slice_iq<32, ..., 1>) against the same stream widened
first (the switch off) and against the oracle on to_cf32(raw).  The same assertions run against the CPU emulation of the kernels
(tests/test_raw_front_end.py) and on the real GPU (tests/test_gpu_raw_front_end.py).  All comparisons are exact."""
import functools

import numpy as np

import oracle
import air_modes
from air_modes import _capi, formats
from air_modes.formats import to_cf32

import formats_common as fc

RATE = 64e6
CPU_CAPTURE = fc.CAPTURES[64]                    # 3 000 000 samples
GPU_CAPTURE = (64e6, 8_000_000, 5000.0)          # several am_k_fe3 steps per workgroup
SC16_OFFSETS = (0, 2, 4, 6, 8, 14)               # byte offsets of a device buffer inside a 16-byte-aligned allocation
BYTE_OFFSETS = (0, 1, 2, 3, 8, 15)
FIRST_CHUNKS = (1, 31, 3071, 3073)


@functools.lru_cache(maxsize=None)
def capture(key, fmt):
    """(raw, iq, the oracle's packets on to_cf32(raw), their texts): computed once per capture and format, never written to."""
    rate, raw = fc.raw_capture(key, fmt)
    assert rate == RATE
    iq = to_cf32(raw, fmt)
    want = oracle.demod(iq, rate, 7.0, True)
    assert len(want) >= 50, "only %d packets in the converted capture" % len(want)
    for a in (raw, iq, want):
        a.setflags(write=False)
    return raw, iq, want, tuple(oracle.format_messages(want))


def offsets_of(fmt):
    return SC16_OFFSETS if fmt == "sc16" else BYTE_OFFSETS


def context(lib, switch=True, rate=RATE, **kw):
    ctx = _capi.Context(rate, 7.0, True, lib=lib, **kw)
    assert ctx.get_raw_front_end() is True                  # the default
    if not switch:
        ctx.set_raw_front_end(False)
    assert ctx.get_raw_front_end() is bool(switch)
    return ctx


def receiver(lib, switch=True, **kw):
    q = air_modes.msg_queue()
    rx = air_modes.rx_path(RATE, 7.0, q, use_pmf=True, lib=lib, **kw)
    if not switch:
        rx.context().set_raw_front_end(False)
    return rx, q


class DeviceCopy(object):
    """The raw array in 'device' memory, its first byte `offset` bytes behind a 16-byte-aligned address."""

    def __init__(self, lib, raw, offset=0):
        b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self.mem = fc.mem_class(lib)(b.size + 48)
        self.offset = (-self.mem.ptr) % 16 + offset
        self.mem.write(self.offset, b)
        self.ptr = self.mem.ptr + self.offset
        assert (self.ptr - offset) % 16 == 0


def feed(rx, raw, fmt, edges, dev=None, rx_time=()):
    """The stream in the chunks edges describe (sample indices), from the host array or from a DeviceCopy; the last chunk flushes.
    Returns the packets and, per call, what the front end of the last scan read."""
    bps = formats.bytes_per_sample(fmt)
    parts, read = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        for tag in rx_time:
            if a <= tag[0] < b:
                rx.set_rx_time(*tag)
        if dev is None:
            parts.append(rx.work(raw[2 * a:2 * b], flush=(b == edges[-1])))
        else:
            parts.append(rx.work_device(dev.ptr + bps * a, b - a, flush=(b == edges[-1]), fmt=fmt))
        read.append(rx.context().last_scan_format())
    return np.concatenate(parts), read


def same_packets(got, want, what):
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), "%s: %d vs %d packets" % (what, len(got), len(want))


# ---- 1. the native route is taken, and only where promised ---------------------------------------------------------------
def check_route(lib):
    n = 60_000
    assert lib.L.am_last_scan_format(None) < 0 and lib.L.am_get_raw_front_end(None) == 0
    for fmt in fc.RAW_FORMATS:
        raw = fc.random_raw(fmt, n, 5)
        code = formats.code(fmt)
        assert code != formats.CF32
        ctx = context(lib)
        assert ctx.last_scan_format() == formats.CF32        # before any scan
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == code
        ctx.process_iq(to_cf32(raw, fmt), flush=True)        # float input
        assert ctx.last_scan_format() == formats.CF32
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == code
        # the switch: survives am_reset and am_set_rate, takes effect with the next stream
        ctx.set_raw_front_end(False)
        ctx.reset()
        assert ctx.get_raw_front_end() is False
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == formats.CF32
        ctx.set_rate(RATE)
        assert ctx.get_raw_front_end() is False
        ctx.set_raw_front_end(True)
        ctx.set_rate(RATE)
        ctx.process_samples(raw, flush=True)
        assert ctx.get_raw_front_end() is True and ctx.last_scan_format() == code
        # another rate: widened first
        ctx.set_rate(20e6)
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == formats.CF32
        ctx.close()
        # the DC blocker: widened first
        ctx = context(lib, use_dcblock=True)
        ctx.process_samples(raw, flush=True)
        assert ctx.last_scan_format() == formats.CF32
        ctx.close()
    # a format change in the middle of a stream: widened from that call on, native again with the next stream
    raw = fc.random_raw("sc16", n, 6)
    ctx = context(lib)
    third = n // 3
    ctx.process_samples(raw[:2 * third])
    assert ctx.last_scan_format() == formats.SC16
    ctx.process_iq(to_cf32(raw[2 * third:4 * third]))
    assert ctx.last_scan_format() == formats.CF32
    ctx.process_samples(raw[4 * third:], flush=True)
    assert ctx.last_scan_format() == formats.CF32
    ctx.process_samples(raw, flush=True)
    assert ctx.last_scan_format() == formats.SC16
    ctx.close()


# ---- 2. packets: switch on == switch off == oracle, host and device input, uneven chunks ---------------------------------------
def check_packets(lib, key, fmt, seed, device):
    raw, _, want, want_texts = capture(key, fmt)
    n = raw.size // 2
    edges = [0] + fc.cut_points(n, seed) + [n]
    dev = DeviceCopy(lib, raw) if device else None
    for switch in (True, False):
        rx, q = receiver(lib, switch)
        got, read = feed(rx, raw, fmt, edges, dev)
        what = "%s, switch %s, %s input" % (fmt, switch, "device" if device else "host")
        same_packets(got, want, what)
        assert tuple(fc.drain(q)) == want_texts, what
        assert set(read) <= {formats.code(fmt) if switch else formats.CF32, formats.CF32}
        assert read[-1] == (formats.code(fmt) if switch else formats.CF32), what
        assert rx.samples == n and rx.packets == len(want)
    return len(want)


# ---- 3. stage level: every candidate record --------------------------------------------------------------------------------
def candidates(lib, raw, fmt, switch):
    ctx = context(lib, switch)
    pk = ctx.process_samples(raw, fmt, flush=True)
    assert ctx.last_scan_format() == (formats.code(fmt) if switch else formats.CF32)
    pos, ref, val, iav = ctx.fetch_candidates()
    ctx.close()
    return pk, pos, ref, val, fc.u32(iav)


def check_stage(lib, raw, fmt, at_least):
    on, off = candidates(lib, raw, fmt, True), candidates(lib, raw, fmt, False)
    assert len(on[1]) >= at_least, "only %d candidates" % len(on[1])
    for a, b, name in zip(on, off, ("packets", "pos", "refined", "valid", "inavg")):
        assert np.array_equal(a, b), "%s: %s differs between the raw and the widened scan" % (fmt, name)
    return len(on[1])


# ---- 4. extraction: bursts and tags ----------------------------------------------------------------------------------------
def check_extraction(lib, key, fmt):
    raw, _, want, _ = capture(key, fmt)
    n = raw.size // 2
    cut = n // 2 + 7
    res = []
    for switch in (True, False):
        ctx = context(lib, switch)
        calls = []
        for a, b in ((0, cut), (cut, n)):
            pk = ctx.process_samples(raw[2 * a:2 * b], fmt, flush=(b == n), keep_tags=True)
            bursts, tags = ctx.fetch_tags()
            calls.append((pk, fc.u32(bursts), tags))
        assert ctx.last_scan_format() == (formats.code(fmt) if switch else formats.CF32)
        ctx.close()
        res.append(calls)
    total = 0
    for (pa, ba, ta), (pb, bb, tb) in zip(*res):
        assert len(ta) >= len(pa) and ba.shape == (len(ta), 240)
        assert np.array_equal(pa, pb) and np.array_equal(ba, bb) and ta.tobytes() == tb.tobytes(), fmt
        total += len(pa)
    assert total == len(want)
    same_packets(np.concatenate([c[0] for c in res[0]]), want, fmt)


# ---- 5. alignment ------------------------------------------------------------------------------------------------------
def check_alignment(lib, key, fmt, offsets):
    """A whole stream in one flushing call from a device buffer at every byte offset."""
    raw, _, want, _ = capture(key, fmt)
    n = raw.size // 2
    for off in offsets:
        dev = DeviceCopy(lib, raw, off)
        ctx = context(lib)
        got = ctx.process_samples_device(dev.ptr, n, fmt, flush=True)
        assert ctx.last_scan_format() == formats.code(fmt)
        ctx.close()
        same_packets(got, want, "%s at byte offset %d" % (fmt, off))


def check_first_chunk(lib, key, fmt, device, lengths=FIRST_CHUNKS):
    raw, _, want, _ = capture(key, fmt)
    n = raw.size // 2
    dev = DeviceCopy(lib, raw) if device else None
    for k in lengths:
        rx, _ = receiver(lib)
        got, read = feed(rx, raw, fmt, [0, k, n], dev)
        assert read[-1] == formats.code(fmt)
        same_packets(got, want, "%s, first chunk of %d samples" % (fmt, k))


# ---- 6. the decode options ride along ---------------------------------------------------------------------------------------
def check_options(lib, key, seed):
    fmt = "sc16"
    raw, _, plain, _ = capture(key, fmt)
    n = raw.size // 2
    edges = [0] + fc.cut_points(n, seed) + [n]
    tag = (100_003, 1_600_000_000, 0.625)
    res = []
    for switch in (True, False):
        rx, q = receiver(lib, switch, fix_errors=2, long_formats=(18, 19), address_gate=1, address_repair=1)
        got, read = feed(rx, raw, fmt, edges, rx_time=(tag,))
        assert read[-1] == (formats.SC16 if switch else formats.CF32)
        ctx = rx.context()
        res.append((got, tuple(fc.drain(q)), ctx.address_gate_stats(), ctx.address_repair_stats(), rx.repaired, rx.gated))
    on, off = res
    assert len(on[0]) >= 50 and np.array_equal(on[0], off[0]) and on[0].tobytes() == off[0].tobytes()
    assert on[1:] == off[1:], (on[2:], off[2:])
    assert on[2]["taught"] > 0 and on[2]["passed"] + on[2]["dropped"] > 0          # the gate saw both kinds of reply
    return len(on[0]), len(plain)


# ---- 7. format change and switch change in the middle of a stream -----------------------------------------------------------
def check_changes(lib, key):
    fmt = "sc16"
    raw, iq, want, want_texts = capture(key, fmt)
    n = raw.size // 2
    a, b, c = n // 4 + 1, n // 2 + 3, 3 * (n // 4)
    rx, q = receiver(lib)
    ctx = rx.context()
    parts = [rx.work(raw[:2 * a])]
    assert ctx.last_scan_format() == formats.SC16
    parts.append(rx.work(iq[a:b]))                           # a float32 chunk: the rest of the stream is widened
    assert ctx.last_scan_format() == formats.CF32
    parts.append(rx.work(raw[2 * b:2 * c]))
    assert ctx.last_scan_format() == formats.CF32
    parts.append(rx.work(raw[2 * c:], flush=True))
    assert ctx.last_scan_format() == formats.CF32
    same_packets(np.concatenate(parts), want, "sc16, float32, sc16")
    assert tuple(fc.drain(q)) == want_texts
    # the switch between two chunks: reported at once, obeyed by the next stream
    for first in (True, False):
        rx, q = receiver(lib, first)
        ctx = rx.context()
        now = formats.SC16 if first else formats.CF32
        parts = [rx.work(raw[:2 * a])]
        assert ctx.last_scan_format() == now
        ctx.set_raw_front_end(not first)
        assert ctx.get_raw_front_end() is (not first)
        parts.append(rx.work(raw[2 * a:2 * c]))
        assert ctx.last_scan_format() == now
        parts.append(rx.work(raw[2 * c:], flush=True))
        assert ctx.last_scan_format() == now
        same_packets(np.concatenate(parts), want, "switch %s -> %s in mid-stream" % (first, not first))
        assert tuple(fc.drain(q)) == want_texts
        same_packets(rx.work(raw, flush=True), want, "the stream after it")
        assert ctx.last_scan_format() == (formats.CF32 if first else formats.SC16)
