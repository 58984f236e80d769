"""Shared checks of the resampler's raw entry (am_resampler_work_samples, am_k_resample_raw<FMT> of csrc/am_resample.hip): the
same assertions run against the CPU emulation of the kernel (tests/test_resample_raw.py) and on the real GPU
(tests/test_gpu_resample_raw.py).  The definition is arb_resampler.work_samples (air_modes/resample.py); every comparison is
np.array_equal on the float32 bit patterns, call by call: there is no tolerance anywhere."""
import ctypes as C
import io

import numpy as np

import formats_common as fc
from air_modes import _capi, formats
from air_modes.resample import TAPS_PER_PHASE, arb_resampler, gpu_resampler

FORMATS = ("cf32", "sc16", "cs8", "cu8")
RATIOS = (2.0, 4e6 / 2.4e6, 1.25, 1.0)
BLOCK = 1 << 17
# calls of the history stream: shorter than the carried history, exactly it, one more, a call without outputs (the first:
# one sample), more than a block, and the rest
HISTORY_CALLS = (1, 3, 7, 8, 9, 1000, BLOCK + 3, 777)


def samples(fmt, n, seed):
    """n complex samples of format fmt as a flat component array: seeded random integers over the whole range (cf32: random
    floats over many binades), with the extreme codes planted in the first and the last eight samples and in the middle."""
    if fmt == "cf32":
        rng = np.random.default_rng(seed)
        x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.exp(rng.uniform(-12, 2, n))).astype(np.complex64)
        return x.view(np.float32).copy()
    raw = fc.random_raw(fmt, n, seed)
    info = np.iinfo(raw.dtype)
    mid = {"sc16": 0, "cs8": 0, "cu8": 127}[fmt]
    codes = [info.min, info.max, mid, info.max, info.min, info.min, mid, info.max]
    for at in (0, 2 * n - 16, (n // 2) * 2):
        for k in range(16):
            if 0 <= at + k < raw.size:
                raw[at + k] = codes[(k + k // 8) % 8]
    return raw


def same(got, want):
    got, want = np.ascontiguousarray(got, np.complex64), np.ascontiguousarray(want, np.complex64)
    return got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))


class Feeder(object):
    """One gpu_resampler on the stream of a receive context, with a slab of device memory in front of it: feeds raw components as
    host or as device input at a chosen byte offset from a 16-byte boundary.  Modes of a call: "host" (host in, host out),
    "dev" (device in, output left in the handle's buffer and fetched by a copy on the context's stream, which is ordered
    behind the kernel by nothing but that stream), "devhost" (device in, host out)."""

    def __init__(self, lib, ratio, nbytes):
        self.lib, self.g = lib, gpu_resampler(ratio, lib=lib)
        self.ctx = _capi.Context(4e6, 7.0, True, lib=lib)
        self.g.set_stream(self.ctx.stream())
        self.Mem = fc.mem_class(lib)
        self.mem = self.Mem(nbytes + 64)
        self.pad = (-self.mem.ptr) % 16

    def close(self):
        self.g.set_stream(None)
        self.g.close()
        self.ctx.close()

    def device_output(self, m):
        """The first m samples of the handle's device buffer."""
        if not m:
            return np.zeros(0, np.complex64)
        ptr = int(self.lib.L.am_resampler_device_output(self.g._h) or 0)
        dst = self.Mem(8 * m)
        self.ctx.stream_copy(dst.ptr, ptr, 8 * m)
        self.ctx.synchronize()
        return dst.read()[:8 * m].view(np.complex64).copy()

    def call(self, raw, fmt, mode, flush=False, offset=0):
        """One am_resampler_work_samples call on the components `raw`; returns the outputs (host array)."""
        raw = np.ascontiguousarray(raw)
        n = raw.size // 2
        if mode == "host":
            host = np.zeros(raw.nbytes + offset + 32, np.uint8)
            base = (-host.ctypes.data) % 16 + offset
            host[base:base + raw.nbytes] = raw.view(np.uint8)
            src, flags = host.ctypes.data + base, 0
        else:
            at = self.pad + offset
            self.mem.write(at, raw.view(np.uint8))
            src, flags = self.mem.ptr + at, _capi.AM_F_DEVICE_IN
        if mode == "dev":
            ptr, m = self.g.work_device_samples(src, n, fmt, flush=flush)
            assert ptr or not m
            return self.device_output(m)
        got = C.c_uint64(0)
        out = np.zeros(int((n + TAPS_PER_PHASE) * self.g.ratio) + 16, np.complex64)
        rc = self.lib.L.am_resampler_work_samples(self.g._h, C.c_void_p(src if n else None), n, formats.code(fmt),
                                                  flags | (_capi.AM_F_FLUSH if flush else 0), C.c_void_p(out.ctypes.data),
                                                  out.size, C.byref(got))
        assert rc == 0, (rc, self.lib.L.am_resampler_last_error(self.g._h))
        assert np.all(out[got.value:] == 0)
        return out[:got.value].copy()


def check_stream(lib, ratio, fmt, raw, calls, offsets=(0,), flush=True, inputs=("host", "dev", "devhost")):
    """The stream `raw` cut into `calls` (lengths in samples; the rest follows as a last call) against the definition fed the same
    cuts, call by call.  The calls cycle over the modes `inputs` (Feeder), offsets cycle over `offsets` (bytes)."""
    n = raw.size // 2
    f = Feeder(lib, ratio, raw.nbytes + max(offsets))
    ref = arb_resampler(ratio)
    edges = [0]
    for c in calls:
        if edges[-1] + c < n:
            edges.append(edges[-1] + c)
    edges.append(n)
    outs = []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        last = b == n and flush
        piece = raw[2 * a:2 * b]
        want = ref.work_samples(piece, fmt, flush=last)
        got = f.call(piece, fmt, inputs[k % len(inputs)], flush=last, offset=offsets[k % len(offsets)])
        assert same(got, want), (fmt, ratio, k, a, b, got.size, want.size)
        outs.append(got)
    f.close()
    return np.concatenate(outs)


def check_formats_ratios_history(lib, fmt, ratio):
    """Every format at every ratio, on the history stream: calls of 1, 3, 7, 8, 9, 1000, 2^17 + 3 samples and the rest."""
    n = sum(HISTORY_CALLS)
    raw = samples(fmt, n, 11 + FORMATS.index(fmt))
    whole = arb_resampler(ratio).work_samples(raw, fmt, flush=True)
    got = check_stream(lib, ratio, fmt, raw, HISTORY_CALLS[:-1])
    # (where 1 / ratio is a power of two every read position is exact, and the chunking is invisible to the last bit; elsewhere
    # the carried position rounds differently with other cuts, in the definition as on the GPU)
    assert got.size == whole.size and (same(got, whole) or ratio not in (1.0, 2.0))
    assert abs(whole.size - (n + TAPS_PER_PHASE) * ratio) <= 2
    if fmt == "cf32":
        # the new entry with AM_FMT_CF32 is am_resampler_work
        g = gpu_resampler(ratio, lib=lib)
        x = raw.view(np.complex64)
        assert same(g.work(x), arb_resampler(ratio).work(x))
        g.close()


def check_block_table(lib):
    """One call that spans three blocks in one launch, and the same stream cut around the block boundary."""
    n = 2 * BLOCK + 5
    ratio = 4e6 / 2.4e6
    for fmt in ("cu8", "sc16"):
        raw = samples(fmt, n, 21)
        whole = check_stream(lib, ratio, fmt, raw, (), inputs=("dev",))
        if fmt == "cu8":
            for cut in (BLOCK - 1, BLOCK, BLOCK + 1):
                got = check_stream(lib, ratio, fmt, raw, (cut,), inputs=("dev", "host"))
                # (a cut on the block boundary leaves the blocks, and so every bit, as they were)
                assert got.size == whole.size and (same(got, whole) or cut != BLOCK), cut


def check_table_growth(lib):
    """Calls of 1, 2 and 5 blocks on one handle: the block table outgrows its buffers twice while the stream goes on, and
    shorter calls follow."""
    calls = (100, BLOCK + 7, 4 * BLOCK + 9, 5, 2 * BLOCK)
    raw = samples("cs8", sum(calls) + 3000, 31)
    check_stream(lib, 1.0, "cs8", raw, calls, inputs=("dev", "dev", "dev", "host"))


def check_alignment(lib, fmt):
    """Input offset by one complex sample from a 16-byte boundary, and by one component more: device and host input."""
    bps = formats.bytes_per_sample(fmt)
    raw = samples(fmt, 3001, 41)
    first = check_stream(lib, 4e6 / 2.4e6, fmt, raw, (700, 701, 3, 1100), inputs=("host",))
    for offsets in ((bps,), (bps + bps // 2,), (0, bps // 2, bps, 3 * bps + bps // 2)):
        for inputs in (("dev",), ("host",), ("devhost",)):
            got = check_stream(lib, 4e6 / 2.4e6, fmt, raw, (700, 701, 3, 1100), offsets=offsets, inputs=inputs)
            assert same(got, first), (fmt, offsets, inputs)


def check_flush(lib):
    """Flush with the data, flush on its own, and a second stream on the same handle: it equals a fresh definition."""
    ratio = 1.25
    a, b = samples("cu8", 5000, 51), samples("sc16", 4000, 52)
    f = Feeder(lib, ratio, 64000)
    want_a = arb_resampler(ratio).work_samples(a, "cu8", flush=True)
    want_b = arb_resampler(ratio).work_samples(b, "sc16", flush=True)
    assert same(f.call(a, "cu8", "dev", flush=True), want_a)                   # flush in the same call as the data
    got = [f.call(b[:5000], "sc16", "dev"), f.call(b[5000:], "sc16", "host"), f.call(b[:0], "sc16", "dev", flush=True)]
    ref = arb_resampler(ratio)
    want = [ref.work_samples(b[:5000], "sc16"), ref.work_samples(b[5000:], "sc16"), ref.work_samples(b[:0], "sc16", flush=True)]
    assert all(same(g, w) for g, w in zip(got, want)) and got[2].size > 0      # flush with n == 0 drains only
    assert same(np.concatenate(got), want_b)                                   # ... the second stream is a fresh one
    assert same(f.call(a, "cu8", "host", flush=True), want_a)                  # and so is the third
    # reset in the middle of a stream: the next call starts a new one
    f.call(b[:3000], "sc16", "devhost")
    f.g.reset()
    assert same(f.call(a, "cu8", "dev", flush=True), want_a)
    ref.work_samples(b[:3000], "sc16")
    ref.reset()
    assert same(ref.work_samples(a, "cu8", flush=True), want_a)
    f.close()


def check_mixing(lib):
    """am_resampler_work and am_resampler_work_samples alternate on one handle, formats alternate too: one state."""
    ratio = 4e6 / 2.4e6
    g, ref = gpu_resampler(ratio, lib=lib), arb_resampler(ratio)
    lens = (5, 4000, 9, 2, BLOCK + 1, 1234, 7, 600)
    for k, n in enumerate(lens):
        fmt = FORMATS[k % 4]
        raw = samples(fmt, n, 60 + k)
        last = k == len(lens) - 1
        if fmt == "cf32" and k % 8 == 0:
            got, want = g.work(raw.view(np.complex64)), ref.work(raw.view(np.complex64))     # the old entry
        else:
            got, want = g.work_samples(raw, fmt, flush=last), ref.work_samples(raw, fmt, flush=last)
        assert same(got, want), (k, fmt, n)
        if k == 4:
            x = samples("cf32", 3000, 70).view(np.complex64)
            assert same(g.work(x), ref.work(x))
    g.close()


def check_errors(lib):
    L = lib.L
    f, ref = Feeder(lib, 2.0, 64), arb_resampler(2.0)
    g = f.g
    raw = samples("cu8", 1000, 81)
    out = np.zeros(4096, np.complex64)
    got = C.c_uint64(99)

    def call(ptr, n, fmt, cap=out.size, flags=0):
        got.value = 99
        return L.am_resampler_work_samples(g._h, C.c_void_p(ptr), n, fmt, flags, C.c_void_p(out.ctypes.data), cap, C.byref(got))

    assert same(g.work_samples(raw[:600], "cu8"), ref.work_samples(raw[:600], "cu8"))
    for args in ((raw.ctypes.data, 16, 7), (raw.ctypes.data, 16, -1), (None, 16, formats.CU8), (None, 16, formats.CF32),
                 (raw.ctypes.data, (1 << 31) + 1, formats.CU8)):
        assert call(*args) == _capi.AM_EINVAL and got.value == 0 and L.am_resampler_last_error(g._h)
    assert call(None, 0, formats.CU8) == 0 and got.value == 0               # an empty call is fine
    # the stream after the failed calls is intact
    assert same(g.work_samples(raw[600:1200], "cu8"), ref.work_samples(raw[600:1200], "cu8"))
    # too small an output array: the count needed, and the outputs stay in the handle's buffer
    want = ref.work_samples(raw[1200:], "cu8", flush=True)
    assert call(raw[1200:].ctypes.data, 400, formats.CU8, cap=want.size - 1, flags=_capi.AM_F_FLUSH) == _capi.AM_ECAPACITY
    assert got.value == want.size
    assert same(f.device_output(want.size), want)
    with np.testing.assert_raises(TypeError):
        g.work_samples(raw, "cs8")                                           # the dtype says cu8
    f.close()


def check_device_output(lib):
    """AM_F_DEVICE_OUT: the outputs go to the caller's device memory and nowhere beyond."""
    ratio, n, guard = 2.0, 4001, 8
    raw = samples("cs8", n, 91)
    want = arb_resampler(ratio).work_samples(raw, "cs8", flush=True)
    g = gpu_resampler(ratio, lib=lib)
    Mem = fc.mem_class(lib)
    src, dst = Mem(raw.nbytes + 16), Mem((2 * guard + 2 * want.size) * 4 + 16)
    pad_s, pad_d = (-src.ptr) % 16, (-dst.ptr) % 16
    src.write(pad_s + 2, raw.view(np.uint8))
    dst.fill_u32(fc.SENTINEL)
    got = C.c_uint64(0)
    rc = lib.L.am_resampler_work_samples(g._h, C.c_void_p(src.ptr + pad_s + 2), n, formats.CS8,
                                         _capi.AM_F_DEVICE_IN | _capi.AM_F_DEVICE_OUT | _capi.AM_F_FLUSH,
                                         C.c_void_p(dst.ptr + pad_d + 4 * guard), want.size, C.byref(got))
    assert rc == 0 and got.value == want.size
    g.set_stream(None)                                                         # (waits for the handle's stream)
    words = dst.read()[pad_d:pad_d + (2 * guard + 2 * want.size) * 4].view(np.uint32)
    assert np.array_equal(words[guard:-guard], want.view(np.uint32))
    assert np.all(words[:guard] == fc.SENTINEL) and np.all(words[-guard:] == fc.SENTINEL)
    g.close()


CHECKS = (check_block_table, check_table_growth, check_flush, check_mixing, check_errors, check_device_output)


def check(lib):
    """Everything above on one library."""
    for fmt in FORMATS:
        for ratio in RATIOS:
            check_formats_ratios_history(lib, fmt, ratio)
        check_alignment(lib, fmt)
    for c in CHECKS:
        c(lib)


def check_modes_rx(oracle_mod, tmp_path, monkeypatch, fmt, rate):
    """The command line on a raw file below 4 Msps: no am_unpack and no host wait in front of the interpolator, and the messages
    are the receive path's on arb_resampler.work_samples of the file."""
    from air_modes import modes_rx
    import synth
    iq, _ = synth.synth_capture(rate, 300_000, 2500.0, seed=41)
    raw = fc.quantise(iq, fmt)
    path = tmp_path / ("cap." + fmt)
    raw.tofile(path)
    calls = {"unpack": 0, "synchronize": 0, "work_device_samples": 0}

    def counted(name, fn):
        def wrapper(*args, **kwargs):
            calls[name] += 1
            return fn(*args, **kwargs)
        return wrapper

    monkeypatch.setattr(_capi.Context, "unpack", counted("unpack", _capi.Context.unpack))
    monkeypatch.setattr(_capi.Context, "synchronize", counted("synchronize", _capi.Context.synchronize))
    monkeypatch.setattr(gpu_resampler, "work_device_samples", counted("work_device_samples", gpu_resampler.work_device_samples))
    text = io.StringIO()
    assert modes_rx.main(["-s", str(path), "-r", repr(rate), "--raw", "--chunk", "70001"], out=text) == 0
    assert calls == {"unpack": 0, "synchronize": 0, "work_device_samples": 5}, calls
    up = arb_resampler(4e6 / rate).work_samples(raw, fmt, flush=True)
    want = oracle_mod.format_messages(oracle_mod.demod(up, 4e6, 7.0, True), 4e6)
    assert text.getvalue().splitlines() == want and len(want) > 10
