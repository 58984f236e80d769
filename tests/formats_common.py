"""Shared checks of the native sample formats (air_modes/formats.py, am_unpack, am_process_samples): the same assertions
run against the CPU emulation of the kernels (tests/test_formats.py) and on the real GPU (tests/test_gpu_formats.py).
All comparisons are exact."""
import ctypes as C

import numpy as np

import oracle
import synth
import air_modes
from air_modes import _capi, formats
from air_modes.formats import to_cf32

RAW_FORMATS = ("sc16", "cs8", "cu8")
UNPACK_LENGTHS = (0, 1, 2, 3, 5, 63, 64, 65, 4099, 2 ** 18 + 7)
# rate, n, lam of the captures the packet tests run on (seed 41)
CAPTURES = {2: (2e6, 400_000, 2500.0), 4: (4e6, 600_000, 2500.0), 20: (20e6, 2_000_000, 2500.0), 64: (64e6, 3_000_000, 5000.0)}
SENTINEL = 0x7FC0DEAD


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def quantise(v, fmt):
    """A float capture (complex64) as raw components of format fmt: the converter a radio of that kind would be."""
    f = np.ascontiguousarray(v).view(np.float32).astype(np.float64)
    if fmt == "sc16":
        return np.clip(np.rint(f * 32768.0), -32768, 32767).astype(np.int16)
    if fmt == "cs8":
        return np.clip(np.rint(f * 128.0), -128, 127).astype(np.int8)
    if fmt == "cu8":
        return np.clip(np.rint(f * 128.0 + 127.5), 0, 255).astype(np.uint8)
    raise ValueError(fmt)


def random_raw(fmt, n, seed):
    """n complex samples of seeded random integers over the whole range of the format's component."""
    dt = formats.component_dtype(fmt)
    info = np.iinfo(dt)
    return np.random.default_rng(seed).integers(info.min, info.max + 1, 2 * n, dtype=dt)


class HostMem(object):
    """'Device' memory of the emulated library: host memory."""

    def __init__(self, nbytes):
        self.a = np.zeros(nbytes, np.uint8)
        self.ptr = self.a.ctypes.data

    def write(self, offset, data):
        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.a[offset:offset + b.size] = b

    def fill_u32(self, word):
        self.a.view(np.uint32)[:] = word

    def read(self):
        return self.a.copy()


class TorchMem(object):
    """Device memory of the real library: a torch byte tensor on the current GPU."""

    def __init__(self, nbytes):
        import torch
        self.torch = torch
        self.t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def write(self, offset, data):
        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.t[offset:offset + b.size] = self.torch.from_numpy(b.copy()).cuda()
        self.torch.cuda.synchronize()

    def fill_u32(self, word):
        self.t.view(self.torch.int32).fill_(int(np.uint32(word).view(np.int32)))
        self.torch.cuda.synchronize()

    def read(self):
        self.torch.cuda.synchronize()
        return self.t.cpu().numpy()


def mem_class(lib):
    return HostMem if lib.emulated else TorchMem


def check_unpack_case(lib, ctx, Mem, fmt, n, seed, raw_offsets, extra_bytes, out_offsets):
    """am_unpack == to_cf32 as uint32 for one format and length, for every raw offset (complex samples, plus an extra byte
    where the component is one byte), output offset (complex samples) and for host and device input; the words before and
    behind the output keep their value."""
    bps = formats.bytes_per_sample(fmt)
    raw = random_raw(fmt, n, seed)
    # both ends of the integer range occur in every case that has room for them
    if raw.size >= 4:
        info = np.iinfo(raw.dtype)
        raw[0], raw[-1], raw[1], raw[-2] = info.min, info.max, info.max, info.min
    want = u32(to_cf32(raw, fmt))
    rawb = raw.view(np.uint8)
    guard = 8                                                    # words either side of the output
    out = Mem((guard + 2 * max(out_offsets) + 2 * n + guard) * 4)
    host = np.zeros(max(raw_offsets) * bps + max(extra_bytes) + rawb.size + 16, np.uint8)
    dev = Mem(host.size)
    L = lib.L
    cases = 0
    for ro in raw_offsets:
        for xb in extra_bytes:
            off = ro * bps + xb
            host[:] = 0xA5
            host[off:off + rawb.size] = rawb
            dev.write(0, host)
            for oo in out_offsets:
                for device_in in (False, True):
                    out.fill_u32(SENTINEL)
                    src = (dev.ptr if device_in else host.ctypes.data) + off
                    rc = L.am_unpack(ctx._h, C.c_void_p(src), n, formats.code(fmt),
                                     _capi.AM_F_DEVICE_IN if device_in else 0, C.c_void_p(out.ptr + (guard + 2 * oo) * 4))
                    assert rc == 0, (rc, L.am_last_error(ctx._h))
                    ctx.synchronize()
                    got = out.read().view(np.uint32)
                    a = guard + 2 * oo
                    what = (fmt, n, ro, xb, oo, device_in)
                    assert np.array_equal(got[a:a + 2 * n], want), what
                    assert np.all(got[:a] == SENTINEL) and np.all(got[a + 2 * n:] == SENTINEL), what
                    cases += 1
    return cases


def check_unpack(lib, fmt, lengths=UNPACK_LENGTHS):
    ctx = _capi.Context(2e6, 7.0, True, lib=lib)
    Mem = mem_class(lib)
    extra = (0, 1) if formats.bytes_per_sample(fmt) == 2 else (0,)
    total = 0
    for k, n in enumerate(lengths):
        total += check_unpack_case(lib, ctx, Mem, fmt, n, 1000 + k, tuple(range(8)), extra, tuple(range(4)))
    ctx.close()
    assert total == len(lengths) * 8 * len(extra) * 4 * 2


def raw_capture(key, fmt):
    rate, n, lam = CAPTURES[key] if not isinstance(key, tuple) else key
    iq, _ = synth.synth_capture(rate, n, lam, seed=41)
    raw = quantise(iq, fmt)
    info = np.iinfo(raw.dtype)
    assert ((raw == info.min) | (raw == info.max)).any()            # the strongest bursts clip: the ends of the integer range occur
    return rate, raw


def cut_points(n, seed, pieces=9):
    """Chunk boundaries from a seeded generator: uneven, some chunks of one sample, some of odd length."""
    rng = np.random.default_rng(seed)
    cuts = sorted(set(int(c) for c in rng.integers(1, n - 1, pieces)))
    extra = []
    for c in cuts[::3]:
        extra += [c + 1, c + 2]                                     # two chunks of length 1 behind every third cut
    cuts = sorted(set(cuts + [c for c in extra if c < n]) | {1})    # (and the stream's first sample on its own)
    lens = np.diff([0] + cuts + [n])
    assert (lens == 1).sum() >= 3 and (lens % 2 == 1).sum() >= 4 and lens.min() >= 1
    return cuts


def drain(q):
    texts = []
    while not q.empty_p():
        texts.append(q.delete_head().to_string())
    return texts


def check_packets(lib, key, fmt, seed, use_pmf=True, use_dcblock=False, rx_time=None, shape2=False):
    """rx_path.work fed the raw array in uneven chunks == the oracle on to_cf32(raw) == rx_path.work(to_cf32(raw)) in one
    call: every field of every packet, and the texts in the queue."""
    rate, raw = raw_capture(key, fmt)
    n = raw.size // 2
    iq = to_cf32(raw, fmt)
    tags = [rx_time] if rx_time else []
    want = oracle.demod(iq, rate, 7.0, use_pmf, use_dcblock=use_dcblock, rx_time=tags or None)
    assert len(want) >= 50, "only %d packets in the converted capture" % len(want)
    want_texts = oracle.format_messages(want)

    q1 = air_modes.msg_queue()
    rx1 = air_modes.rx_path(rate, 7.0, q1, use_pmf=use_pmf, use_dcblock=use_dcblock, lib=lib)
    one = rx1.work(iq, flush=True, rx_time=tags)
    assert np.array_equal(one, want), "float path differs from the oracle (%d vs %d packets)" % (len(one), len(want))
    assert drain(q1) == want_texts

    q2 = air_modes.msg_queue()
    rx2 = air_modes.rx_path(rate, 7.0, q2, use_pmf=use_pmf, use_dcblock=use_dcblock, lib=lib)
    edges = [0] + cut_points(n, seed) + [n]
    parts = []
    for a, b in zip(edges[:-1], edges[1:]):
        piece = raw[2 * a:2 * b]
        if shape2:
            piece = piece.reshape(-1, 2)
        parts.append(rx2.work(piece, flush=(b == n), rx_time=[t for t in tags if a <= t[0] < b]))
    got = np.concatenate(parts)
    assert np.array_equal(got, want), "raw %s path differs (%d vs %d packets)" % (fmt, len(got), len(want))
    assert got.tobytes() == want.tobytes()
    assert drain(q2) == want_texts
    assert rx2.samples == n and rx2.packets == len(want)
    return len(want)
