"""The raw front end at 2 .. 40 Msps against the staged form ("The raw front end at 2-40 Msps"), on the MI355X:
am_process_samples on device-resident sc16 / cs8 / cu8 samples, whole-stream flushing calls, this checkout's library at level 2
and at level 1 (am_set_raw_front_end) and another build of it (the parent commit's), interleaved in ONE process on the SAME
buffers.

    python tools/bench_raw_rates.py --parent PATH/libairmodes_hip.so [--steps 120] [--rounds 6] [--rates 20,2]
        Per rate and format: two sets of 20 M samples on the device, used in turn.  The configurations
            parent       the other library (it widens every raw stream at these rates with am_k_unpack first)
            level1       this library as it is by default: the same staged form -- the sanity line
            level2       this library with am_set_raw_front_end(2): am_k_fe4<SPC, G, NW, FMT> and am_k_extract_slice_iq<SPC, ..., 1>
                         read the integers
        take turns, `rounds` times `steps / rounds` calls each.  Per configuration: ms per call (host clock around the call,
        which returns when the packets are in host memory) as the median over all calls and as the range of the rounds' medians,
        the dominant kernel's device time (am_last_timing), packets per call (equal everywhere, asserted).
    python tools/bench_raw_rates.py --only level2 --formats sc16 --rates 20 --steps 6 --rounds 1
        a short run of one configuration, for `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.

One JSON line per result on stdout.  No GPU, no numbers: context creation fails."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gr-air-modes_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

FMT_CODE = {"cf32": 0, "sc16": 1, "cs8": 2, "cu8": 3}
AM_F_DEVICE_IN, AM_F_FLUSH = 0x1, 0x2
PACKET_BYTES = 64


class Lib(object):
    """The few entry points the measurement needs, through ctypes alone."""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        L.am_create.restype = C.c_void_p
        L.am_create.argtypes = [C.c_int, C.c_double, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.am_destroy.argtypes = [C.c_void_p]
        L.am_process_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64)]
        L.am_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.am_last_error.restype = C.c_char_p
        L.am_last_error.argtypes = [C.c_void_p]
        L.am_set_raw_front_end.argtypes = [C.c_void_p, C.c_int]
        L.am_get_raw_front_end.argtypes = [C.c_void_p]
        L.am_last_scan_format.argtypes = [C.c_void_p]

    def context(self, rate, level):
        err = C.c_int(0)
        h = self.L.am_create(-1, rate, 7.0, 1, 0, C.byref(err))
        if not h:
            raise RuntimeError("am_create failed: %d" % err.value)
        if level is not None:
            assert self.L.am_set_raw_front_end(h, int(level)) == 0 and self.L.am_get_raw_front_end(h) == int(level)
        return h


class Config(object):
    def __init__(self, name, lib, level):
        self.name, self.lib, self.level = name, lib, level
        self.h = None
        self.cap = 1 << 18
        self.out = np.zeros(self.cap * PACKET_BYTES, np.uint8)
        self.ms, self.dom, self.round_medians, self.packets = [], [], [], None

    def open(self, rate):
        self.close()
        self.h = self.lib.context(rate, self.level)

    def close(self):
        if self.h:
            self.lib.L.am_destroy(self.h)
        self.h = None

    def step(self, ptr, n, fmt):
        got = C.c_uint64(0)
        t0 = time.perf_counter()
        rc = self.lib.L.am_process_samples(self.h, C.c_void_p(ptr), n, fmt, AM_F_DEVICE_IN | AM_F_FLUSH, self.out.ctypes.data, self.cap,
                                           C.byref(got))
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError("%s: am_process_samples: %d %s" % (self.name, rc, self.lib.L.am_last_error(self.h)))
        a, b = C.c_float(0), C.c_float(0)
        self.lib.L.am_last_timing(self.h, C.byref(a), C.byref(b))
        return dt * 1e3, b.value, int(got.value)


def quantise(iq, fmt):
    f = np.ascontiguousarray(iq).view(np.float32).astype(np.float64)
    if fmt == "sc16":
        return np.clip(np.rint(f * 32768.0), -32768, 32767).astype(np.int16)
    if fmt == "cs8":
        return np.clip(np.rint(f * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(f * 128.0 + 127.5), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default=None, help="the other build of the library (the parent commit's)")
    ap.add_argument("--this", default=os.path.join(ROOT, "gr-air-modes_amd", "csrc", "libairmodes_hip.so"))
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--rates", default="20,2", help="Msps")
    ap.add_argument("--lam", type=float, default=5000.0, help="bursts per second")
    ap.add_argument("--formats", default="sc16,cs8,cu8")
    ap.add_argument("--only", default=None, help="comma-separated configurations to run (parent, level1, level2)")
    ap.add_argument("--order", default=None, help="the configurations' order inside a round, e.g. level1,parent,level2 [default: parent,level1,level2]")
    ap.add_argument("--samples", type=int, default=20_000_000)
    ap.add_argument("--base", type=int, default=2_000_000, help="samples synthesised per buffer set; tiled up to --samples on the device")
    args = ap.parse_args()
    import torch
    import synth

    this = Lib(args.this)
    parent = Lib(args.parent) if args.parent else None
    cfgs = []
    if parent:
        cfgs.append(Config("parent", parent, None))
    cfgs += [Config("level1", this, 1), Config("level2", this, 2)]
    if args.only:
        cfgs = [c for c in cfgs if c.name in args.only.split(",")]
    if args.order:                                                       # who goes first in a round (is a difference the turn's or the code's?)
        cfgs.sort(key=lambda c: args.order.split(",").index(c.name))
    n, reps = args.samples, args.samples // args.base
    assert reps * args.base == n and args.steps % args.rounds == 0
    per_round = args.steps // args.rounds
    for msps in [int(x) for x in args.rates.split(",")]:
        rate = msps * 1e6
        for c in cfgs:
            c.open(rate)
        for fmt in args.formats.split(","):
            raws = []
            for k in range(2):
                iq, _ = synth.synth_capture(rate, args.base, args.lam, seed=1300 + k)
                raws.append(torch.from_numpy(quantise(iq, fmt)).cuda().repeat(reps))
            torch.cuda.synchronize()
            for c in cfgs:
                c.ms, c.dom, c.round_medians, c.packets = [], [], [], None
                for k in range(4):                                       # warm-up: buffers, code objects, the capacity estimate
                    c.step(raws[k % 2].data_ptr(), n, FMT_CODE[fmt])
            for r in range(args.rounds):
                for c in cfgs:
                    ms = []
                    for k in range(per_round):
                        t, d, got = c.step(raws[k % 2].data_ptr(), n, FMT_CODE[fmt])
                        ms.append(t)
                        c.dom.append(d)
                        c.packets = (c.packets or {})
                        c.packets[k % 2] = got
                    c.ms += ms
                    c.round_medians.append(float(np.median(ms)))
            for c in cfgs:
                assert c.packets == cfgs[0].packets, (c.name, c.packets, cfgs[0].packets)
                print(json.dumps({"what": "am_process_samples, %d Msps, device input, flushing calls" % msps, "config": c.name,
                                  "format": fmt, "front_end_read": c.lib.L.am_last_scan_format(c.h), "bursts_per_second": args.lam,
                                  "samples": n, "calls": len(c.ms), "ms_per_call_median": float(np.median(c.ms)),
                                  "round_medians_ms": c.round_medians,
                                  "round_medians_range_ms": [float(min(c.round_medians)), float(max(c.round_medians))],
                                  "dominant_kernel_ms_median": float(np.median(c.dom)),
                                  "packets_per_call": [c.packets[k] for k in sorted(c.packets)]}), flush=True)
            del raws
            torch.cuda.empty_cache()
    for c in cfgs:
        c.close()


if __name__ == "__main__":
    main()
