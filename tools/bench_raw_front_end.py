"""The raw front end against the staged form, on the MI355X: am_process_samples at 64 Msps on device-resident
sc16 / cs8 / cu8 samples, this checkout's library against another build of it (the parent commit's), interleaved in ONE process
on the SAME buffers.

    python tools/bench_raw_front_end.py --parent PATH/libairmodes_hip.so [--steps 300] [--rounds 6] [--lams 20000,2000]
        Per format and burst rate: two sets of 64 Mi samples on the device, used in turn (past the 256 MiB Infinity Cache).  The
        configurations
            parent       the other library (it widens every raw stream with am_k_unpack first)
            staged       this library, am_set_raw_front_end(0): the same staged form -- the sanity line
            native       this library as it is: am_k_fe3<FMT> and what follows it read the integers
            cf32         this library on to_cf32 of the same samples (float32 input: no conversion anywhere)
        take turns, `rounds` times `steps / rounds` flushing calls each.  Per configuration: ms per call (host clock around the
        call, which returns when the packets are in host memory) as the median over all calls and as the spread of the rounds'
        medians, the dominant kernel's device time (am_last_timing), packets per call (equal everywhere, asserted).
    python tools/bench_raw_front_end.py --only native --formats sc16 --steps 6 --rounds 1
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
    """The few entry points the measurement needs, through ctypes alone: works on a library that lacks the newer ones."""

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
        self.has_switch = hasattr(L, "am_set_raw_front_end")
        if self.has_switch:
            L.am_set_raw_front_end.argtypes = [C.c_void_p, C.c_int]
            L.am_last_scan_format.argtypes = [C.c_void_p]

    def context(self, switch):
        err = C.c_int(0)
        h = self.L.am_create(-1, 64e6, 7.0, 1, 0, C.byref(err))
        if not h:
            raise RuntimeError("am_create failed: %d" % err.value)
        if switch is not None:
            assert self.L.am_set_raw_front_end(h, int(switch)) == 0
        return h


class Config(object):
    def __init__(self, name, lib, switch, float_input):
        self.name, self.lib, self.float_input = name, lib, float_input
        self.h = lib.context(switch)
        self.cap = 1 << 18
        self.out = np.zeros(self.cap * PACKET_BYTES, np.uint8)
        self.ms, self.dom, self.round_medians, self.packets = [], [], [], None

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
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--lams", default="20000,2000", help="bursts per second: the stress density and the realistic one")
    ap.add_argument("--formats", default="sc16,cs8,cu8")
    ap.add_argument("--only", default=None, help="comma-separated configurations to run (parent, staged, native, cf32)")
    ap.add_argument("--samples", type=int, default=64 * 1024 * 1024)
    ap.add_argument("--base", type=int, default=4 * 1024 * 1024, help="samples synthesised per buffer set; tiled up to --samples on the device")
    args = ap.parse_args()
    import torch
    import synth
    from air_modes.formats import to_cf32

    this = Lib(args.this)
    parent = Lib(args.parent) if args.parent else None
    cfgs = []
    if parent:
        cfgs.append(Config("parent", parent, None, False))
    cfgs += [Config("staged", this, 0, False), Config("native", this, 1, False), Config("cf32", this, 1, True)]
    if args.only:
        cfgs = [c for c in cfgs if c.name in args.only.split(",")]
    n, reps = args.samples, args.samples // args.base
    assert reps * args.base == n and args.steps % args.rounds == 0
    per_round = args.steps // args.rounds
    for lam in [float(x) for x in args.lams.split(",")]:
        for fmt in args.formats.split(","):
            raws, floats = [], []
            for k in range(2):
                iq, _ = synth.synth_capture(64e6, args.base, lam, seed=1200 + k)
                raw = quantise(iq, fmt)
                raws.append(torch.from_numpy(raw).cuda().repeat(reps))
                if any(c.float_input for c in cfgs):
                    floats.append(torch.from_numpy(to_cf32(raw, fmt).view(np.float32)).cuda().repeat(reps))
            torch.cuda.synchronize()
            for c in cfgs:
                c.ms, c.dom, c.round_medians, c.packets = [], [], [], None
                for k in range(4):                                       # warm-up: buffers, code objects, the capacity estimate
                    c.step((floats if c.float_input else raws)[k % 2].data_ptr(), n, 0 if c.float_input else FMT_CODE[fmt])
            for r in range(args.rounds):
                for c in cfgs:
                    ms = []
                    for k in range(per_round):
                        t, d, got = c.step((floats if c.float_input else raws)[k % 2].data_ptr(), n, 0 if c.float_input else FMT_CODE[fmt])
                        ms.append(t)
                        c.dom.append(d)
                        c.packets = (c.packets or {})
                        c.packets[k % 2] = got
                    c.ms += ms
                    c.round_medians.append(float(np.median(ms)))
            for c in cfgs:
                assert c.packets == cfgs[0].packets, (c.name, c.packets, cfgs[0].packets)
                read = this.L.am_last_scan_format(c.h) if c.lib.has_switch else None
                print(json.dumps({"what": "am_process_samples, 64 Msps, device input, flushing calls", "config": c.name, "format": fmt,
                                  "front_end_read": read, "bursts_per_second": lam, "samples": n, "calls": len(c.ms),
                                  "ms_per_call_median": float(np.median(c.ms)), "round_medians_ms": c.round_medians,
                                  "round_spread_ms": float(max(c.round_medians) - min(c.round_medians)),
                                  "dominant_kernel_ms_median": float(np.median(c.dom)),
                                  "packets_per_call": [c.packets[k] for k in sorted(c.packets)]}), flush=True)
            del raws, floats
            torch.cuda.empty_cache()
    for c in cfgs:
        c.lib.L.am_destroy(c.h)


if __name__ == "__main__":
    main()
