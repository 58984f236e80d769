"""The resampler in front of the receive path on raw samples ("Resampling raw samples in place"), on the MI355X:
a seeded cu8 capture at 2.4 Msps, resampled to 4 Msps in modes_rx's default chunks of 2^22 samples, input resident on the device.

    python tools/bench_resample_raw.py --parent PATH/libairmodes_hip.so [--steps 60] [--rounds 6]
        Two routes take turns in ONE process on the SAME buffers, `rounds` times `steps / rounds` chunks each:
            parent   the parent commit's library (another build, given by path) driven as modes_rx drove it: am_unpack into a
                     float32 twin, am_synchronize, am_resampler_work(AM_F_DEVICE_IN) -- one launch, three copies and one host
                     wait per block of 2^17 samples
            raw      this checkout's library: am_resampler_work_samples(AM_F_DEVICE_IN) on the context's stream -- one launch
        Two measures per route, host clock per chunk:
            stage    the resampling stage alone, until its output is complete on the device (the raw route does not wait by
                     itself: an am_synchronize stands behind it here, inside the clock)
            chain    the stage and the scan behind it (am_process_iq with AM_F_DEVICE_IN, which returns with the packets)
        The outputs of the two routes are compared bit for bit before anything is timed, the packets of every chunk afterwards.
    python tools/bench_resample_raw.py --only raw --steps 6 --rounds 1
        a short run of one route, for `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.

One JSON line per route and measure on stdout (min, median and max over all chunks, and the range of the rounds' medians), then
the verdict: is the raw route's median below the parent route's minimum?  No GPU, no numbers: context creation fails."""
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

CU8 = 3
AM_F_DEVICE_IN = 0x1
PACKET_BYTES = 64


class Route(object):
    """One library through ctypes alone (the parent's lacks the new entry points), one context and one resampler."""

    def __init__(self, name, path, ratio, taps, raw_route):
        self.name, self.raw_route = name, raw_route
        self.L = L = C.CDLL(path)
        vp, u64 = C.c_void_p, C.c_uint64
        L.am_create.restype = vp
        L.am_create.argtypes = [C.c_int, C.c_double, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.am_destroy.argtypes = [vp]
        L.am_process_iq.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64)]
        L.am_unpack.argtypes = [vp, vp, u64, C.c_int, C.c_uint32, vp]
        L.am_synchronize.argtypes = [vp]
        L.am_resampler_create.restype = vp
        L.am_resampler_create.argtypes = [C.c_int, C.c_double, vp, C.POINTER(C.c_int)]
        L.am_resampler_destroy.argtypes = [vp]
        L.am_resampler_work.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64)]
        L.am_resampler_device_output.restype = vp
        L.am_resampler_device_output.argtypes = [vp]
        err = C.c_int(0)
        self.ctx = L.am_create(-1, 4e6, 7.0, 1, 0, C.byref(err))
        if not self.ctx:
            raise RuntimeError("%s: am_create failed: %d" % (name, err.value))
        self.rs = L.am_resampler_create(-1, ratio, taps.ctypes.data, C.byref(err))
        if not self.rs:
            raise RuntimeError("%s: am_resampler_create failed: %d" % (name, err.value))
        if raw_route:
            L.am_resampler_work_samples.argtypes = [vp, vp, u64, C.c_int, C.c_uint32, vp, u64, C.POINTER(u64)]
            L.am_resampler_set_stream.argtypes = [vp, vp]
            L.am_get_stream.restype = vp
            L.am_get_stream.argtypes = [vp]
            assert L.am_resampler_set_stream(self.rs, L.am_get_stream(self.ctx)) == 0
        self.cap = 1 << 16
        self.out = np.zeros(self.cap * PACKET_BYTES, np.uint8)
        self.got = C.c_uint64(0)
        self.reset_stats()

    def reset_stats(self):
        self.ms = {"stage": [], "chain": []}
        self.round_medians = {"stage": [], "chain": []}
        self.packets = []

    def close(self):
        self.L.am_resampler_destroy(self.rs)
        self.L.am_destroy(self.ctx)

    def stage(self, raw_ptr, n, twin_ptr, wait, host_out=None):
        """The resampling stage on one chunk -> (device pointer, outputs); host_out: a complex64 array that gets a copy."""
        L = self.L
        out, cap = (host_out.ctypes.data, host_out.size) if host_out is not None else (None, 0)
        if self.raw_route:
            rc = L.am_resampler_work_samples(self.rs, raw_ptr, n, CU8, AM_F_DEVICE_IN, out, cap, C.byref(self.got))
            if rc == 0 and wait:
                rc = L.am_synchronize(self.ctx)
        else:
            rc = L.am_unpack(self.ctx, raw_ptr, n, CU8, AM_F_DEVICE_IN, twin_ptr)
            rc = rc or L.am_synchronize(self.ctx)
            rc = rc or L.am_resampler_work(self.rs, twin_ptr, n, AM_F_DEVICE_IN, out, cap, C.byref(self.got))
        if rc != 0:
            raise RuntimeError("%s: stage failed: %d" % (self.name, rc))
        return L.am_resampler_device_output(self.rs), int(self.got.value)

    def scan(self, ptr, m):
        got = C.c_uint64(0)
        rc = self.L.am_process_iq(self.ctx, ptr, m, AM_F_DEVICE_IN, self.out.ctypes.data, self.cap, C.byref(got))
        if rc != 0:
            raise RuntimeError("%s: am_process_iq: %d" % (self.name, rc))
        return int(got.value)

    def step(self, raw_ptr, n, twin_ptr, measure):
        t0 = time.perf_counter()
        ptr, m = self.stage(raw_ptr, n, twin_ptr, wait=(measure == "stage"))
        if measure == "stage":
            dt = time.perf_counter() - t0
            self.scan(ptr, m)                                           # (outside the clock: both routes keep one stream going)
        else:
            self.packets.append(self.scan(ptr, m))
            dt = time.perf_counter() - t0
        return dt * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default=None, help="the parent commit's build of the library")
    ap.add_argument("--this", default=os.path.join(ROOT, "gr-air-modes_amd", "csrc", "libairmodes_hip.so"))
    ap.add_argument("--steps", type=int, default=60, help="chunks per route and measure")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--rate", type=float, default=2.4e6)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--base", type=int, default=1 << 20, help="samples synthesised per buffer; tiled up to --chunk on the device")
    ap.add_argument("--lam", type=float, default=2500.0, help="bursts per second")
    ap.add_argument("--only", default=None, help="comma-separated routes to run (parent, raw)")
    args = ap.parse_args()
    import torch
    import synth
    from air_modes.resample import design_taps

    ratio, taps, n = 4e6 / args.rate, design_taps(), args.chunk
    routes = []
    if args.parent:
        routes.append(Route("parent", args.parent, ratio, taps, False))
    routes.append(Route("raw", args.this, ratio, taps, True))
    if args.only:
        routes = [r for r in routes if r.name in args.only.split(",")]
    assert args.steps % args.rounds == 0 and n % args.base == 0
    per_round = args.steps // args.rounds
    raws = []
    for k in range(2):
        iq, _ = synth.synth_capture(args.rate, args.base, args.lam, seed=1700 + k)
        f = np.ascontiguousarray(iq).view(np.float32).astype(np.float64)
        cu8 = np.clip(np.rint(f * 128.0 + 127.5), 0, 255).astype(np.uint8)
        raws.append(torch.from_numpy(cu8).cuda().repeat(n // args.base))
    twin = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    # the same bits out of both routes, chunk by chunk (and the warm-up: buffers, code objects)
    outs = {}
    for r in routes:
        outs[r.name] = []
        for k in range(4):
            host = np.zeros(int(n * ratio) + 64, np.complex64)
            ptr, m = r.stage(raws[k % 2].data_ptr(), n, twin.data_ptr(), wait=True, host_out=host)
            outs[r.name].append(host[:m].view(np.uint32).copy())
            r.scan(ptr, m)
    names = [r.name for r in routes]
    if len(names) == 2:
        for a, b in zip(outs[names[0]], outs[names[1]]):
            assert np.array_equal(a, b), "the two routes' outputs differ"
    for r in routes:
        r.reset_stats()

    for measure in ("stage", "chain"):
        for rnd in range(args.rounds):
            for r in routes:
                ms = [r.step(raws[k % 2].data_ptr(), n, twin.data_ptr(), measure) for k in range(per_round)]
                r.ms[measure] += ms
                r.round_medians[measure].append(float(np.median(ms)))
    if len(routes) == 2:
        assert routes[0].packets == routes[1].packets and sum(routes[0].packets) > 0, "the two routes' packets differ"
    res = {}
    for measure in ("stage", "chain"):
        for r in routes:
            ms = r.ms[measure]
            res[(r.name, measure)] = ms
            print(json.dumps({"what": "cu8 at %.1f Msps -> 4 Msps, chunks of %d samples, device input" % (args.rate / 1e6, n),
                              "route": r.name, "measure": measure, "chunks": len(ms), "ms_per_chunk_min": float(min(ms)),
                              "ms_per_chunk_median": float(np.median(ms)), "ms_per_chunk_max": float(max(ms)),
                              "round_medians_range_ms": [min(r.round_medians[measure]), max(r.round_medians[measure])],
                              "packets_per_chunk": float(np.mean(r.packets)) if r.packets else None}), flush=True)
    if len(routes) == 2:
        for measure in ("stage", "chain"):
            new, old = float(np.median(res[("raw", measure)])), float(min(res[("parent", measure)]))
            print(json.dumps({"measure": measure, "raw_median_ms": new, "parent_min_ms": old,
                              "raw_median_below_parent_min": bool(new < old)}), flush=True)
    for r in routes:
        r.close()


if __name__ == "__main__":
    main()
