"""Measurements of the native sample formats ("Native sample formats"), on the MI355X.

    python tools/gpu_native_formats.py kernel [--launches 24]
        am_k_unpack per format on 64 Mi complex samples, rotating over two sets of buffers (every launch moves 640 - 768 MiB,
        past the 256 MiB Infinity Cache), device events around `launches` launches after a warm-up, against a device-to-device
        hipMemcpyAsync of the same output size timed in the same process.  Run it once more under
        `rocprofv3 --kernel-trace --stats -- python tools/gpu_native_formats.py kernel --launches 5` for the kernel's own time.
    python tools/gpu_native_formats.py e2e --mode raw|widen [--tree CHECKOUT] [--repeat 3]
        A stream of 2^22-sample chunks in host memory at 20 and 64 Msps, as cu8 and as sc16:  raw = rx_path.work on the raw
        array;  widen = numpy widening to float32 on the host, then rx_path.work (the only way before am_process_samples;
        --tree runs it on another checkout's package, e.g. the parent commit's).  Samples per second of each; interleave the
        two modes from the calling script.

One JSON line per result on stdout.  No GPU, no numbers: context creation raises."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAW_DTYPE = {"sc16": np.int16, "cs8": np.int8, "cu8": np.uint8}
RAW_BYTES = {"sc16": 4, "cs8": 2, "cu8": 2}


def widen(raw, fmt):
    """The host-side conversion a user of float32-only entry points has to write (the table of air_modes/formats.py)."""
    f = raw.astype(np.float32)
    if fmt == "cu8":
        f -= np.float32(127.5)
    f *= np.float32(2.0 ** -15 if fmt == "sc16" else 2.0 ** -7)
    return f.view(np.complex64)


def quantise(iq, fmt):
    f = np.ascontiguousarray(iq).view(np.float32).astype(np.float64)
    if fmt == "sc16":
        return np.clip(np.rint(f * 32768.0), -32768, 32767).astype(np.int16)
    if fmt == "cs8":
        return np.clip(np.rint(f * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(f * 128.0 + 127.5), 0, 255).astype(np.uint8)


def kernel(args):
    import torch
    from air_modes import _capi, formats
    n = 64 * 1024 * 1024
    sets = 2
    ctx = _capi.Context(64e6, 7.0, True)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    outs = [torch.empty(2 * n, dtype=torch.float32, device="cuda") for _ in range(sets)]
    srcs = [torch.zeros(2 * n, dtype=torch.float32, device="cuda") for _ in range(sets)]
    torch.cuda.synchronize()

    def timed(enqueue, launches):
        for k in range(3):
            enqueue(k)
        ctx.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            for k in range(launches):
                enqueue(k)
                ev[k + 1].record(stream)
        ctx.synchronize()
        return np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(launches)])

    copy_ms = timed(lambda k: ctx.stream_copy(outs[k % sets].data_ptr(), srcs[k % sets].data_ptr(), 8 * n), args.launches)
    copy_bytes = 16 * n
    print(json.dumps({"what": "hipMemcpyAsync device to device", "output_bytes": 8 * n, "bytes_moved": copy_bytes,
                      "launches": args.launches, "ms_median": float(np.median(copy_ms)), "ms_min": float(copy_ms.min()),
                      "ms_max": float(copy_ms.max()), "TBps_median": copy_bytes / np.median(copy_ms) / 1e9}), flush=True)
    for fmt in ("sc16", "cs8", "cu8"):
        rng = np.random.default_rng(64)
        info = np.iinfo(RAW_DTYPE[fmt])
        raws = [torch.from_numpy(rng.integers(info.min, info.max + 1, 2 * n, dtype=RAW_DTYPE[fmt])).cuda() for _ in range(sets)]
        torch.cuda.synchronize()
        ms = timed(lambda k: ctx.unpack(raws[k % sets].data_ptr(), fmt, outs[k % sets].data_ptr(), n_complex=n), args.launches)
        moved = (RAW_BYTES[fmt] + 8) * n
        med = float(np.median(ms))
        print(json.dumps({"what": "am_k_unpack", "format": fmt, "samples": n, "bytes_moved": moved, "launches": args.launches,
                          "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()),
                          "TBps_median": moved / med / 1e9, "share_of_8TBps_peak": moved / med / 1e9 / 8.0,
                          "time_vs_copy": med / float(np.median(copy_ms))}), flush=True)
        del raws
    ctx.close()


def e2e(args):
    import synth
    import air_modes
    chunk, chunks = 1 << 22, args.chunks
    for rate, lam in ((20e6, 5000.0), (64e6, 20000.0)):
        iq, _ = synth.synth_capture(rate, chunk, lam, seed=4100)
        for fmt in ("cu8", "sc16"):
            raw = quantise(iq, fmt)
            rx = air_modes.rx_path(rate, 7.0, air_modes.msg_queue(), use_pmf=True)
            rates, packets = [], 0
            for rep in range(args.repeat + 1):                         # (the first pass warms up: buffers, code objects)
                packets = 0
                t0 = time.perf_counter()
                for k in range(chunks):
                    # the same chunk again and again: a stream of `chunks` x 2^22 samples (the widening is redone every
                    # time, as it would be on a live stream)
                    x = raw if args.mode == "raw" else widen(raw, fmt)
                    packets += len(rx.work(x, flush=(k == chunks - 1)))     # (returns after the device is done)
                dt = time.perf_counter() - t0
                while not rx._queue.empty_p():
                    rx._queue.delete_head()
                if rep:
                    rates.append(chunk * chunks / dt)
            print(json.dumps({"what": "end to end from host memory", "mode": args.mode, "tree": args.tree or "this checkout",
                              "rate_msps": rate / 1e6, "format": fmt, "chunk": chunk, "chunks": chunks, "packets": packets,
                              "samples_per_s": [float(r) for r in rates], "samples_per_s_median": float(np.median(rates))}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--launches", type=int, default=24)
    e = sub.add_parser("e2e")
    e.add_argument("--mode", choices=["raw", "widen"], required=True)
    e.add_argument("--tree", default=None, help="run on this checkout's package instead (e.g. the parent commit's)")
    e.add_argument("--repeat", type=int, default=3)
    e.add_argument("--chunks", type=int, default=16)
    args = ap.parse_args()
    tree = os.path.abspath(getattr(args, "tree", None) or ROOT)
    for p in (os.path.join(tree, "gr-air-modes_amd"), os.path.join(tree, "tools")):
        sys.path.insert(0, p)
    {"kernel": kernel, "e2e": e2e}[args.cmd](args)


if __name__ == "__main__":
    main()
