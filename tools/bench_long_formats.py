#!/usr/bin/env python3
"""What the opt-in 112-bit slicing of DF18 / DF19 squitters (am_set_long_formats) costs at 64 Msps.

One second of the benchmark's stress capture (tools/synth.py, 20 000 bursts/s, SNR 10-35 dB, no DF18 / DF19 in it) and of one
where a quarter of the bursts are clean-parity DF18 squitters (tests/longfmt_common.py): the time of one step -- the samples are
on the device; am_process_iq with AM_F_FLUSH; the host clock around a call that returns with the packets, and the HIP events the
library records around the step's device work (am_last_timing) -- for every mask of --masks, interleaved step by step in ONE
run, so that whatever else the machine does hits all of them alike; the packets, and whether they are the definition's.

    python tools/bench_long_formats.py                       mask 0 against mask 3, this checkout
    python tools/bench_long_formats.py --masks 0 --root DIR  mask 0 with the package and the library of the checkout at DIR

The second form is for the parent commit, which has no am_set_long_formats (mask 0 calls no setter): runs of it interleaved with
runs of the first form on one machine show whether this commit's step with the option off lies inside the parent's own
run-to-run spread (profiles/long_formats/bench_long.txt).

Kernel times come from a run of its own under the profiler (no counters in that run):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_long_formats.py --profile
The slicing kernel with the option on is another instantiation (am_k_extract_slice_iq<32, 0, 0, 1>), so the kernel statistics
separate the two by themselves.

Prints one JSON line per capture."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 64e6
DF18_MIX = ((17, 0.45), (18, 0.25), (11, 0.10), (0, 0.05), (4, 0.05), (5, 0.05), (20, 0.025), (21, 0.025))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30, help="timed steps per mask")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="signal seconds per step")
    ap.add_argument("--masks", default="0,3")
    ap.add_argument("--captures", default="stress,df18")
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library run (default: this one)")
    ap.add_argument("--label", default=None)
    ap.add_argument("--profile", action="store_true", help="steps only, mask by mask (for a run under rocprofv3)")
    ap.add_argument("--no-definition", action="store_true", help="skip the comparison with the definition on the CPU")
    args = ap.parse_args(argv)
    root = os.path.abspath(args.root)
    # the generator, the oracle and the definition are this checkout's; the package and its library are --root's
    for p in (os.path.join(HERE, "tests"), os.path.join(HERE, "tools"), os.path.join(HERE, "oracle"),
              os.path.join(root, "gr-air-modes_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)

    import torch
    import synth
    from air_modes import _capi
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_formats.py measures on the GPU: no HIP device")
    lib = _capi.Library()
    masks = [int(m) for m in args.masks.split(",")]
    n = int(round(RATE * args.seconds))
    for name in args.captures.split(","):
        if name == "stress":
            iq = synth.config_capture("64msps", seconds=args.seconds)[1][0]
        else:
            import longfmt_common as lf
            iq = synth.synth_capture(RATE, n, 20000.0, 6418, df_mix=DF18_MIX, frame_fn=lf.frame)[0]
        dev = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
        torch.cuda.synchronize()
        ctxs = {}
        for m in masks:
            ctxs[m] = _capi.Context(RATE, 7.0, True, device=0, lib=lib)
            if m:
                ctxs[m].set_long_formats(m)
        out = {"label": args.label or os.path.basename(root), "capture": name, "rate": RATE, "seconds": args.seconds,
               "steps": args.steps, "masks": {}}
        last, times, dev_ms = {}, {m: [] for m in masks}, {m: [] for m in masks}

        def step(m, timed):
            t0 = time.perf_counter()
            last[m] = ctxs[m].process_iq_device(dev.data_ptr(), n, flush=True)
            dt = time.perf_counter() - t0
            if timed:
                times[m].append(dt * 1e3)
                dev_ms[m].append(ctxs[m].last_timing()[0])

        if args.profile:
            for m in masks:
                for k in range(args.warmup + args.steps):
                    step(m, k >= args.warmup)
        else:
            for k in range(args.warmup + args.steps):
                for m in masks:
                    step(m, k >= args.warmup)
        for m in masks:
            t, d = np.array(times[m]), np.array(dev_ms[m])
            pk = last[m]
            out["masks"][str(m)] = {
                "ms_per_step_median": float(np.median(t)), "ms_per_step_min": float(t.min()), "ms_per_step_max": float(t.max()),
                "device_ms_per_step_median": float(np.median(d)), "device_ms_per_step_min": float(d.min()),
                "packets": int(len(pk)), "long_df18": int(np.count_nonzero((pk["df"] == 18) & (pk["nbytes"] == 14))),
                "long_df19": int(np.count_nonzero((pk["df"] == 19) & (pk["nbytes"] == 14)))}
        for m in masks:
            if m and 0 in masks:
                for key in ("ms_per_step_median", "device_ms_per_step_median"):
                    out["masks"][str(m)][key.replace("_median", "") + "_vs_off"] = out["masks"][str(m)][key] / out["masks"]["0"][key]
        if not args.no_definition:
            import longfmt_common as lf
            import oracle
            oracle.build()
            sc = lf.scan(iq, RATE)
            for m in masks:
                out["masks"][str(m)]["equals_definition"] = bool(lf.expected(sc, 0, m).tobytes() == last[m].tobytes())
        for c in ctxs.values():
            c.close()
        del dev
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
