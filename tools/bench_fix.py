#!/usr/bin/env python3
"""What the opt-in repair of DF11 / DF17 replies (am_set_fix_errors) costs at 64 Msps.

For max_bits = 0, 1, 2 in ONE run, on one second of the benchmark's stress capture (20 000 bursts/s, SNR 10-35 dB) and of a
low-SNR capture (4-14 dB): the time of one step (the samples are on the device; am_process_iq with AM_F_FLUSH, host clock
around a call that returns with the packets), the packets, the repairs, and -- counted on the CPU by the definition in
tests/fix_common.py -- the DF11 / DF17 bursts that entered the search.  The settings are interleaved step by step, so that
whatever else the machine does hits all three alike.

Kernel times come from a run of its own under the profiler (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_fix.py --profile
The three settings launch three kernels of different names (am_k_extract_slice_iq<32, 0 / 1 / 2>), so the kernel statistics
separate them by themselves; --profile runs the steps only, setting by setting.

Prints one JSON line per capture."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gr-air-modes_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"),
          os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

RATE = 64e6
CAPTURES = {
    # name: (bursts per second, SNR range in dB, seed)
    "stress": (20000.0, (10.0, 35.0), 6400),       # synth.CONFIGS["64msps"]: what bench.py times
    "low_snr": (6000.0, (4.0, 14.0), 6484),
}


# the captures of the yield table in DESIGN.md 13: (rate, SNR range, seed); 0.5 s at 4 000 bursts/s, threshold 7 dB, pmf on
YIELD = [(4e6, (4.0, 14.0), 77), (4e6, (8.0, 30.0), 78), (8e6, (4.0, 14.0), 79)]


def yield_table(lib):
    """Packets without and with the repair through the library, and the repaired frames that are not a transmitted frame."""
    import synth
    from air_modes import _capi
    for rate, snr, seed in YIELD:
        iq, truth = synth.synth_capture(rate, int(rate * 0.5), 4000.0, seed, snr_db=snr)
        frames = set(x["frame"] for x in truth)
        ctx = _capi.Context(rate, 7.0, True, device=0, lib=lib)
        row = {"rate": rate, "snr_db": list(snr), "seed": seed, "transmitted": len(truth)}
        for mb in (0, 1, 2):
            ctx.set_fix_errors(mb)
            pk = ctx.process_iq(iq, flush=True)
            rep = pk[pk["reserved"][:, 1] > 0]
            row["packets_%d" % mb] = int(len(pk))
            row["repaired_not_transmitted_%d" % mb] = int(sum(bytes(p["data"][:p["nbytes"]]).hex() not in frames for p in rep))
        ctx.close()
        print(json.dumps(row), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30, help="timed steps per setting")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="signal seconds per step")
    ap.add_argument("--captures", default="stress,low_snr")
    ap.add_argument("--profile", action="store_true", help="steps only, setting by setting (for a run under rocprofv3)")
    ap.add_argument("--yield-table", action="store_true", help="the yield table of DESIGN.md 13 through the library, nothing else")
    ap.add_argument("--no-definition", action="store_true", help="skip the CPU count of the bursts that entered the search")
    args = ap.parse_args(argv)

    import torch
    import synth
    from air_modes import _capi
    if not torch.cuda.is_available():
        raise SystemExit("bench_fix.py measures on the GPU: no HIP device")
    lib = _capi.Library()
    if args.yield_table:
        return yield_table(lib)
    n = int(round(RATE * args.seconds))
    for name in args.captures.split(","):
        lam, snr, seed = CAPTURES[name]
        iq, _ = synth.synth_capture(RATE, n, lam, seed, snr_db=snr)
        dev = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
        torch.cuda.synchronize()
        ctxs = {}
        for mb in (0, 1, 2):
            ctxs[mb] = _capi.Context(RATE, 7.0, True, device=0, lib=lib)
            ctxs[mb].set_fix_errors(mb)
        out = {"capture": name, "rate": RATE, "seconds": args.seconds, "bursts_per_second": lam, "snr_db": list(snr),
               "steps": args.steps, "settings": {}}
        last = {}
        times = {mb: [] for mb in ctxs}
        dom = {mb: [] for mb in ctxs}

        def step(mb, timed):
            t0 = time.perf_counter()
            last[mb] = ctxs[mb].process_iq_device(dev.data_ptr(), n, flush=True)
            dt = time.perf_counter() - t0
            if timed:
                times[mb].append(dt * 1e3)
                dom[mb].append(ctxs[mb].last_dom_ms())

        if args.profile:
            for mb in ctxs:
                for k in range(args.warmup + args.steps):
                    step(mb, k >= args.warmup)
        else:
            for k in range(args.warmup + args.steps):
                for mb in ctxs:
                    step(mb, k >= args.warmup)
        for mb in ctxs:
            pk = last[mb]
            r = pk["reserved"][:, 1]
            t = np.array(times[mb])
            out["settings"][str(mb)] = {
                "ms_per_step_median": float(np.median(t)), "ms_per_step_min": float(t.min()), "ms_per_step_max": float(t.max()),
                "dominant_kernel_ms_median": float(np.median(dom[mb])),
                "packets": int(len(pk)), "repaired_one_bit": int(np.count_nonzero(r == 1)),
                "repaired_two_bits": int(np.count_nonzero(r == 2))}
        base = out["settings"]["0"]["ms_per_step_median"]
        for mb in ("1", "2"):
            out["settings"][mb]["step_vs_off"] = out["settings"][mb]["ms_per_step_median"] / base
        if not args.no_definition:
            import fix_common as fx
            import oracle
            oracle.build()
            bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, int(RATE / 2e6), True), int(RATE / 2e6), 7.0, RATE)
            out["preamble_hits"] = int(len(tags))
            for mb in (0, 1, 2):
                want, _, searched = fx.slice_fix(bursts, tags, mb)
                out["settings"][str(mb)]["entered_search"] = int(searched)
                out["settings"][str(mb)]["equals_definition"] = bool(want.tobytes() == last[mb].tobytes())
        for c in ctxs.values():
            c.close()
        del dev
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
