#!/usr/bin/env python3
"""What the opt-in address gate (am_set_address_gate) costs at 64 Msps.

For mode = 0, 1, 2 in ONE run, on one second of a fleet capture (tests/gate_common.py) at the benchmark's stress density
(20 000 bursts/s, SNR 10-35 dB) and of a low-SNR one (6-30 dB ... 4-14 dB): the time of one step -- the samples are on the
device; am_process_iq with AM_F_FLUSH; the host clock around a call that returns with the packets, and the HIP events the
library records around the step's device work (am_last_timing) --, the packets, what the gate dropped, and whether the packets
are the definition's.  The modes are interleaved step by step, so that whatever else the machine does hits all three alike.

Kernel times come from a run of its own under the profiler (tracing slows the host; no counters in that run):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_gate.py --profile
The gate's kernels have names of their own (am_k_gate_teach, am_k_gate_test, am_k_gate_ticket) and the slicing kernel is another
instantiation (am_k_extract_slice_iq<32, 0, 1>), so the kernel statistics separate them by themselves.

--repair adds a fourth leg "1r": mode 1 with am_set_address_repair(1), interleaved with the others, so that "1r" against "1" is
what the repair costs on top of the gate (its kernels: am_k_gate_test<1>, am_k_gate_repair, am_k_gate_repair_ticket, and the
slicing kernel's <.., 2> instantiation); its packets are compared with tests/aprepair_common.py.

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
    # name: (bursts per second, SNR range in dB, seed, aircraft)
    "stress": (20000.0, (10.0, 35.0), 6401, 200),
    "low_snr": (6000.0, (4.0, 14.0), 6485, 200),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30, help="timed steps per mode")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="signal seconds per step")
    ap.add_argument("--ttl", type=float, default=60.0, help="window in seconds")
    ap.add_argument("--captures", default="stress,low_snr")
    ap.add_argument("--repair", action="store_true", help="add the leg 1r: mode 1 with am_set_address_repair(1)")
    ap.add_argument("--profile", action="store_true", help="steps only, mode by mode (for a run under rocprofv3)")
    ap.add_argument("--no-definition", action="store_true", help="skip the comparison with the definition on the CPU")
    args = ap.parse_args(argv)

    import torch
    import gate_common as gc
    from air_modes import _capi
    if not torch.cuda.is_available():
        raise SystemExit("bench_gate.py measures on the GPU: no HIP device")
    lib = _capi.Library()
    n = int(round(RATE * args.seconds))
    for name in args.captures.split(","):
        lam, snr, seed, naddr = CAPTURES[name]
        iq, truth, _ = gc.fleet_capture(RATE, n, lam, seed, naddr, snr)
        dev = torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))).to("cuda:0")
        torch.cuda.synchronize()
        ctxs = {}
        for mode in (0, 1, 2):
            ctxs[mode] = _capi.Context(RATE, 7.0, True, device=0, lib=lib)
            ctxs[mode].set_address_gate(mode, args.ttl)
        if args.repair:
            ctxs["1r"] = _capi.Context(RATE, 7.0, True, device=0, lib=lib)
            ctxs["1r"].set_address_gate(1, args.ttl)
            ctxs["1r"].set_address_repair(1)
        out = {"capture": name, "rate": RATE, "seconds": args.seconds, "bursts_per_second": lam, "snr_db": list(snr),
               "aircraft": naddr, "ttl_seconds": args.ttl, "steps": args.steps, "modes": {}}
        last = {}
        times = {m: [] for m in ctxs}
        dev_ms = {m: [] for m in ctxs}

        def step(m, timed):
            t0 = time.perf_counter()
            last[m] = ctxs[m].process_iq_device(dev.data_ptr(), n, flush=True)
            dt = time.perf_counter() - t0
            if timed:
                times[m].append(dt * 1e3)
                dev_ms[m].append(ctxs[m].last_timing()[0])

        if args.profile:
            for m in ctxs:
                for k in range(args.warmup + args.steps):
                    step(m, k >= args.warmup)
        else:
            for k in range(args.warmup + args.steps):
                for m in ctxs:
                    step(m, k >= args.warmup)
        for m in ctxs:
            t, d = np.array(times[m]), np.array(dev_ms[m])
            st = ctxs[m].address_gate_stats()
            per = args.warmup + args.steps
            out["modes"][str(m)] = {
                "ms_per_step_median": float(np.median(t)), "ms_per_step_min": float(t.min()), "ms_per_step_max": float(t.max()),
                "device_ms_per_step_median": float(np.median(d)), "device_ms_per_step_min": float(d.min()),
                "packets": int(len(last[m])), "taught": st["taught"] // per, "passed": st["passed"] // per,
                "dropped": st["dropped"] // per, "not_learned": st["not_learned"]}
            if m == "1r":
                rs = ctxs[m].address_repair_stats()
                out["modes"][m].update(repaired=rs["repaired"] // per, ambiguous=rs["ambiguous"] // per)
        if args.repair:
            for key in ("ms_per_step_median", "device_ms_per_step_median"):
                out["modes"]["1r"][key.replace("_median", "") + "_vs_gate"] = out["modes"]["1r"][key] / out["modes"]["1"][key]
        for m in ("1", "2"):
            for key in ("ms_per_step_median", "device_ms_per_step_median"):
                out["modes"][m][key.replace("_median", "") + "_vs_off"] = out["modes"][m][key] / out["modes"]["0"][key]
        if not args.no_definition:
            import oracle
            oracle.build()
            pk = oracle.demod(iq, RATE, 7.0)
            true = gc.transmitted(pk, truth)
            isap = np.isin(pk["df"], gc.AP)
            out["false_ap_packets_gate_off"] = int((isap & ~true).sum())
            for m in (0, 1, 2):
                k = gc.gate(pk, m, gc.ttl_samples(args.ttl, RATE))
                out["modes"][str(m)]["equals_definition"] = bool(pk[k].tobytes() == last[m].tobytes())
                out["modes"][str(m)]["false_ap_packets_kept"] = int((k & isap & ~true).sum())
            if args.repair:
                import aprepair_common as ar
                want, keep, fixed, amb = ar.repair(pk, 1, gc.ttl_samples(args.ttl, RATE))
                r = want[want["reserved"][:, 1] != 0]
                out["modes"]["1r"].update(equals_definition=bool(want.tobytes() == last["1r"].tobytes()),
                                          repaired_not_transmitted=int((~gc.transmitted(r, truth)).sum()))
        for c in ctxs.values():
            c.close()
        del dev
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
