#!/usr/bin/env python3
"""What the address gate and the address repair cost ONE stream with chunks in flight (am_spipe_set_address_gate / _repair) at
64 Msps.

One second of the stress capture of tools/bench_gate.py (20 000 bursts/s, SNR 10-35 dB, 200 aircraft; tests/gate_common.py) lies
on the device in two buffers; a pass sends it `--chunks` times over, as the consecutive chunks of ONE stream (bench.py's
pipelined_stream does the same with its batches), through StreamPipe(depth=4).  Legs, each with a pipe of its own: "0" gate off,
"1" mode 1, "1r" mode 1 with the repair.  The legs are interleaved pass by pass in ONE run, every pass starting with another leg, so that
whatever else the machine does -- and whatever a leg's place in the round costs -- hits all of them alike.  The time of a pass is the host clock around StreamPipe.run, which returns with every chunk's
packets; a chunk's time is the pass's divided by its chunks.  Every leg's packets are compared with the definition on the CPU.

--parent-tree DIR adds two legs "parent_a" and "parent_b": the gate-off pipe of ANOTHER checkout of this project (its own
_capi.py and the library built there), twice, interleaved with the others.  "0" against "parent_a" is what this commit costs
the default path; "parent_a" against "parent_b" is the spread the same code shows against itself in the same run, which is the
yardstick for that difference.  No leg's pipe is the first one the process creates (see the comment where that one is made).

Prints one JSON line."""
import argparse
import importlib.util
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
STRESS = (20000.0, (10.0, 35.0), 6401, 200)      # bursts per second, SNR range in dB, seed, aircraft (tools/bench_gate.py)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--passes", type=int, default=30, help="timed passes per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="signal seconds per chunk")
    ap.add_argument("--chunks", type=int, default=8, help="chunks per pass (one stream)")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--ttl", type=float, default=60.0, help="window in seconds")
    ap.add_argument("--parent-tree", default=None, help="another checkout of the project, built: its gate-off pipe, twice")
    ap.add_argument("--no-definition", action="store_true", help="skip the comparison with the definition on the CPU")
    args = ap.parse_args(argv)

    import torch
    import gate_common as gc
    from air_modes import _capi
    if not torch.cuda.is_available():
        raise SystemExit("bench_spipe_gate.py measures on the GPU: no HIP device")
    lam, snr, seed, naddr = STRESS
    nchunks = max(2, args.chunks)
    n = int(round(RATE * args.seconds))
    iq, truth, _ = gc.fleet_capture(RATE, n, lam, seed, naddr, snr)
    lib = _capi.Library()
    # The leg whose pipe was created first has been measured about 27 us per chunk slower than every pipe created after it, the
    # same library or another (profiles/spipe_gate/bench_spipe_gate.txt, runs 1-4; cause unknown).  A throw-away pipe takes that
    # place: it is created first, sent one pass and kept open, idle, until the end.
    first = _capi.StreamPipe(RATE, 7.0, True, depth=args.depth, lib=lib, device=0)
    front = first.front()
    # two buffers with room for the previous chunk's tail in front (the library copies it there): a chunk and the one before it
    # never share a buffer
    dev = []
    for _ in range(2):
        buf = torch.zeros(2 * (front + n), dtype=torch.float32, device="cuda:0")
        buf[2 * front:].copy_(torch.from_numpy(np.ascontiguousarray(iq.view(np.float32))))
        dev.append(buf)
    torch.cuda.synchronize()
    chunks = [(dev[k % 2].data_ptr() + 8 * front, n) for k in range(nchunks)]

    first.run(chunks)
    pipes = {}
    if args.parent_tree:
        spec = importlib.util.spec_from_file_location(
            "parent_capi", os.path.join(args.parent_tree, "gr-air-modes_amd", "air_modes", "_capi.py"))
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        plib = parent.Library(os.path.join(args.parent_tree, "gr-air-modes_amd", "csrc", "libairmodes_hip.so"))
        for leg in ("parent_a", "parent_b"):
            pipes[leg] = parent.StreamPipe(RATE, 7.0, True, depth=args.depth, lib=plib, device=0)
    for leg, mode, repair in (("0", 0, 0), ("1", 1, 0), ("1r", 1, 1)):
        pipes[leg] = _capi.StreamPipe(RATE, 7.0, True, depth=args.depth, lib=lib, device=0)
        pipes[leg].set_address_gate(mode, args.ttl)
        pipes[leg].set_address_repair(repair)

    times = {leg: [] for leg in pipes}
    last = {}
    legs = list(pipes)
    for k in range(args.warmup + args.passes):
        # (every pass starts with another leg: whichever leg follows the host's work between two passes runs slower, and would
        # otherwise always be the same one)
        for leg in legs[k % len(legs):] + legs[:k % len(legs)]:
            pipe = pipes[leg]
            t0 = time.perf_counter()
            got = pipe.run(chunks)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                times[leg].append(dt * 1e3 / nchunks)
            last[leg] = np.concatenate(got)
    out = {"rate": RATE, "seconds_per_chunk": n / RATE, "chunk_samples": n, "chunks_per_pass": nchunks, "depth": args.depth,
           "bursts_per_second": lam, "snr_db": list(snr), "aircraft": naddr, "ttl_seconds": args.ttl, "passes": args.passes,
           "chunks_timed_per_leg": args.passes * nchunks, "legs": {}}
    for leg, pipe in pipes.items():
        t = np.array(times[leg])
        out["legs"][leg] = {"ms_per_chunk_median": float(np.median(t)), "ms_per_chunk_min": float(t.min()),
                            "ms_per_chunk_max": float(t.max()), "gsamples_per_s_median": n / float(np.median(t)) / 1e6,
                            "packets": int(len(last[leg])), "redone": int(pipe.redone())}
        if leg in ("1", "1r"):
            per = args.warmup + args.passes
            st = pipe.address_gate_stats()
            rs = pipe.address_repair_stats()
            out["legs"][leg].update(taught=st["taught"] // per, passed=st["passed"] // per, dropped=st["dropped"] // per,
                                    not_learned=st["not_learned"], repaired=rs["repaired"] // per, ambiguous=rs["ambiguous"] // per)
    med = {leg: out["legs"][leg]["ms_per_chunk_median"] for leg in pipes}
    out["gate_us_per_chunk"] = (med["1"] - med["0"]) * 1e3
    out["repair_us_per_chunk_on_top"] = (med["1r"] - med["1"]) * 1e3
    if args.parent_tree:
        out["this_vs_parent_a_us_per_chunk"] = (med["0"] - med["parent_a"]) * 1e3
        out["this_vs_parent_b_us_per_chunk"] = (med["0"] - med["parent_b"]) * 1e3
        out["parent_vs_itself_us_per_chunk"] = (med["parent_b"] - med["parent_a"]) * 1e3
    if not args.no_definition:
        import aprepair_common as ar
        import oracle
        oracle.build()
        pk = oracle.demod(np.tile(iq, nchunks), RATE, 7.0)
        ttl = gc.ttl_samples(args.ttl, RATE)
        want = {"0": pk, "parent_a": pk, "parent_b": pk, "1": pk[gc.gate(pk, 1, ttl)], "1r": ar.repair(pk, 1, ttl)[0]}
        for leg in pipes:
            out["legs"][leg]["equals_definition"] = bool(want[leg].tobytes() == last[leg].tobytes())
    for pipe in pipes.values():
        pipe.close()
    first.close()
    del dev
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
