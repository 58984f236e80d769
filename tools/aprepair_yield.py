#!/usr/bin/env python3
"""The yield table of DESIGN.md section 15: what the repair of one wrong bit in an address/parity reply (am_set_address_repair)
recovers, from the CPU oracle's packets and the numpy definition in tests/aprepair_common.py alone -- no library, no GPU.

Captures are those of tests/gate_common.py::fleet_capture, threshold 7 dB (noise alone: 5 dB), mode 1.  One markdown row per
capture and window."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gr-air-modes_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"),
          os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (rate, samples, bursts/s, seed, fleet, SNR), threshold, windows in seconds
ROWS = [((4e6, 8_000_000, 3000.0, 21, 40, (10.0, 35.0)), 7.0, (60.0,)),
        ((4e6, 8_000_000, 4000.0, 22, 40, (4.0, 14.0)), 7.0, (60.0,)),
        ((4e6, 2_000_000, 4000.0, 22, 40, (4.0, 14.0)), 7.0, (60.0,)),
        ((5e6, 3_000_000, 3000.0, 27, 30, (4.0, 14.0)), 7.0, (60.0,)),
        ((20e6, 20_000_000, 5000.0, 23, 60, (6.0, 30.0)), 7.0, (60.0, 0.02)),
        ((64e6, 16_000_000, 20000.0, 24, 30, (6.0, 30.0)), 7.0, (60.0, 0.01)),
        ((4e6, 8_000_000, 0.0, 3, 40, (10.0, 35.0)), 5.0, (60.0,))]


def main():
    import aprepair_common as ar
    import gate_common as gc
    import oracle
    oracle.build()
    print("| rate, samples, bursts/s, seed, fleet, SNR dB | threshold dB | ttl s | AP packets | true AP kept by gate | dropped by gate "
          "| repaired, transmitted | repaired, not transmitted | ambiguous |")
    print("|---|---|---|---|---|---|---|---|---|")
    for args, thr, ttls in ROWS:
        iq, truth, _ = gc.fleet_capture(*args)
        pk = oracle.demod(iq, args[0], thr)
        isap = np.isin(pk["df"], gc.AP)
        true = gc.transmitted(pk, truth)
        for ttl_s in ttls:
            ttl = gc.ttl_samples(ttl_s, args[0])
            k0 = gc.gate(pk, 1, ttl)
            out, keep, fixed, amb = ar.repair(pk, 1, ttl)
            rep = out[out["reserved"][:, 1] != 0]
            t = gc.transmitted(rep, truth)
            print("| %g, %d, %g, %d, %d, %g-%g | %g | %g | %d | %d | %d | %d | %d | %d |"
                  % (args[0], args[1], args[2], args[3], args[4], args[5][0], args[5][1], thr, ttl_s, isap.sum(),
                     (k0 & isap & true).sum(), (isap & ~k0).sum(), t.sum(), (~t).sum(), amb), flush=True)


if __name__ == "__main__":
    main()
