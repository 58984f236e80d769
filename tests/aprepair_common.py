"""The opt-in repair of one wrong bit in an address/parity reply (am_set_address_repair) restated in numpy.

DEFINITION.  The packets of a stream are formed and gated exactly as tests/gate_common.py says.  Repair is considered only for a
packet p with p.df in {0, 4, 5, 16, 20, 21} that step 2 of the gate drops, with the gate on (mode 1 or 2) and the repair set:
  nbits = 8 * nbytes;  syn(j) = the syndrome of a frame of nbits bits whose only set bit is j (fix_common.SYN);
  candidates j = 5 .. nbits - 1, A_j = p.crc ^ syn(j);
  A_j is live if last[A_j] exists and s - last[A_j] <= ttl_samples -- the map as the gate's own test sees it at p;
  exactly one live j: the packet is kept with bit j of data flipped, crc = A_j, reserved[1] = 1, every other field as sliced;
  none, or more than one: dropped as without the repair; the second case is counted as ambiguous.
A repaired reply does not teach.  Nothing here looks at the library; gate_common is imported, not edited."""
import numpy as np

import fix_common as fx
import gate_common as gc

AP = gc.AP


def address_of(p):
    return (int(p["data"][1]) << 16) | (int(p["data"][2]) << 8) | int(p["data"][3])


def repair(pk, mode, ttl, on=1):
    """The definition over the packets of ONE stream, in stream order; ttl in item counts.
    Returns (out, keep, fixed, ambiguous): out = the packets handed out (the kept ones, repaired ones rewritten), keep = mask
    over pk of the packets handed out, fixed = per packet the bit that was flipped or -1, ambiguous = their number."""
    last = {}
    keep = np.ones(len(pk), bool)
    fixed = np.full(len(pk), -1, np.int64)
    new = pk.copy()
    ambiguous = 0
    if mode == 0:
        return new, keep, fixed, 0
    for i, p in enumerate(pk):
        df = int(p["df"])
        s = int(p["sample"])
        if df in (11, 17):
            if p["crc"] == 0 and p["reserved"][1] == 0:
                last[address_of(p)] = s
        elif df in AP:
            l = last.get(int(p["crc"]))
            keep[i] = l is not None and s - l <= ttl
            if not keep[i] and on:
                nbits = 8 * int(p["nbytes"])
                live = []
                for j in range(5, nbits):
                    l = last.get(int(p["crc"]) ^ int(fx.SYN[nbits][j]))
                    if l is not None and s - l <= ttl:
                        live.append(j)
                if len(live) == 1:
                    j = live[0]
                    keep[i] = True
                    fixed[i] = j
                    new[i]["data"][j >> 3] ^= 0x80 >> (j & 7)
                    new[i]["crc"] = int(p["crc"]) ^ int(fx.SYN[nbits][j])
                    new[i]["reserved"][1] = 1
                elif len(live) > 1:
                    ambiguous += 1
        elif mode == 2:
            keep[i] = False
    return new[keep], keep, fixed, ambiguous


def counts(pk, keep, fixed):
    """What the library's stats add for this stream: (taught, passed, dropped, repaired).  passed: kept by the gate as sliced."""
    teach = np.isin(pk["df"], (11, 17)) & (pk["crc"] == 0) & (pk["reserved"][:, 1] == 0)
    rep = fixed >= 0
    return int(teach.sum()), int((np.isin(pk["df"], AP) & keep & ~rep).sum()), int((~keep).sum()), int(rep.sum())


def brute_force(pk, ttl):
    """Independently of the dict loop, O(n^2): for every address/parity packet whose own address fails, the set of candidate
    bits j whose address's LATEST teach in front of the packet is at most ttl item counts old.  -> {packet index: [j, ...]}"""
    teach = [i for i, q in enumerate(pk) if int(q["df"]) in (11, 17) and q["crc"] == 0 and q["reserved"][1] == 0]
    t_addr = np.array([address_of(pk[i]) for i in teach], np.int64)
    t_s = np.array([int(pk[i]["sample"]) for i in teach], np.int64)
    t_i = np.array(teach, np.int64)
    out = {}

    def alive(addr, i, s):
        m = np.flatnonzero((t_addr == addr) & (t_i < i))
        return len(m) > 0 and s - int(t_s[m[-1]]) <= ttl

    for i, p in enumerate(pk):
        if int(p["df"]) not in AP:
            continue
        s = int(p["sample"])
        if alive(int(p["crc"]), i, s):
            continue
        nbits = 8 * int(p["nbytes"])
        out[i] = [j for j in range(5, nbits) if alive(int(p["crc"]) ^ int(fx.SYN[nbits][j]), i, s)]
    return out


def off_is_subsequence_of_on(pk, keep_off, keep_on, fixed):
    """The packets with the repair off are those with it on, less the repaired ones."""
    return bool((keep_off == (keep_on & (fixed < 0))).all()) and gc.is_subsequence(pk[keep_off], pk[keep_on])
