"""The opt-in repair of DF11 / DF17 replies (am_set_fix_errors) restated in numpy, and the bursts the tests feed it.

DEFINITION.  A burst is sliced as lib/slicer_impl.cc does (:67-100 the chip-pair decision, :128-171 reference level, length
from the first five bits, decisions, low-confidence count, the all-zero test and the two low-confidence drops), its syndrome
S is formed (:173-177).  Only where :182 drops the packet -- S != 0 and DF 11 or 17 -- and max_bits >= 1:
  candidates are the bit positions 5 .. nbits-1;  syn(j) = the syndrome of the frame whose only set bit is j;
  1. if some a has syn(a) == S, bit a is flipped (DF11 and DF17);
  2. otherwise, max_bits == 2 and DF17: if some a < b have syn(a) ^ syn(b) == S, both are flipped;
  3. otherwise the packet is dropped as before.
A repaired packet has data = the repaired bits, crc = 0, reserved[1] = bits flipped, everything else as sliced.

Nothing here looks at the library: the CRC is bit-serial (crc_serial), the search is a plain search over the candidates.
slice_fix(..., 0) must equal oracle.slice_bursts byte for byte (tests/test_fix_errors.py proves that first)."""
import numpy as np

import oracle
import synth

PK = oracle.PACKET_DTYPE
f32 = np.float32
GEN = 0x1FFF409                      # x^24 + generator 0xFFF409 (lib/modes_crc.cc)


def crc_serial(bits):
    """Remainder of the frame (bits, MSB first, parity field included) modulo the generator, one bit at a time."""
    reg = 0
    for b in bits:
        reg = (reg << 1) | int(b)
        if reg & (1 << 24):
            reg ^= GEN
    return reg


def syn_table(nbits):
    """syn(j), j = 0 .. nbits-1: the syndrome of a frame of nbits bits whose only set bit is j."""
    out = np.zeros(nbits, np.int64)
    for j in range(nbits):
        unit = np.zeros(nbits, np.uint8)
        unit[j] = 1
        out[j] = crc_serial(unit)
    return out


SYN = {56: syn_table(56), 112: syn_table(112)}
# pair syndromes over the candidates 5 .. nbits-1, upper triangle only (a < b); -1 elsewhere (no syndrome is negative)
PAIR = {}
for _n, _s in SYN.items():
    _c = _s[5:]
    _m = _c[:, None] ^ _c[None, :]
    _m[np.tril_indices(len(_c))] = -1
    PAIR[_n] = _m


def slice_all(bursts):
    """slicer_impl.cc:67-100,128-159 for every burst: (ref[n], decisions[n, 112], low-confidence[n, 112], nbits[n])."""
    b = np.ascontiguousarray(bursts, f32).reshape(-1, 240)
    with np.errstate(all="ignore"):
        s = (((b[:, 0] + b[:, 2]).astype(f32) + b[:, 7]).astype(f32) + b[:, 9]).astype(f32)        # :128-131
        ref = (s.astype(np.float64) / 4.0).astype(f32)
        hi = (ref.astype(np.float64) * 1.414).astype(f32)[:, None]                                # :71
        lo = (ref.astype(np.float64) * 0.707).astype(f32)[:, None]                                # :72
        half = lo.astype(np.float64) * 0.5                                                         # :92,:95
        c0, c1 = b[:, 16::2], b[:, 17::2]
        in0 = (c0 > lo) & (c0 < hi)
        in1 = (c1 > lo) & (c1 < hi)
        gt = c0 > c1
        dec = np.where(in0 & ~in1, True, np.where(in1 & ~in0, False, gt))                          # :74-98
        loser = np.where(gt, c1, c0).astype(np.float64)
        conf = np.where(in0 ^ in1, True, np.where(in0 & in1, False, loser < half))
    hdr = np.zeros(len(b), np.int64)
    for j in range(5):
        hdr = (hdr << 1) | dec[:, j]
    nbits = np.where(np.isin(hdr, (16, 17, 20, 21)), 112, 56)                                      # :135-140
    return ref, dec.astype(np.uint8), ~conf, nbits


def find_repair(nbits, syndrome, two):
    """Plain search: () if none, (a,) or (a, b): the positions whose flipping clears the syndrome."""
    syn = SYN[nbits]
    one = np.nonzero(syn[5:] == syndrome)[0]
    if len(one):
        return (int(one[0]) + 5,)
    if two:
        ab = np.argwhere(PAIR[nbits] == syndrome)
        if len(ab):
            return (int(ab[0, 0]) + 5, int(ab[0, 1]) + 5)
    return ()


def slice_fix(bursts, tags, max_bits):
    """The definition: (packets, index of each packet's burst, syndromes that entered the search)."""
    ref, dec, low, nbits = slice_all(bursts)
    n = len(nbits)
    long_ = nbits == 112
    dec = dec.copy()
    low = low.copy()
    dec[~long_, 56:] = 0
    low[~long_, 56:] = False
    nlow = np.minimum(low.sum(axis=1), 24)                                                         # :157
    mt = np.zeros(n, np.int64)
    for j in range(5):
        mt = (mt << 1) | dec[:, j]
    # syndrome = XOR of syn(j) over the set bits (checked against crc_serial in the tests)
    table = np.zeros((n, 112), np.int64)
    table[long_] = SYN[112]
    table[~long_, :56] = SYN[56]
    synd = np.bitwise_xor.reduce(np.where(dec == 1, table, 0), axis=1)
    ok = dec.any(axis=1)                                                                           # :162-166
    ok &= ~(~long_ & (mt != 11) & (nlow > 0))                                                      # :170
    ok &= ~((mt == 11) & (nlow >= 10))                                                             # :171
    bad = ok & (synd != 0) & ((mt == 11) | (mt == 17))                                             # :182
    fixed = np.zeros(n, np.uint8)
    searched = 0
    for i in np.nonzero(bad)[0]:
        sol = ()
        if max_bits >= 1:
            searched += 1
            sol = find_repair(int(nbits[i]), int(synd[i]), max_bits >= 2 and mt[i] == 17)
        if not sol:
            ok[i] = False
            continue
        for a in sol:
            dec[i, a] ^= 1
        synd[i] = 0
        fixed[i] = len(sol)
    idx = np.nonzero(ok)[0]
    out = np.zeros(len(idx), PK)
    out["data"] = np.packbits(dec[idx], axis=1)
    out["nbytes"] = nbits[idx] // 8
    out["df"] = mt[idx]
    out["numlowconf"] = nlow[idx]
    out["reserved"][:, 1] = fixed[idx]
    out["crc"] = synd[idx]
    out["ref"] = ref[idx]
    for k in ("sample", "secs", "frac"):
        out[k] = tags[k][idx]
    return out, idx, searched


def repaired_counts(pk):
    """(one-bit DF11, one-bit DF17, two-bit) repairs in a packet list."""
    r = pk["reserved"][:, 1]
    return (int(np.count_nonzero((r == 1) & (pk["df"] == 11))), int(np.count_nonzero((r == 1) & (pk["df"] == 17))),
            int(np.count_nonzero(r == 2)))


def exchange_chips(bursts, pk, idx):
    """For every repaired packet: its burst with the two chips of each repaired bit exchanged (slicer_impl.cc:74-98: all
    four branches then flip the decision and keep the confidence -- for finite, unequal chips).  Returns (bursts, tags index,
    packets) of the repaired ones that qualify, and the number left out."""
    _, dec, _, _ = slice_all(bursts)
    rows, keep, left_out = [], [], 0
    for k in np.nonzero(pk["reserved"][:, 1])[0]:
        i = idx[k]
        nb = int(pk["nbytes"][k]) * 8
        js = np.nonzero(np.unpackbits(pk["data"][k][:nb // 8]) != dec[i, :nb])[0]
        assert len(js) == pk["reserved"][k, 1] and js.min() >= 5
        b = np.array(bursts[i], f32)
        c0, c1 = b[16 + 2 * js].copy(), b[17 + 2 * js].copy()
        if not (np.isfinite(c0).all() and np.isfinite(c1).all() and (c0 != c1).all()):
            left_out += 1
            continue
        b[16 + 2 * js], b[17 + 2 * js] = c1, c0
        rows.append(b)
        keep.append(k)
    return np.array(rows, f32).reshape(-1, 240), idx[keep], pk[keep], left_out


def damaged_bursts(n, seed):
    """Valid DF17 (70 %) / DF11 frames with 0-3 wrong bits: the wrong bits low-confidence (both chips inside the 3 dB window),
    or one of them confidently wrong, or one in the DF field; 0-30 further low-confidence bits that are right; reference
    levels over four decades.  -> (bursts, tags, meta[(df, wrong bits, style, transmitted frame)])."""
    rng = np.random.default_rng(seed)
    bursts = np.zeros((n, 240), f32)
    tags = np.zeros(n, oracle.TAG_DTYPE)
    tags["sample"] = np.arange(n, dtype=np.uint64) * 4801 + 7
    tags["secs"] = rng.integers(0, 1 << 33, n)
    tags["frac"] = rng.random(n)
    meta = []
    for i in range(n):
        df = 17 if rng.random() < 0.7 else 11
        frame = synth.make_frame(rng, df)
        bits = np.unpackbits(np.frombuffer(frame, np.uint8))
        nb = len(bits)
        scale = f32(10.0 ** rng.uniform(-3, 1))
        pre = (f32(1.0) + rng.uniform(-0.1, 0.1, 4).astype(f32)) * scale
        bb = bursts[i]
        bb[:16] = rng.uniform(0, 0.1, 16).astype(f32) * scale
        bb[[0, 2, 7, 9]] = pre
        ref = f32(np.float64(f32(f32(f32(pre[0] + pre[1]) + pre[2]) + pre[3])) / 4.0)
        strong = ref * (f32(1.0) + rng.uniform(-0.15, 0.15, 112).astype(f32))
        weak = ref * f32(0.3) * rng.uniform(0, 0.9, 112).astype(f32)
        tx = np.zeros(112, np.uint8)
        tx[:nb] = bits
        if nb == 56:
            tx[56:] = rng.integers(0, 2, 56)
        nerr = int(rng.choice([0, 1, 1, 2, 2, 3]))
        nlow_ok = int(rng.choice([0, 1, 3, 8, 20, 30]))          # low-confidence bits that are right
        style = int(rng.integers(0, 3))      # 0: wrong bits low-confidence; 1: one wrong bit CONFIDENT; 2: a wrong bit in the DF field
        lo_pos = 0 if style == 2 else 5
        errs = rng.choice(np.arange(lo_pos, nb), nerr, replace=False) if nerr else np.array([], int)
        if style == 2 and nerr:
            errs[0] = int(rng.integers(0, 5))
        rx = tx.copy()
        rx[errs] ^= 1
        c0 = np.where(rx == 1, strong, weak).astype(f32)
        c1 = np.where(rx == 1, weak, strong).astype(f32)

        def lowconf(j):
            a, d = ref * f32(1.05), ref * f32(0.95)
            c0[j], c1[j] = (a, d) if rx[j] else (d, a)
        for k, j in enumerate(errs):
            if style == 1 and k == 0:
                continue
            lowconf(int(j))
        others = np.setdiff1d(np.arange(5, nb), errs)
        for j in rng.choice(others, min(nlow_ok, len(others)), replace=False):
            lowconf(int(j))
        bb[16::2] = c0
        bb[17::2] = c1
        meta.append((df, nerr, style, frame))
    return bursts, tags, meta


def expected_from_capture(iq, rate, max_bits, thr=7.0, pmf=True):
    """The definition applied to what the oracle's preamble scan hands the slicer for a capture."""
    spc = int(rate / 2e6)
    bursts, tags = oracle.preamble_scan(*oracle.frontend(iq, spc, pmf), spc, thr, rate)
    return slice_fix(bursts, tags, max_bits)[0]


def low_snr_capture(rate, n, seed, lam=4000.0):
    return synth.synth_capture(rate, n, lam, seed, snr_db=(4.0, 14.0))
