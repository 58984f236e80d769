"""The opt-in 112-bit slicing and parity check of DF18 / DF19 squitters (am_set_long_formats) restated in numpy, composed with
the repair (tests/fix_common.py) and the address gate (tests/gate_common.py), and the bursts and captures the tests feed it.

DEFINITION.  mask = OR of 1 (DF18) and 2 (DF19); E = the enabled formats; hdr = the five header bits as sliced
(lib/slicer_impl.cc:135-139).
  length:  long iff hdr in {16, 17, 20, 21} | E.  :142-171 run with that length: 112 decisions, the low-confidence count over 112
           bits, and :170 (short packets only) does not apply to a format in E.
  parity:  (:182) dropped if the syndrome is non-zero and DF in {11, 17} | E.
  repair:  (fix_common's definition) a format in E is treated as DF17 is: one bit, two bits at max_bits = 2, candidates 5..111.
  gate:    (gate_common's definition) a kept packet of a format in E takes no part: kept in mode 1 and 2, teaches nothing, is
           not tested.  A format not in E stays with the "others".
  packet:  nbytes = 14, df = 18 or 19, crc = 0, reserved[1] as for DF17.
mask = 0 is fix_common.slice_fix, which with max_bits = 0 is oracle.slice_bursts (tests/test_long_formats.py proves both first).

Nothing here looks at the library."""
import numpy as np

import fix_common as fx
import gate_common as gc
import oracle
import synth

PK = oracle.PACKET_DTYPE
f32 = np.float32
LF_DF18, LF_DF19 = 1, 2
REF_LONG = (16, 17, 20, 21)                              # slicer_impl.cc:140
# the formats of the constructed bursts: the two squitters, what they are treated as, the reference's other long format, a
# short address/parity reply, and a format long on the air that stays short whatever the mask
BURST_DFS = (17, 11, 18, 19, 16, 0, 24)
# synth.DF_MIX_EDGE's formats with most of the weight on the two squitters
MIX = ((17, 0.10), (11, 0.05), (16, 0.05), (18, 0.40), (19, 0.20), (24, 0.05), (0, 0.05), (20, 0.05), (21, 0.05))


def enabled(mask):
    return tuple(df for df, bit in ((18, LF_DF18), (19, LF_DF19)) if mask & bit)


def frame(rng, df):
    """synth.make_frame, except that DF18 / DF19 carry a clean PI (the address overlay make_frame puts on them is taken off
    again): draws from rng exactly what make_frame draws, so a capture made with it differs from make_frame's in those frames
    only."""
    fr = synth.make_frame(rng, df)
    if df in (18, 19):
        fr = fr[:-3] + synth._crc24(fr[:-3]).to_bytes(3, "big")
    return fr


def slice_raw(bursts, mask):
    """:128-177 with the definition's length for every burst: dict of ref, dec[n, 112] (zero beyond the length), nlow, nbits,
    hdr, synd."""
    ref, dec, low, _ = fx.slice_all(bursts)
    hdr = np.zeros(len(ref), np.int64)
    for j in range(5):
        hdr = (hdr << 1) | dec[:, j]
    long_ = np.isin(hdr, REF_LONG + enabled(mask))
    dec = dec.copy()
    low = low.copy()
    dec[~long_, 56:] = 0
    low[~long_, 56:] = False
    table = np.zeros((len(ref), 112), np.int64)
    table[long_] = fx.SYN[112]
    table[~long_, :56] = fx.SYN[56]
    synd = np.bitwise_xor.reduce(np.where(dec == 1, table, 0), axis=1)
    return dict(ref=ref, dec=dec, nlow=np.minimum(low.sum(axis=1), 24), nbits=np.where(long_, 112, 56), hdr=hdr, synd=synd)


def slice_long(bursts, tags, max_bits, mask):
    """The definition: (packets, index of each packet's burst)."""
    r = slice_raw(bursts, mask)
    dec, nlow, nbits, mt, synd = r["dec"], r["nlow"], r["nbits"], r["hdr"], r["synd"].copy()
    long_ = nbits == 112
    as17 = np.isin(mt, (17,) + enabled(mask))
    ok = dec.any(axis=1)                                                                           # :162-166
    ok &= ~(~long_ & (mt != 11) & (nlow > 0))                                                      # :170
    ok &= ~((mt == 11) & (nlow >= 10))                                                             # :171
    bad = ok & (synd != 0) & ((mt == 11) | as17)                                                   # :182
    fixed = np.zeros(len(mt), np.uint8)
    for i in np.nonzero(bad)[0]:
        sol = fx.find_repair(int(nbits[i]), int(synd[i]), max_bits >= 2 and bool(as17[i])) if max_bits >= 1 else ()
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
    out["ref"] = r["ref"][idx]
    for k in ("sample", "secs", "frac"):
        out[k] = tags[k][idx]
    return out, idx


def gate(pk, mode, ttl, mask):
    """gate_common.gate over the packets that take part; a packet of an enabled format is kept and is invisible to it."""
    apart = np.isin(pk["df"], enabled(mask))
    keep = np.ones(len(pk), bool)
    keep[~apart] = gc.gate(pk[~apart], mode, ttl)
    return keep


def counts(pk):
    """(clean DF18, clean DF19, repaired DF18, repaired DF19) among 112-bit packets."""
    l, r = pk["nbytes"] == 14, pk["reserved"][:, 1]
    return tuple(int(np.count_nonzero(l & (pk["df"] == df) & ((r > 0) == rep))) for rep in (False, True) for df in (18, 19))


def long_bursts(n, seed):
    """fix_common.damaged_bursts with the format drawn from BURST_DFS (DF18 / DF19 with a clean PI): 0-3 wrong bits, low-confidence
    or confidently wrong or in the DF field, 0-30 further low-confidence bits that are right, levels over four decades.  Every
    chip is finite and no bit's two chips are equal.  -> (bursts, tags, meta[(df, wrong bits, style, transmitted frame)])."""
    rng = np.random.default_rng(seed)
    bursts = np.zeros((n, 240), f32)
    tags = np.zeros(n, oracle.TAG_DTYPE)
    tags["sample"] = np.arange(n, dtype=np.uint64) * 4801 + 7
    tags["secs"] = rng.integers(0, 1 << 33, n)
    tags["frac"] = rng.random(n)
    meta = []
    for i in range(n):
        df = int(rng.choice(BURST_DFS, p=(0.15, 0.1, 0.3, 0.25, 0.08, 0.06, 0.06)))
        fr = frame(rng, df)
        bits = np.unpackbits(np.frombuffer(fr, np.uint8))
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
        nerr = int(rng.choice([0, 0, 1, 1, 2, 2, 3]))
        nlow_ok = int(rng.choice([0, 1, 3, 8, 20, 30]))
        style = int(rng.integers(0, 3))      # 0: wrong bits low-confidence; 1: one wrong bit CONFIDENT; 2: a wrong bit in the DF field
        errs = rng.choice(np.arange(0 if style == 2 else 5, nb), nerr, replace=False) if nerr else np.array([], int)
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
            if not (style == 1 and k == 0):
                lowconf(int(j))
        others = np.setdiff1d(np.arange(5, nb), errs)
        for j in rng.choice(others, min(nlow_ok, len(others)), replace=False):
            lowconf(int(j))
        bb[16::2] = c0
        bb[17::2] = c1
        meta.append((df, nerr, style, fr))
    assert np.isfinite(bursts).all() and (bursts[:, 16::2] != bursts[:, 17::2]).all()
    return bursts, tags, meta


def as_df16(bursts, hdr):
    """Every burst with the chips of header bit 3 exchanged, and of bit 4 too where hdr is 19: 18 = 10010 and 19 = 10011 both
    read 10000 = 16 then (slicer_impl.cc:74-98: for finite, unequal chips the decision flips and the confidence stays), which
    the reference slices as 112 bits with no parity test.  -> (bursts, flipped bit positions per burst)."""
    out = np.array(bursts, f32)
    flipped = []
    for i, h in enumerate(hdr):
        js = (3, 4) if h == 19 else (3,)
        for j in js:
            out[i, 16 + 2 * j], out[i, 17 + 2 * j] = bursts[i, 17 + 2 * j], bursts[i, 16 + 2 * j]
        flipped.append(js)
    return out, flipped


def capture(rate, n, lam, seed, snr_db=(6.0, 14.0), mix=MIX):
    """A seeded capture of the edge formats with clean-PI DF18 / DF19 frames, at low SNR (wrong bits of every kind)."""
    return synth.synth_capture(rate, n, lam, seed, snr_db=snr_db, df_mix=mix, frame_fn=frame)


def add_burst(iq, rate, start, fr, amp=0.5):
    """The capture with frame fr on top of it from sample `start` on (whole samples per chip, no carrier offset)."""
    out = np.array(iq, np.complex64)
    env = np.repeat(synth.frame_chips(fr), int(round(rate / 2e6)))
    out[start:start + env.size] += (amp * env).astype(np.complex64)
    return out


def scan(iq, rate, thr=7.0, pmf=True):
    """What the oracle's preamble scan hands the slicer for a capture: (bursts, tags).  It does not depend on the mask."""
    spc = int(rate / 2e6)
    return oracle.preamble_scan(*oracle.frontend(iq, spc, pmf), spc, thr, rate)


def expected(scanned, max_bits, mask, gate_mode=0, ttl=1):
    bursts, tags = scanned
    pk = slice_long(bursts, tags, max_bits, mask)[0]
    return pk[gate(pk, gate_mode, ttl, mask)] if gate_mode else pk
