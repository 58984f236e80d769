"""Boundary vectors for the preamble detector (lib/preamble_impl.cc:172-216): inputs that put a sample ON the edge of every
rule -- the strict comparisons of the first stage, the ties of the peak wait and of the late-peak search, the cap of that
search, the first and last sample of both quiet zones (inclusive loops) and the samples next to them, the end-of-stream room
rule -- and a census that proves, from the inputs alone, that a case really had such samples.

The census restates the detector in plain numpy (binary32 where the reference computes in float, binary64 for the
correlation sums).  It calls no kernel and reads no kernel output.  The same vectors run on the CPU emulation
(tests/test_detector.py) and on the device (tests/test_gpu_detector.py)."""
import functools

import numpy as np

import oracle
import parity_common as pc
import synth

# (pmf, threshold) of the production cases: both filters at the default threshold everywhere, the exact thresholds 0 dB (1.0)
# and 20 dB (10.0) with one filter each; the full cross at 2 and 8 Msps
def stream_plan(rates):
    plan = [(r, p, t) for r in rates for p, t in ((True, 7.0), (False, 7.0), (True, 0.0), (False, 20.0))]
    return plan + [(r, p, t) for r in (2e6, 8e6) for p, t in ((False, 0.0), (True, 20.0))]


def case_id(v):
    return ("pmf" if v else "raw") if isinstance(v, bool) else "%g" % (v / 1e6 if v >= 1e6 else v)


f32 = np.float32
UP, DOWN = f32(np.inf), f32(-np.inf)
EDGES = ("za0", "za0-1", "za1", "za1+1", "zb0", "zb0-1", "zb1", "zb1+1")
INSIDE = ("za0", "za1", "zb0", "zb1")


class Geometry(object):
    """The block's geometry in the reference's own float arithmetic (preamble_impl.cc:56-63,150,158-162,205-208,212)."""

    def __init__(self, rate):
        spcf = f32(f32(int(rate)) / f32(2000000))
        sps = f32(spcf * f32(2))
        self.spcf, self.S, self.hist = spcf, int(spcf), int(sps) - 1
        self.o = (0, int(f32(2) * spcf), int(f32(7) * spcf), int(f32(9) * spcf))
        self.za0 = int(1.5 * float(sps))
        self.za1 = int(np.floor(f32(f32(3) * sps)))
        self.zb0 = int(f32(f32(5) * sps))
        self.zb1 = int(np.floor(7.5 * float(sps)))
        self.Bf = f32(f32(240) * spcf)
        self.B = int(f32(f32(1024) + self.Bf)) - 1024
        self.edge = {"za0": self.za0, "za0-1": self.za0 - 1, "za1": self.za1, "za1+1": self.za1 + 1,
                     "zb0": self.zb0, "zb0-1": self.zb0 - 1, "zb1": self.zb1, "zb1+1": self.zb1 + 1}
        self.zone = np.concatenate([np.arange(self.za0, self.za1 + 1), np.arange(self.zb0, self.zb1 + 1)])
        self.corr_idx = np.concatenate([c * self.S + np.arange(self.S) for c in (0, 2, 7, 9)])   # chip-major, then samples

    def ninputs(self, n):
        K = n + self.hist
        return max(K - K % self.S - self.S, 0)


def threshold_lin(thr_db):
    """powf(10., threshold_db / 20.): the quotient in double, both arguments narrowed to float (:67)."""
    return f32(np.power(f32(10.0), f32(float(thr_db) / 20.0)))


def space_threshold(peaks, av, T):
    """:198-203 in the reference's arithmetic: float sums left to right, a double division by 4.0, narrowed; then
    inavg + (avgpeak - inavg) / threshold in float."""
    s = f32(f32(f32(f32(peaks[0]) + f32(peaks[1])) + f32(peaks[2])) + f32(peaks[3]))
    avgpeak = f32(float(s) / 4.0)
    return f32(f32(av) + f32(f32(avgpeak - f32(av)) / f32(T)))


def boundary_census(bb, avg, spc, thr_db, rate, greedy=True, ranges=None):
    """Counters of the samples that sit on a rule's edge, for the candidates of the reference's scan over (bb, avg) taken
    as ONE work() call (greedy=False: for every position that passes the first stage, each refined on its own, as the
    candidate records of the production path are).  Keys:
      first_eq        in[i] == pulse_threshold, both non-zero, at a position the scan tests
      first_eq_zero   ... both zero (constant-input plateaus)
      peak_tie        in[i+1] == in[i] at a candidate
      pulse_eq        [pulse 1, 2, 3] exactly equal to pulse_threshold at a candidate
      late_tie        searches in which late_corr == now_corr exactly
      how_late        histogram over 0..spc;  rising_at_cap: searches the cap stopped while the correlation still rose
      sole            {edge: 32 counters by e % 32}: candidates whose only sample above space_threshold, inside the zones
                      and on the four samples next to them, is the one at that edge.  For the four outside edges (no part
                      of a zone) that means: nothing inside the zones is above, and the outside sample is.
      below           {edge: 32 counters}: valid candidates whose sample at that edge is the largest of its zone (of the
                      outside edge and the zone next to it) and not above space_threshold: one step from deciding
      zone_eq         zone samples exactly equal to space_threshold
      room            valid candidates at ninputs - i == 240 spc - 1, 240 spc, 240 spc + 1
      hits            item counts of the preambles the scan emits (greedy only);  cands: the candidate records
    e counts stream samples (item count minus the block's history).  ranges (with greedy=False): only the candidates whose
    first-stage position lies in one of these [lo, hi) stretches of stream samples."""
    g = Geometry(rate)
    assert g.S == spc
    n = len(bb)
    K = n + g.hist
    pad = 260 * (g.S + 1)
    x = np.zeros(K + pad, f32)
    av = np.zeros(K + pad, f32)
    x[g.hist:K] = bb
    av[g.hist:K] = avg
    x64 = x.astype(np.float64)
    T = threshold_lin(thr_db)
    nin = g.ninputs(n)
    with np.errstate(all="ignore"):
        thr = (av * T).astype(f32)
        first = x[:nin] > thr[:nin]
        cand = first & ~(x[1:nin + 1] > x[:nin])
        for o in g.o[1:]:
            cand &= ~(x[o:nin + o] < thr[:nin])
    eq = x[:nin] == thr[:nin]
    tested = np.zeros(nin, bool)
    if ranges is not None:
        assert not greedy
        keep = np.zeros(nin + 1, np.int32)
        for lo, hi in ranges:
            keep[min(lo + g.hist, nin)] += 1
            keep[min(hi + g.hist, nin)] -= 1
        cand &= np.cumsum(keep)[:nin] > 0
    cpos = np.flatnonzero(cand)
    c = dict(first_eq=0, first_eq_zero=0, peak_tie=0, pulse_eq=[0, 0, 0], late_tie=0, how_late=[0] * (spc + 1),
             rising_at_cap=0, sole={e: [0] * 32 for e in EDGES}, below={e: [0] * 32 for e in EDGES}, zone_eq=0,
             room=[0, 0, 0], hits=[], cands=[], ncand=0)
    inside = {e: g.edge[e] for e in INSIDE}
    near = {"za0-1": "za0", "za1+1": "za1", "zb0-1": "zb0", "zb1+1": "zb1"}
    zone_a = np.arange(g.za0, g.za1 + 1)
    zone_b = np.arange(g.zb0, g.zb1 + 1)
    room240 = 240 * spc

    def corr(k):
        return np.cumsum(x64[k + g.corr_idx])[-1]          # (sequential double accumulation, :91-98)

    k_from = 0
    ci = 0
    while True:
        ci = np.searchsorted(cpos, k_from) if greedy else ci
        if ci >= len(cpos):
            tested[k_from:] = greedy
            break
        k0 = int(cpos[ci])
        if greedy:
            tested[k_from:k0 + 1] = True
        c["ncand"] += 1
        if x[k0 + 1] == x[k0]:
            c["peak_tie"] += 1
        for m, o in enumerate(g.o[1:]):
            if x[k0 + o] == thr[k0] and thr[k0] != 0:
                c["pulse_eq"][m] += 1
        k, how_late, tie = k0, 0, False
        while True:
            now, nxt = corr(k), corr(k + 1)
            tie |= bool(nxt == now)
            late = bool(nxt > now)
            if late:
                k += 1
                how_late += 1
            if not (late and f32(how_late) < g.spcf):
                break
        if late and corr(k + 1) > corr(k):
            c["rising_at_cap"] += 1
        c["late_tie"] += int(tie)
        c["how_late"][min(how_late, spc)] += 1
        with np.errstate(all="ignore"):
            st = space_threshold([x[k + o] for o in g.o], av[k], T)
            za, zb = x[k + zone_a], x[k + zone_b]
            above = set(int(j) for j in g.zone[np.concatenate([za, zb]) > st])
            c["zone_eq"] += int(np.count_nonzero(za == st) + np.count_nonzero(zb == st))
        valid = not above
        e = k - g.hist
        for name, j in inside.items():
            if above == {j}:
                c["sole"][name][e % 32] += 1
            if valid and x[k + j] == (za if name[1] == "a" else zb).max():
                c["below"][name][e % 32] += 1
        for name, i_ in near.items():
            j = g.edge[name]
            if valid and x[k + j] > st:
                c["sole"][name][e % 32] += 1
            zmax = (za if name[1] == "a" else zb).max()
            if valid and not (x[k + j] > st) and x[k + j] >= zmax:
                c["below"][name][e % 32] += 1
        c["cands"].append((k0, k, how_late, float(st), valid))
        if valid and nin - k in (room240 - 1, room240, room240 + 1):
            c["room"][nin - k - room240 + 1] += 1
        if not greedy:
            ci += 1
            continue
        if not valid:
            k_from = k + 1
            continue
        if k >= nin or f32(nin - k) < g.Bf:
            break
        c["hits"].append(k)
        k_from = k + g.B
    if not greedy:
        tested[:] = True
    nz = tested & eq
    c["first_eq"] = int(np.count_nonzero(nz & (thr[:nin] != 0)))
    c["first_eq_zero"] = int(np.count_nonzero(nz & (thr[:nin] == 0)))
    return c


def census_line(name, c):
    """One printed line per case: the tests print it before they compare anything."""
    sole = " ".join("%s:%d/%d" % (e, sum(c["sole"][e]), sum(1 for v in c["sole"][e] if v)) for e in EDGES)
    below = " ".join("%s:%d" % (e, sum(c["below"][e])) for e in EDGES)
    return ("census %s: cand %d hits %d first_eq %d first_eq_zero %d peak_tie %d pulse_eq %s late_tie %d how_late %s "
            "rising_at_cap %d zone_eq %d room %s sole(n/residues of 32) %s below %s" % (
                name, c["ncand"], len(c["hits"]), c["first_eq"], c["first_eq_zero"], c["peak_tie"], c["pulse_eq"],
                c["late_tie"], c["how_late"], c["rising_at_cap"], c["zone_eq"], c["room"], sole, below))


def residues4(counters32):
    return [sum(counters32[r::4]) for r in range(4)]


# ---- block level: bb and avg are independent inputs, every value can be placed exactly ---------------------------------
class _Layout(object):
    def __init__(self, rate, thr_db, rng):
        self.g = Geometry(rate)
        self.spc = self.g.S
        self.T = threshold_lin(thr_db)
        self.rng = rng
        self.bb, self.avg = [], []
        self.at = 0

    def template(self, residue=None, pre=0, mod=32, rising=False, wide=0, top=None):
        """One clean preamble + burst on a flat floor; returns (start, A, thr, st, P[4], view of bb from start on) -- start
        is the stream index of the first sample of pulse 0, start % mod = residue.
        pre <= spc: pulses 1, 2, 3 get `pre` samples at exactly the pulse threshold in front of them and pulse 0 starts
        `pre` samples early: the first stage fires `pre` samples early and the late-peak search takes `pre` steps.
        rising: pulse 0 starts spc + 1 samples early, the chips in front of pulses 1 and 3 hold ramps that end above
        pulse 0 / pulse 2 and below pulse 1 / pulse 3, and a ramp from the pulse threshold leads to pulse 2: the
        correlation grows with every one of spc + 1 steps, the cap stops the search after spc of them.
        wide: all four pulses start `wide` samples early: late_corr == now_corr exactly, the search must not move."""
        spc, rng, T = self.spc, self.rng, self.T
        lead = 24 * spc + 8
        start = self.at + lead
        if residue is not None:
            start += (residue - start) % mod
        A = f32(int(rng.integers(1, 9)) * 2.0 ** int(rng.integers(-3, 4)))
        thr = f32(A * T)
        F = f32(A * f32(0.5))
        P = (thr * rng.uniform(3.0, 6.0, 4)).astype(f32)
        if rising:
            P = (P[0] * np.array([1.0, 1.5, 1.0, 1.5])).astype(f32)
        if top is not None:                                  # pulse `top` is the largest: above space_threshold at any threshold
            P[top] = f32(P.max() * f32(1.25))
        st = space_threshold(P, A, T)
        # (a short frame, and floor behind it for as long as a burst is: a hit inside the data -- 0 dB makes them easy --
        # must not carry the scan over the next template)
        chips = synth.frame_chips(synth.make_frame(rng, 11))
        n = start + (chips.size + 240 + 8) * spc - self.at
        bb = np.full(n, F, f32)
        s = start - self.at
        lvl = (thr * rng.uniform(3.0, 6.0, chips.size)).astype(f32)
        body = np.repeat(np.where(chips > 0, lvl, F).astype(f32), spc)
        bb[s + 16 * spc:s + chips.size * spc] = body[16 * spc:]
        for m, ch in enumerate((0, 2, 7, 9)):
            bb[s + ch * spc:s + (ch + 1) * spc] = P[m]
        if rising:
            bb[s - spc - 1:s] = P[0]
            for ch in (1, 8):
                bb[s + ch * spc:s + (ch + 1) * spc] = (P[0] * np.linspace(1.05, 1.3, spc)).astype(f32) if spc > 1 else f32(P[0] * f32(1.3))
            bb[s + 6 * spc - 1:s + 7 * spc] = (thr + (f32(0.9) * P[2] - thr) * np.linspace(0.0, 1.0, spc + 1)).astype(f32)
        elif wide:
            for m, ch in enumerate((0, 2, 7, 9)):
                bb[s + ch * spc - wide:s + ch * spc] = P[m]
        elif pre:
            assert pre <= spc
            for m, ch in enumerate((0, 2, 7, 9)):
                w = bb[s + ch * spc - pre:s + ch * spc]
                w[:] = np.maximum(w, P[0] if m == 0 else thr)
        self.bb.append(bb)
        self.avg.append(np.full(n, A, f32))
        self.at += n
        return start, A, thr, st, P, bb[s:]

    def arrays(self, tail=0):
        bb = np.concatenate(self.bb + [np.zeros(tail, f32)])
        avg = np.concatenate(self.avg + [np.zeros(tail, f32)])
        return bb, avg


def _three(v):
    return (v, np.nextafter(v, UP), np.nextafter(v, DOWN))


def detector_vectors(rate, seed, thr_db=7.0):
    """Block-level inputs for am_preamble_work / oracle.preamble_scan: (bb, avg, rooms).  Clean preamble + burst templates
    on a flat floor, start positions stepped through all residues of 32, one perturbation each:
      * a sample at one of the eight quiet-zone edges set to space_threshold exactly -- formed in the reference's own
        arithmetic -- or one float above or below it (above: at every residue of 32; equal, below: at every residue of 4);
      * pulse 0 (the first-stage test) and the first sample of pulses 1, 2, 3 at pulse_threshold and one float either side;
      * in[i+1] one float above / below in[i] (equal is what a flat pulse top is);
      * pulses with 0..spc samples at exactly pulse_threshold in front (how_late takes every value), ramps over spc + 1
        samples (the cap stops a search that still rises), and pulses widened in front (late_corr == now_corr exactly).
    rooms: three short streams [(bb, avg, d)] whose last template starts at ninputs - i == 240 spc + d, d = -1, 0, 1."""
    rng = np.random.default_rng(seed)
    L = _Layout(rate, thr_db, rng)
    g, spc = L.g, L.spc
    for name in EDGES:
        j = g.edge[name]
        # (at one sample per chip three of the outside edges ARE pulses 1, 2 and 3: nothing to place, the pulse is made the
        # largest of the four so that it is above space_threshold at 0 dB too)
        natural = g.o.index(j) if (spc == 1 and j in g.o) else None
        for r in range(32):
            for which in ((1, 0, 2) if r < 4 else (1,)):
                start, A, thr, st, P, v = L.template(r, top=natural)
                if natural is None:
                    v[j] = _three(st)[which]
    for which in range(3):
        for m in range(4):                                   # pulse m against pulse_threshold
            start, A, thr, st, P, v = L.template()
            if m == 0:
                v[:spc] = _three(thr)[which]
            else:
                v[g.o[m]] = _three(thr)[which]
    for which in (1, 2):                                     # the peak wait
        start, A, thr, st, P, v = L.template()
        v[1] = _three(v[0])[which]
    for h in range(spc + 1):
        L.template(pre=h)
        L.template(residue=int(rng.integers(0, 32)), pre=h)
    for r in range(4):
        L.template(residue=r + 4 * int(rng.integers(0, 8)), rising=True)
        L.template(residue=r + 4 * int(rng.integers(0, 8)), wide=1 + r % 2)
    bb, avg = L.arrays(tail=300 * spc)
    rooms = []
    for d in (-1, 0, 1):
        R = _Layout(rate, thr_db, np.random.default_rng(seed + 100 + d))
        R.template()
        # ninputs = K - K % S - S with K = n + hist (:150) is a multiple of S: so must start + hist + 240 spc + d be
        start, A, thr, st, P, v = R.template(residue=(-(g.hist + d)) % spc, mod=spc)
        rb, ra = R.arrays()
        n = next(n for n in range(start + 240 * spc, len(rb)) if g.ninputs(n) - (start + g.hist) == 240 * spc + d)
        rooms.append((rb[:n].copy(), ra[:n].copy(), d))
    return bb, avg, rooms


# ---- production path: avg is the front end's own, values are placed through integer-amplitude IQ -----------------------
_AMP = 1023
_GRID = (np.arange(_AMP + 1, dtype=np.int64)[:, None] ** 2 + np.arange(_AMP + 1, dtype=np.int64)[None, :] ** 2).ravel()
_ORDER = np.argsort(_GRID, kind="stable")
_SQ = _GRID[_ORDER]                                          # every |a + bj|^2 with integers 0 <= a, b <= 1023, sorted


def _bracket(need, above):
    """(a + bj, |.|^2): the smallest representable |.|^2 above `need`, or the largest one not above it."""
    i = int(np.searchsorted(_SQ, need, side="right"))
    i = min(i, len(_SQ) - 1) if above else max(i - 1, 0)
    a, b = divmod(int(_ORDER[i]), _AMP + 1)
    return np.complex64(complex(a, b)), int(_SQ[i])


def _weak_template(spc, smoothed, m, X, W, frame):
    """Floor 2, pulse 0 with |.|^2 = X at its first sample (behind the matched filter: at that sample only), pulse m at W."""
    chips = synth.frame_chips(frame).astype(np.complex64) * _bracket(X - 0.5, True)[0]
    body = np.repeat(chips, spc)
    out = np.full(300 * spc, np.complex64(1 + 1j))
    out[:body.size] = np.where(body != 0, body, np.complex64(1 + 1j))
    if smoothed:
        out[1:spc] = np.complex64(1 + 1j)
    o = (0, 2 * spc, 7 * spc, 9 * spc)[m] - (spc - 1 if smoothed else 0)    # (the filter's output at pulse 0's first sample looks back)
    out[o:o + spc] = _bracket(W - 0.5, True)[0]
    return out


@functools.lru_cache(maxsize=None)
def _weak_levels(spc, smoothed):
    """(X, W), both |a + bj|^2 of integers: with 48 chips of floor 2 in front, the front end's average at the first sample of a
    pulse 0 of power X is exactly W in its own float arithmetic (checked on the oracle's front end, not assumed)."""
    sq = set(int(v) for v in _SQ[:400000])
    L = 48 * spc
    for W in (int(v) for v in _SQ[3:4000]):
        # the window of the average holds L - 1 floor samples and one that carries X (behind the filter: X / spc of it)
        X = (spc * (L * W - 2 * (L - 1)) - 2 * (spc - 1)) if smoothed else (L * W - 2 * (L - 1))
        if X not in sq or X >= int(_SQ[-1]):
            continue
        iq = np.full(700 * spc, np.complex64(1 + 1j))
        iq[200 * spc:500 * spc] = _weak_template(spc, smoothed, 1, X, W, bytes(7))
        bb, avg = oracle.frontend(iq, spc, smoothed)
        k0 = 200 * spc
        if bb[k0] > avg[k0] and not bb[k0 + 1] > bb[k0] and bb[k0 + 2 * spc] == avg[k0]:
            return X, W
    raise AssertionError("no exact level found at %d samples per chip" % spc)


def _search_templates(rng, g, smoothed, thr_db):
    """Templates for the first-stage test and the late-peak search, through the front end: short frames, 312 chips apart.
      * late-peak family, h = 0 .. : pulse 0 starts h samples early and pulses 1, 2, 3 stand on a pedestal of half their power
        that starts h + spc samples early.  The first stage fires on pulse 0's flat front, every step to the right trades
        pedestal for pulse: without the matched filter how_late = min(h, spc), and h > spc leaves a search the cap stops
        while it still rises.  Behind the matched filter (`smoothed`) the same shapes are ramps and the steps come out fewer:
        h runs further, and what each template gave is for the census to say;
      * two ramp templates as in _Layout.template(rising=True), pulse 0 early by spc + 1 samples (2 spc + 2 behind the matched
        filter, whose output then rises for spc + 1 steps and more): the cap stops a search that still rises;
      * at 0 dB, where pulse_threshold is the reference level itself: pulse m = 1, 2, 3 at exactly the level the front end's
        average has at the first sample of pulse 0 (_weak_levels)."""
    spc = g.S
    period = 312 * spc
    hs = list(range(0, (2 * spc + 3) if smoothed else (spc + 3)))
    weak = []
    if thr_db == 0.0:
        XW = _weak_levels(spc, smoothed)
        weak = [(m, XW) for m in (1, 2, 3) for _ in range(2)]
    out = np.full((len(hs) + len(weak) + 4) * period, np.complex64(1 + 1j))
    at = 0
    for h in hs:
        at += period
        s = at + int(rng.integers(0, 32))
        a = int(rng.integers(50, 90))
        P, Q = np.complex64(complex(a, a // 3)), np.complex64(complex(int(0.7 * a), int(0.7 * a) // 3))
        chips = synth.frame_chips(synth.make_frame(rng, 11)).astype(np.complex64) * P
        body = np.repeat(chips, spc)
        out[s:s + body.size] = np.where(body != 0, body, np.complex64(1 + 1j))
        for c in (2, 7, 9):
            w = out[s + c * spc - h - spc:s + c * spc]
            w[np.abs(w) < np.abs(Q)] = Q
        out[s - h:s] = P
    E = (2 * spc + 2) if smoothed else (spc + 1)
    for _ in range(2):                                       # the cap stops a search that still rises (see _Layout.template)
        at += period
        s = at + 2 * spc + 2 + int(rng.integers(0, 32))
        a0 = int(rng.integers(90, 110))
        amp = lambda power: np.complex64(complex(int(round(a0 * np.sqrt(power))), 0))
        chips = synth.frame_chips(synth.make_frame(rng, 11)).astype(np.complex64) * amp(1.0)
        body = np.repeat(chips, spc)
        out[s:s + body.size] = np.where(body != 0, body, np.complex64(1 + 1j))
        for c in (2, 9):
            out[s + c * spc:s + (c + 1) * spc] = amp(1.5)
        for c in (1, 8):
            out[s + c * spc:s + (c + 1) * spc] = [amp(q) for q in np.linspace(1.05, 1.3, spc)]
        out[s + 7 * spc - E:s + 7 * spc] = [amp(q) for q in np.linspace(0.5, 0.9, E)]
        out[s - E:s] = amp(1.0)
    for m, (X, W) in weak:
        at += period
        s = at + int(rng.integers(0, 32))
        out[s:s + 300 * spc] = _weak_template(spc, smoothed, m, X, W, synth.make_frame(rng, 11))
    return out


@functools.lru_cache(maxsize=4)
def detector_streams(rate, pmf, seed, thr_db=7.0, copies=1, passes=3):
    """Integer-amplitude IQ whose templates have ONE sample, at one of the eight quiet-zone edges, bracketing the
    space_threshold the oracle's front end gives that template: the smallest |.|^2 a pair of integers can form above it
    (the sample is then the sole decider) or the largest one not above it (one step from deciding).  With pmf the IQ sample
    is chosen so that the matched filter's output moves at that one zone sample only.  The values are found from the
    oracle's front end and the census, re-run `passes` times; which templates made it is for the census to say.  Behind them
    come the templates of _search_templates: the first stage and the late-peak search.
    (Cached: the callers only read the arrays.)  Returns (iq, marks): marks = [(e, edge sample, name, above)] in stream
    samples, for the cuts of the chunked runs."""
    rng = np.random.default_rng(seed)
    g = Geometry(rate)
    spc = g.S
    period = 240 * spc + 72 * spc
    plan = []
    for name in EDGES:
        for r in range(4):
            for above in (True, False):
                for _ in range(copies):
                    plan.append((name, r, above))
    order = rng.permutation(len(plan))
    n = (len(plan) + 2) * period + 32
    iq = np.full(n, np.complex64(1 + 1j))
    starts = []
    for t, pi in enumerate(order):
        name, r, above = plan[pi]
        s = (t + 1) * period
        peak = s + (spc - 1 if pmf else 0)                   # where the matched filter's output peaks
        s += (r - peak) % 4 + 4 * int(rng.integers(0, 8))    # (e % 4 = r, e % 32 anything)
        amp = np.array([complex(int(rng.integers(40, 80)), int(rng.integers(0, 40)))] * 4)
        j = g.edge[name]
        if spc == 1 and j in g.o:                            # this edge IS pulse 1, 2 or 3: the largest of the four, so above
            amp[g.o.index(j)] += complex(24, 8)              # space_threshold at 0 dB too
        chips = synth.frame_chips(synth.make_frame(rng, 17 if t % 3 else 11)).astype(np.complex64)
        chips[16:] *= amp[0]
        chips[[0, 2, 7, 9]] = amp
        iq[s:s + chips.size * spc] = np.where(np.repeat(chips, spc) != 0, np.repeat(chips, spc), np.complex64(1 + 1j))
        starts.append((s, name, above))
    iq = np.concatenate([iq, _search_templates(rng, g, pmf and spc > 1, thr_db)])
    where = {}
    marks = []
    T = threshold_lin(thr_db)
    for it in range(passes):
        bb, avg = oracle.frontend(iq, spc, pmf)
        if it == 0:                                          # the clean templates' own positions: the first valid candidate of each
            c = boundary_census(bb, avg, spc, thr_db, rate, greedy=False, ranges=[(s, s + 2 * spc) for s, _, _ in starts])
            valid = sorted(k - g.hist for k0, k, hl, st, ok in c["cands"] if ok)
            for s, name, above in starts:
                i = int(np.searchsorted(valid, s))
                if i < len(valid) and valid[i] < s + 2 * spc:
                    where[s] = valid[i]
        marks = []
        for s, name, above in starts:
            e = where.get(s)
            if e is None:
                continue
            st = float(space_threshold([bb[e + o] for o in g.o], avg[e], T))
            j = g.edge[name]
            x = e + j
            marks.append((e, x, name, above))
            if spc == 1 and j in g.o:
                continue                                     # (a pulse: placed when the template was laid out)
            # with the matched filter one IQ sample moves spc of its outputs: the oldest sample of the window for the edges
            # at the front of a zone, the newest for those at its end -- no other sample of the zone moves
            m = x - spc + 1 if (pmf and name in ("za0-1", "za0", "zb0-1", "zb0")) else x
            cur = float(iq[m].real) ** 2 + float(iq[m].imag) ** 2
            need = cur + (st - float(bb[x])) * (spc if pmf else 1)
            iq[m] = _bracket(need, above)[0]
    iq.setflags(write=False)
    return iq, marks


# 30 000 samples per chip times this, by samples per chip: what it takes for >= 10 late-peak searches with an exact tie in every
# case (counted by the census on the oracle's front end; the searches get rarer as the rate falls)
LATTICE_MULT = {1: 6, 2: 4, 4: 6, 5: 6, 8: 4, 10: 3, 16: 2, 20: 2, 32: 1}


def lattice_capture(rate, n, lam, seed, lsb=0.03, sigma=0.01, **kw):
    """synth.synth_capture rounded to small integers (rint(x / lsb), clipped to +-127, kept as float32): |.|^2 and short
    sums of it are exact, so equal samples, equal correlation sums and samples equal to a threshold are common."""
    iq, _ = synth.synth_capture(rate, n, lam, seed, sigma=sigma, **kw)
    v = np.clip(np.rint(iq.view(f32) / f32(lsb)), -127, 127).astype(f32)
    return v.view(np.complex64)


# ---- the checks (shared by the emulated and the device file) ------------------------------------------------------------
def assert_block_census(c, spc, name):
    for e in EDGES:
        assert all(v > 0 for v in c["sole"][e]), "%s: no sole-decider template at edge %s for some e %% 32: %s" % (name, e, c["sole"][e])
    assert c["first_eq"] > 0 and c["peak_tie"] > 0 and c["zone_eq"] > 0 and all(v > 0 for v in c["pulse_eq"]), name
    assert c["late_tie"] > 0, name
    assert all(v > 0 for v in c["how_late"]) and c["rising_at_cap"] > 0, "%s: how_late %s rising %d" % (name, c["how_late"], c["rising_at_cap"])


def check_block(lib, rate, seed, thr_db):
    """detector_vectors through Context.preamble_work against the oracle's scan and the reference's C++."""
    from air_modes import _capi
    spc = int(rate / 2e6)
    bb, avg, rooms = detector_vectors(rate, seed, thr_db)
    assert float(threshold_lin(thr_db)) == oracle.threshold_lin(thr_db)
    c = boundary_census(bb, avg, spc, thr_db, rate)
    name = "block %g Msps %g dB" % (rate / 1e6, thr_db)
    print(census_line(name, c))
    assert_block_census(c, spc, name)
    room = [0, 0, 0]
    ctx = _capi.Context(rate, thr_db, True, lib=lib)
    total = 0
    for b_, a_, d in [(bb, avg, None)] + rooms:
        cc = c if d is None else boundary_census(b_, a_, spc, thr_db, rate)
        if d is not None:
            room = [x + y for x, y in zip(room, cc["room"])]
        ob, ot = oracle.preamble_scan(b_, a_, spc, thr_db, rate)
        assert [int(s) for s in ot["sample"]] == cc["hits"], "the census and the oracle disagree about the hits"
        bursts, tags = ctx.preamble_work(b_, a_)
        assert len(tags) == len(ot), "tag count differs: %d vs %d (room %s)" % (len(tags), len(ot), d)
        assert np.ascontiguousarray(tags).tobytes() == np.ascontiguousarray(ot).tobytes(), "tags differ (room %s)" % d
        assert np.array_equal(pc.u32(bursts), pc.u32(ob)), "bursts differ"
        if oracle.have_ref():
            rb, rt, _, keep = oracle.ref_preamble_slicer(b_, a_, spc, thr_db, rate)
            rb, rt = rb[keep], rt[keep]
            assert np.array_equal(tags["sample"], rt["sample"]) and np.array_equal(pc.u32(bursts), pc.u32(rb)), "differs from the reference's C++"
        total += len(tags)
    ctx.close()
    print("census %s room %s" % (name, room))
    assert all(v > 0 for v in room), "room rule: %s" % room
    return total


def assert_stream_census(c, name, rate, thr_db):
    """What every production case must hold before it is compared: the eight quiet-zone edges, and the classes of the first
    stage and of the late-peak search that the kernels in front of the refinement decide."""
    g = Geometry(rate)
    for e in EDGES:
        s4 = residues4(c["sole"][e])
        assert all(v > 0 for v in s4), "%s: edge %s has e %% 4 residues without a confirmed sole decider: %s" % (name, e, s4)
        if g.S == 1 and g.edge[e] in g.o:
            continue                                         # (the edge is a pulse: it has no value below the threshold)
        assert sum(c["below"][e]) > 0, "%s: no template one step below at edge %s" % (name, e)
    assert all(v > 0 for v in c["how_late"]), "%s: how_late %s" % (name, c["how_late"])
    assert c["rising_at_cap"] > 0, "%s: the cap never stopped a search that still rose" % name
    assert c["late_tie"] > 0 and c["peak_tie"] > 0, "%s: late ties %d, peak ties %d" % (name, c["late_tie"], c["peak_tie"])
    if thr_db == 0.0:
        # (an exact linear threshold: 1.0.  At 7 dB it is irrational, and at 20 dB -- 10.0 -- ten times the front end's average of
        # integer samples is no value such a sample takes here: equality with non-zero operands needs 0 dB)
        assert c["first_eq"] > 0 and all(v > 0 for v in c["pulse_eq"]), "%s: first_eq %d pulse_eq %s" % (name, c["first_eq"], c["pulse_eq"])


def stream_cuts(marks, n, spc):
    """Cuts inside perturbed templates: at e, at the edge sample and one sample after it."""
    cuts = set()
    for e, x, name, above in marks[::19]:               # (a few templates, different edges: every cut is a call)
        cuts.update((e, x, x + 1))
    return sorted(k for k in cuts if 300 * spc < k < n - 300 * spc)


def check_streams(lib, rate, pmf, seed, thr_db, want_fe=None):
    """detector_streams through the production path: every candidate record, the tags and bursts, chunked, sharded."""
    spc = int(rate / 2e6)
    iq, marks = detector_streams(rate, pmf, seed, thr_db)
    bb, avg = oracle.frontend(iq, spc, pmf)
    c = boundary_census(bb, avg, spc, thr_db, rate, greedy=False)
    name = "stream %g Msps pmf=%d %g dB" % (rate / 1e6, pmf, thr_db)
    print(census_line(name, c))
    assert_stream_census(c, name, rate, thr_db)
    # (64 Msps: the streaming front end, so that am_k_refine_seg is what ran -- unless the caller steers elsewhere)
    npk = pc.check_production_stages(lib, rate, len(iq), 0.0, seed, thr=thr_db, pmf=pmf, iq=iq, with_ref=True,
                                     want_fe=want_fe or (3 if rate == 64e6 else None))
    want = oracle.demod(iq, rate, thr_db, pmf)
    cuts = stream_cuts(marks, len(iq), spc)
    assert len(cuts) >= 9
    pc.check_chunked(lib, rate, iq, cuts, thr=thr_db, pmf=pmf, want=want)
    pc.check_sharded(lib, rate, iq, 3, thr=thr_db, pmf=pmf, want=want)
    return npk, iq


def check_lattice(lib, rate, pmf, lam=6000.0, seed=77, thr_db=7.0, lsb=0.05, sigma=0.01, ties=10, want_fe=None):
    """Weak bursts (8 .. 20 dB: amplitudes of one to three steps) on the integer lattice: exact ties of the late-peak search and of
    the peak wait in searches that really happen -- at least `ties` of each, or the case proves nothing."""
    spc = int(rate / 2e6)
    n = 30000 * spc * LATTICE_MULT[spc]
    iq = lattice_capture(rate, n, lam, seed, lsb, sigma, snr_db=(8.0, 20.0))
    bb, avg = oracle.frontend(iq, spc, pmf)
    c = boundary_census(bb, avg, spc, thr_db, rate, greedy=False)
    name = "lattice %g Msps pmf=%d" % (rate / 1e6, pmf)
    print(census_line(name, c))
    assert c["late_tie"] >= ties and c["peak_tie"] >= ties, "%s: late ties %d, peak ties %d" % (name, c["late_tie"], c["peak_tie"])
    npk = pc.check_production_stages(lib, rate, n, lam, seed, thr=thr_db, pmf=pmf, iq=iq, with_ref=True,
                                     want_fe=want_fe or (3 if rate == 64e6 else None))
    want = oracle.demod(iq, rate, thr_db, pmf)
    pc.check_chunked(lib, rate, iq, [n // 3 + 1, n // 2, n // 2 + 7 * spc + 1], thr=thr_db, pmf=pmf, want=want)
    pc.check_sharded(lib, rate, iq, 3, thr=thr_db, pmf=pmf, want=want)
    return npk


def check_plateaus(lib, rate, n, lam=6000.0, seed=78):
    """Noiseless integer bursts: long constant stretches, 0 == 0 at the first stage all over."""
    spc = int(rate / 2e6)
    full, _ = synth.synth_capture(rate, n, lam, seed, cfo_hz=0.0)
    noise, _ = synth.synth_capture(rate, n, 0.0, seed, cfo_hz=0.0)          # (the same seed draws the same noise first)
    v = np.clip(np.rint((full - noise).view(f32) / f32(0.03)), -127, 127).astype(f32)
    iq = v.view(np.complex64)
    bb, avg = oracle.frontend(iq, spc, True)
    c = boundary_census(bb, avg, spc, 7.0, rate)
    print(census_line("plateaus %g Msps" % (rate / 1e6), c))
    assert c["first_eq_zero"] >= 1000
    return pc.check_production_stages(lib, rate, n, lam, seed, iq=iq, with_ref=True, want_fe=3 if rate == 64e6 else None)


def check_lattice_cuts(lib, rate, n, lam=6000.0, seed=79, dcblock=False):
    """Lattice captures where the oracle's scan is the only witness (fractional samples per chip, the DC blocker in front):
    cut into calls and time-sharded against oracle.demod."""
    iq = lattice_capture(rate, n, lam, seed)
    want = oracle.demod(iq, rate, 7.0, True, use_dcblock=dcblock)
    spc = max(int(rate / 2e6), 1)
    pc.check_chunked(lib, rate, iq, [n // 5, n // 3 + 1, n // 2, n // 2 + 7 * spc + 1], want=want, dcblock=dcblock)
    pc.check_sharded(lib, rate, iq, 3, want=want, dcblock=dcblock)
    return len(want)
