"""The opt-in address gate (am_set_address_gate) restated in numpy, and the captures the tests feed it.

DEFINITION.  The packets of a stream are formed exactly as without the gate (the oracle's, or tests/fix_common.py's when the
repair is on).  Then, in stream order, with a map last[address] -> item count that is empty at the start of the stream, for a
packet p at item count s = p.sample:
  1. teach:  p.df is 11 or 17, p.crc == 0 and p.reserved[1] == 0 (as sliced, not repaired): last[data[1..3], big-endian] = s.
             The packet is kept (and so is a DF11 / DF17 packet that does not teach -- a repaired one).
  2. test:   p.df in {0, 4, 5, 16, 20, 21}: kept iff last[p.crc] exists and s - last[p.crc] <= ttl_samples.  A kept
             address/parity packet does not teach.
  3. others: mode 1 keeps them, mode 2 drops them.
ttl_samples = max(1, int(ttl_seconds * rate)).  mode 0 keeps everything.

Nothing here looks at the library.  tools/synth.py overlays a RANDOM address on every address/parity frame, so none of its frames
would ever pass: fleet_capture draws a fleet of addresses, puts the address into bytes 1-3 of its DF11 / DF17 frames (clean
parity) and overlays the same address on the parity of its DF0/4/5/20/21 frames."""
import numpy as np

import oracle
import synth

AP = (0, 4, 5, 16, 20, 21)
MIX = ((17, 0.40), (11, 0.10), (0, 0.10), (4, 0.10), (5, 0.10), (20, 0.10), (21, 0.10))


def ttl_samples(ttl_seconds, rate):
    return max(1, int(ttl_seconds * rate))


def fleet_frame(rng, df, addr):
    long_ = df in (16, 17, 20, 21)
    nb = 14 if long_ else 7
    body = bytearray(rng.integers(0, 256, nb - 3, dtype=np.uint8).tobytes())
    body[0] = ((df & 31) << 3) | (body[0] & 7)
    if df in (11, 17):
        body[1:4] = addr.to_bytes(3, "big")
    par = synth._crc24(bytes(body))
    if df not in (11, 17):
        par ^= addr
    return bytes(body) + par.to_bytes(3, "big")


def fleet_capture(rate, n, lam, seed, naddr, snr=(10.0, 35.0), sigma=0.01, fleet=None, mix=MIX):
    """Burst placement as synth.synth_capture.  Returns (iq, truth, fleet); truth: (start, frame hex, address, df) per burst.
    fleet: use these addresses instead of drawing naddr (the draw is still made, so the rest of the capture does not move)."""
    rng = np.random.default_rng(np.random.PCG64(seed))
    spc = int(round(rate / 2e6))
    spcf = rate / 2e6
    whole = abs(rate - 2e6 * spc) < 1e-6                     # whole samples per chip: the generator the pinned counts come from
    iq = (rng.standard_normal(2 * n, dtype=np.float32) * np.float32(sigma)).view(np.complex64)
    drawn = [int(a) for a in rng.choice(np.arange(1, 1 << 24), naddr, replace=False)]
    fleet = drawn if fleet is None else list(fleet)
    nb = int(rng.poisson(lam * n / rate))
    starts = np.sort(rng.uniform(0, n - 1, nb))
    dfs = np.array([d for d, _ in mix])
    pr = np.array([p for _, p in mix])
    pr = pr / pr.sum()
    truth = []
    for t0 in starts:
        df = int(rng.choice(dfs, p=pr))
        addr = fleet[int(rng.integers(0, naddr)) % len(fleet)]
        fr_ = fleet_frame(rng, df, addr)
        s = float(rng.uniform(*snr))
        amp = np.sqrt(2.0) * sigma * 10 ** (s / 20)
        ph = float(rng.uniform(0, 2 * np.pi))
        cfo = float(rng.uniform(-50e3, 50e3))
        i0 = int(np.floor(t0))
        fr = t0 - i0
        if whole:
            env = np.repeat(synth.frame_chips(fr_), spc)
            env = np.concatenate([env, [0.0]]) * (1 - fr) + np.concatenate([[0.0], env]) * fr
        else:
            # a rate that is not a multiple of 2 MHz (5 Msps: 2.5 samples per chip): the chips are area-sampled, as
            # synth.synth_capture does -- sample m is the mean of the chip waveform over [(m - fr) / spcf, (m + 1 - fr) / spcf)
            chips = synth.frame_chips(fr_).astype(np.float64)
            cum = np.concatenate([[0.0], np.cumsum(chips)])
            m = np.arange(int(np.ceil(chips.size * spcf)) + 2, dtype=np.float64)

            def integral(x):
                x = np.clip(x, 0.0, float(chips.size))
                q = np.minimum(x.astype(np.int64), chips.size - 1)
                return cum[q] + chips[q] * (x - q)
            env = (integral((m + 1.0 - fr) / spcf) - integral((m - fr) / spcf)) * spcf
        i1 = min(i0 + env.size, n)
        k = np.arange(i0, i1)
        iq[i0:i1] += (amp * env[:i1 - i0] * np.exp(1j * (2 * np.pi * cfo * (k - i0) / rate + ph))).astype(np.complex64)
        truth.append((t0, fr_.hex(), addr, df))
    return iq, truth, fleet


def gate(pk, mode, ttl):
    """The definition: keep mask over the packets of ONE stream, in stream order.  ttl in item counts."""
    last = {}
    keep = np.ones(len(pk), bool)
    if mode == 0:
        return keep
    for i, p in enumerate(pk):
        df = int(p["df"])
        s = int(p["sample"])
        if df in (11, 17):
            if p["crc"] == 0 and p["reserved"][1] == 0:
                last[(int(p["data"][1]) << 16) | (int(p["data"][2]) << 8) | int(p["data"][3])] = s
        elif df in AP:
            l = last.get(int(p["crc"]))
            keep[i] = l is not None and s - l <= ttl
        elif mode == 2:
            keep[i] = False
    return keep


def counts(pk, keep):
    """What am_get_address_gate_stats adds for this stream: (taught, passed, dropped)."""
    teach = np.isin(pk["df"], (11, 17)) & (pk["crc"] == 0) & (pk["reserved"][:, 1] == 0)
    return int(teach.sum()), int((np.isin(pk["df"], AP) & keep).sum()), int((~keep).sum())


def transmitted(pk, truth):
    """Per packet: is it one of the frames the generator put on the air?"""
    frames = set(t[1] for t in truth)
    return np.array([bytes(p["data"][:p["nbytes"]]).hex() in frames for p in pk], bool)


def is_subsequence(sub, full):
    """Are the packets `sub` (structured array) a subsequence of `full`, byte for byte?"""
    j = 0
    for p in sub:
        while j < len(full) and full[j].tobytes() != p.tobytes():
            j += 1
        if j == len(full):
            return False
        j += 1
    return True


def brute_force_ok(pk, keep, ttl):
    """Independently of the dict loop, O(n^2): a test packet is kept iff the LATEST teach of its address in front of it is at
    most ttl item counts old."""
    for i, p in enumerate(pk):
        if int(p["df"]) not in AP:
            continue
        want = False
        for q in pk[:i][::-1]:
            if int(q["df"]) in (11, 17) and q["crc"] == 0 and q["reserved"][1] == 0 and \
                    ((int(q["data"][1]) << 16) | (int(q["data"][2]) << 8) | int(q["data"][3])) == int(p["crc"]):
                want = int(p["sample"]) - int(q["sample"]) <= ttl
                break
        if want != bool(keep[i]):
            return False
    return True
