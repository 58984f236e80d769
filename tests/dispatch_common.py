"""All nine <FIX, GATE> instantiations of the slicing kernels, reached through the library's one dispatch (am_dispatch.h), against
the existing numpy definitions composed: fix_common.slice_fix(..., F), then nothing (gate off), gate_common.gate (on) or
aprepair_common.repair (on with the address repair).

A setting that ran another setting's kernel would go unnoticed wherever the two give the same packets, so each input is first
shown -- on the CPU, before the library is asked -- to give nine expectations that differ pairwise as bytes.

tests/test_slice_dispatch.py runs this against the emulated library, tests/test_gpu_slice_dispatch.py on the device."""
import itertools

import numpy as np

import aprepair_common as ar
import fix_common as fx
import gate_common as gc
import oracle
import synth
from air_modes import _capi

RATE = 4e6
TTL_S = 60.0
TTL = gc.ttl_samples(TTL_S, RATE)
# (fix_errors, address gate mode, address repair): FIX = 0, 1, 2 crossed with GATE = 0, 1, 2
SETTINGS = [(f, m, r) for f in (0, 1, 2) for (m, r) in ((0, 0), (1, 0), (1, 1))]
# the capture of the production-path check: 4 Msps (am_k_extract_slice_iq<2, FIX, GATE>), 1 M samples of a fleet of 40 at
# SNR 4-14 dB -- wrong bits of every kind, some 300 hits
CAPTURE = (RATE, 1_000_000, 4000.0, 22, 40, (4.0, 14.0))


def clean_burst(frame, scale=1.0):
    b = np.zeros(240, np.float32)
    chips = synth.frame_chips(frame)
    b[:chips.size] = chips * np.float32(scale)
    return b


def flip(frame, *bits):
    f = bytearray(frame)
    for j in bits:
        f[j >> 3] ^= 0x80 >> (j & 7)
    return bytes(f)


def burst_list(seed=5):
    """A few hundred bursts with ascending item counts:
      - fix_common.damaged_bursts: DF11 / DF17 replies with 0-3 wrong bits (the clean ones teach their addresses),
      - the chip-exchanged twins of those the two-bit repair mends (fix_common.exchange_chips): clean as sliced,
      - a fleet of eight: a clean DF17 and a clean DF11 of every aircraft, then its address/parity replies, clean and with one wrong
        bit; a DF17 with one and with two wrong bits; a clean address/parity reply of an aircraft nobody taught,
      - one frame of a reserved format (DF19)."""
    rng = np.random.default_rng(seed)
    dam, dtags, _ = fx.damaged_bursts(240, seed)
    pk2, idx2, _ = fx.slice_fix(dam, dtags, 2)
    twins = fx.exchange_chips(dam, pk2, idx2)[0][:24]
    fleet = [int(a) for a in rng.choice(np.arange(1, 1 << 24), 8, replace=False)]
    rows = []
    for addr in fleet:
        rows.append(clean_burst(gc.fleet_frame(rng, 17, addr)))
        rows.append(clean_burst(gc.fleet_frame(rng, 11, addr), 0.25))
    for k, addr in enumerate(fleet * 4):
        df = gc.AP[k % len(gc.AP)]
        frame = gc.fleet_frame(rng, df, addr)
        nbits = 8 * len(frame)
        rows.append(clean_burst(frame))
        rows.append(clean_burst(flip(frame, int(rng.integers(5, nbits))), 3.0))
    for addr in fleet[:4]:
        frame = gc.fleet_frame(rng, 17, addr)
        a, b = sorted(int(x) for x in rng.choice(np.arange(5, 112), 2, replace=False))
        rows.append(clean_burst(flip(frame, a)))
        rows.append(clean_burst(flip(frame, a, b)))
    rows.append(clean_burst(gc.fleet_frame(rng, 4, 0x123456)))            # nobody taught this address
    rows.append(clean_burst(gc.fleet_frame(rng, 19, fleet[0])))           # a reserved format
    half = len(dam) // 2
    bursts = np.concatenate([dam[:half], np.array(rows, np.float32), twins, dam[half:]]).astype(np.float32)
    tags = np.zeros(len(bursts), oracle.TAG_DTYPE)
    tags["sample"] = np.arange(len(bursts), dtype=np.uint64) * 4801 + 7
    tags["secs"] = rng.integers(0, 1 << 33, len(bursts))
    tags["frac"] = rng.random(len(bursts))
    return bursts, tags


def compose(sliced, mode, repair):
    """What a stream's packets become behind the gate: sliced = fix_common.slice_fix(...)[0] or expected_from_capture(...)."""
    if mode == 0:
        return sliced
    if not repair:
        return sliced[gc.gate(sliced, mode, TTL)]
    return ar.repair(sliced, mode, TTL)[0]


def expectations(sliced_for):
    """{setting: packets}; sliced_for(F) = the packets as sliced with max_bits = F.  Asserts the condition."""
    sliced = {f: sliced_for(f) for f in (0, 1, 2)}
    want = {s: compose(sliced[s[0]], s[1], s[2]) for s in SETTINGS}
    for s in SETTINGS:
        print("fix %d gate %d repair %d: %d packets" % (s + (len(want[s]),)))
    for a, b in itertools.combinations(SETTINGS, 2):
        assert want[a].tobytes() != want[b].tobytes(), "settings %r and %r expect the same packets: the input tells nothing apart" % (a, b)
    return want


def configure(ctx, setting):
    f, mode, repair = setting
    ctx.set_fix_errors(f)
    ctx.set_address_gate(mode, TTL_S)
    ctx.set_address_repair(repair)
    ctx.reset()


def check_slicer_block(lib):
    """am_slicer_work -> am_k_slice<FIX, GATE>."""
    bursts, tags = burst_list()
    assert 200 <= len(bursts) <= 500
    want = expectations(lambda f: fx.slice_fix(bursts, tags, f)[0])
    # the list holds what it is meant to hold
    p0, p2 = want[(0, 0, 0)], want[(2, 0, 0)]
    assert (p2["reserved"][:, 1] == 1).any() and (p2["reserved"][:, 1] == 2).any() and (p0["df"] == 19).any()
    on, rep = want[(0, 1, 0)], want[(0, 1, 1)]
    assert np.isin(on["df"], gc.AP).any() and len(on) < len(p0) and (rep["reserved"][:, 1] == 1).sum() >= 8
    ctx = _capi.Context(RATE, 7.0, True, lib=lib)
    for s in SETTINGS:
        configure(ctx, s)
        got = ctx.slicer_work(bursts, tags)
        assert got.tobytes() == want[s].tobytes(), "fix %d gate %d repair %d: %d packets, expected %d" % (s + (len(got), len(want[s])))
    ctx.close()


def check_production_path(lib):
    """am_process_iq at 4 Msps -> the streaming front end and am_k_extract_slice_iq<2, FIX, GATE>."""
    oracle.build()
    iq = gc.fleet_capture(*CAPTURE)[0]
    assert len(iq) <= 4_000_000
    want = expectations(lambda f: fx.expected_from_capture(iq, RATE, f))
    ctx = _capi.Context(RATE, 7.0, True, lib=lib)
    for s in SETTINGS:
        configure(ctx, s)
        got = ctx.process_iq(iq, flush=True)
        assert ctx.last_frontend() == 3
        assert got.tobytes() == want[s].tobytes(), "fix %d gate %d repair %d: %d packets, expected %d" % (s + (len(got), len(want[s])))
    ctx.close()
