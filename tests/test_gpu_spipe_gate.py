"""The address gate and the address repair for ONE stream with chunks in flight (am_spipe_set_address_gate / _repair; DESIGN.md
16) on the device: every chunk's gate kernels on a context and a stream of its own, the pipe's running map handed from chunk to
chunk by events.  Byte for byte against the numpy definitions in tests/gate_common.py and tests/aprepair_common.py applied to the
oracle's packets, and counter for counter."""
import numpy as np
import pytest

import aprepair_common as ar
import gate_common as gc
import oracle
from air_modes import _capi

pytestmark = pytest.mark.gpu

AP = gc.AP
# the two fleet captures tests/test_gpu_address_gate.py pins: (rate, samples, bursts per second, seed, fleet, SNR), the two windows
# in seconds, packets, and per window what the definition keeps (mode 1, mode 2) and repairs (mode 1)
CAPTURES = {64: ((64e6, 16_000_000, 20000.0, 24, 30, (6.0, 30.0)), (60.0, 0.01), 549, {60.0: (369, 361, 8), 0.01: (235, 227, 1)}),
            20: ((20e6, 20_000_000, 5000.0, 23, 60, (6.0, 30.0)), (60.0, 0.02), 2339, {60.0: (2107, 2104, 14), 0.02: (1399, 1396, 2)})}
_cache = {}


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    oracle.build()
    return hip_lib


def expected(pk, rate, mode, ttl_s, repair):
    """(packets, (taught, passed, dropped), (repaired, ambiguous)) by the definition"""
    ttl = gc.ttl_samples(ttl_s, rate)
    if mode == 0:
        return pk, (0, 0, 0), (0, 0)
    if not repair:
        keep = gc.gate(pk, mode, ttl)
        return pk[keep], gc.counts(pk, keep), (0, 0)
    out, keep, fixed, amb = ar.repair(pk, mode, ttl)
    c = ar.counts(pk, keep, fixed)
    return out, c[:3], (c[3], amb)


def capture(msps):
    """(iq, the oracle's packets, {(mode, ttl, repair): expectation}); the pins are checked BEFORE the library is asked."""
    if msps not in _cache:
        args, ttls, n_pk, pins = CAPTURES[msps]
        iq, _, _ = gc.fleet_capture(*args)
        pk = oracle.demod(iq, args[0], 7.0)
        assert len(pk) == n_pk
        want = {(0, ttls[0], 0): expected(pk, args[0], 0, ttls[0], 0)}
        for ttl_s in ttls:
            for mode in (1, 2):
                for repair in (0, 1):
                    want[(mode, ttl_s, repair)] = expected(pk, args[0], mode, ttl_s, repair)
            got = (len(want[(1, ttl_s, 0)][0]), len(want[(2, ttl_s, 0)][0]), want[(1, ttl_s, 1)][2][0])
            print("capture %g Msps, ttl %g s: %d packets -> %d / %d kept, %d repaired" % ((msps, ttl_s, len(pk)) + got))
            assert got == pins[ttl_s] and want[(1, ttl_s, 1)][2][1] == 0
        _cache[msps] = (iq, pk, want)
    return _cache[msps]


def even_cuts(n, k=8):
    return [n * i // k for i in range(k)] + [n]


def uneven_cuts(n):
    return [0, n // 7 + 1, n // 7 + 20_000, n // 2 + 13, n - n // 5, n - 33_333, n]


def device_chunks(iq, edges, front, contiguous, hold):
    """chunks of the stream in device memory: one allocation, or every chunk in a buffer of its own with room in front of it"""
    import torch
    f32 = np.ascontiguousarray(iq.view(np.float32))
    if contiguous:
        base = torch.from_numpy(f32).to("cuda:0")
        hold.append(base)
        chunks = [(base.data_ptr() + 8 * a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    else:
        chunks = []
        for a, b in zip(edges[:-1], edges[1:]):
            buf = torch.full((2 * (front + (b - a)),), 7.0, dtype=torch.float32, device="cuda:0")     # (garbage in front)
            buf[2 * front:].copy_(torch.from_numpy(f32[2 * a:2 * b]))
            hold.append(buf)
            chunks.append((buf.data_ptr() + 8 * front, b - a))
    torch.cuda.synchronize()
    for _, m in chunks:
        assert m > front
    return chunks


class Books(object):
    """what the pipe's counters must read after the streams sent so far"""

    def __init__(self):
        self.gate = dict(taught=0, passed=0, dropped=0, not_learned=0)
        self.rep = dict(repaired=0, ambiguous=0)

    def add(self, g, r):
        for key, v in zip(("taught", "passed", "dropped"), g):
            self.gate[key] += v
        self.rep["repaired"] += r[0]
        self.rep["ambiguous"] += r[1]

    def check(self, pipe):
        assert pipe.address_gate_stats() == self.gate and pipe.address_repair_stats() == self.rep


@pytest.mark.parametrize("contiguous", [True, False])
@pytest.mark.parametrize("msps", [64, 20])
def test_pipe_as_defined(lib, msps, contiguous):
    """Eight equal chunks and uneven cuts, three and four chunks in flight, modes 0 / 1 / 2, two windows (the short one is shorter
    than a chunk), the repair off and on: stream after stream through one pipe, packets and counters as defined."""
    iq, pk, want = capture(msps)
    rate, n = CAPTURES[msps][0][0], len(iq)
    for cuts in (even_cuts(n), uneven_cuts(n)):
        hold = []
        for depth in (3, 4):
            pipe = _capi.StreamPipe(rate, 7.0, True, depth=depth, lib=lib, device=0)
            if not hold:
                chunks = device_chunks(iq, cuts, pipe.front(), contiguous, hold)
            books = Books()
            for (mode, ttl_s, repair), (packets, g, r) in want.items():
                pipe.set_address_gate(mode, ttl_s)
                pipe.set_address_repair(repair)
                got = np.concatenate(pipe.run(chunks))
                assert got.tobytes() == packets.tobytes(), "depth %d mode %d ttl %g repair %d: %d vs %d packets" % (
                    depth, mode, ttl_s, repair, len(got), len(packets))
                books.add(g, r)
                books.check(pipe)
            assert pipe.redone() == 0
            pipe.close()
        del hold


def test_off_means_off(lib):
    """Mode 0 after mode 2 with the repair on: what a fresh pipe hands out, and what the oracle does."""
    iq, pk, want = capture(64)
    hold = []
    pipe = _capi.StreamPipe(64e6, 7.0, True, depth=4, lib=lib, device=0)
    chunks = device_chunks(iq, even_cuts(len(iq)), pipe.front(), True, hold)
    pipe.set_address_gate(2, 0.01)
    pipe.set_address_repair(1)
    assert np.concatenate(pipe.run(chunks)).tobytes() == want[(2, 0.01, 1)][0].tobytes()
    stats = (pipe.address_gate_stats(), pipe.address_repair_stats())
    pipe.set_address_gate(0, 0.01)
    off = pipe.run(chunks)
    fresh = _capi.StreamPipe(64e6, 7.0, True, depth=4, lib=lib, device=0)
    new = fresh.run(chunks)
    assert [g.tobytes() for g in off] == [g.tobytes() for g in new] and np.concatenate(off).tobytes() == pk.tobytes()
    assert (pipe.address_gate_stats(), pipe.address_repair_stats()) == stats
    pipe.close()
    fresh.close()


def test_redone_chunks_teach_and_count_once_on_device(lib, hip_knobs_lib, monkeypatch):
    """A quiet first half, dense traffic of the same fleet behind it, no slack in the capacity estimate: some chunk takes the
    synchronous path, the chunks behind it are drained and submitted again -- and nothing of the attempt that was thrown away
    has taught or counted."""
    monkeypatch.setenv("AIRMODES_SPEC_FLOOR", "0")
    rate = 64e6
    quiet, _, fleet = gc.fleet_capture(rate, 8_000_000, 300.0, 71, 30, (6.0, 30.0))
    busy, _, _ = gc.fleet_capture(rate, 8_000_000, 30000.0, 72, 30, (6.0, 30.0), fleet=fleet)
    iq = np.concatenate([quiet, busy])
    pk = oracle.demod(iq, rate, 7.0)
    packets, g, r = expected(pk, rate, 1, 60.0, 1)
    print("quiet, then busy: %d packets, taught / passed / dropped %s, repaired / ambiguous %s" % (len(pk), g, r))
    assert (len(pk), g, r) == (233, (83, 54, 87), (4, 0))
    hold = []
    pipe = _capi.StreamPipe(rate, 7.0, True, depth=3, lib=hip_knobs_lib, device=0)
    pipe.set_address_gate(1, 60.0)
    pipe.set_address_repair(1)
    got = np.concatenate(pipe.run(device_chunks(iq, even_cuts(len(iq)), pipe.front(), True, hold)))
    assert pipe.redone() >= 1, "no chunk took the synchronous path: the test did not reach it"
    assert got.tobytes() == packets.tobytes(), "%d vs %d packets" % (len(got), len(packets))
    books = Books()
    books.add(g, r)
    books.check(pipe)
    pipe.close()


def test_silent_chunks_hand_the_order_on(lib):
    """Two busy segments of one fleet with 4 M zeros between them, ten chunks, three in flight: the chunks inside the silence have
    nothing to slice and launch no gate of their own, and the second segment's replies still find what the first one taught."""
    rate = 64e6
    a, _, fleet = gc.fleet_capture(rate, 2_000_000, 20000.0, 81, 20, (6.0, 30.0))
    b, _, _ = gc.fleet_capture(rate, 2_000_000, 20000.0, 82, 20, (6.0, 30.0), fleet=fleet)
    iq = np.concatenate([a, np.zeros(4_000_000, np.complex64), b])
    pk = oracle.demod(iq, rate, 7.0)
    packets, g, r = expected(pk, rate, 1, 60.0, 1)
    # replies of the second segment that are kept on teaches of the first segment alone
    keep = gc.gate(pk, 1, gc.ttl_samples(60.0, rate))
    second = pk["sample"] >= 6_000_000
    teach = np.isin(pk["df"], (11, 17)) & (pk["crc"] == 0)
    addr = np.array([ar.address_of(p) for p in pk])
    lives_on_first = 0
    for i in np.flatnonzero(second & np.isin(pk["df"], AP) & keep):
        before = np.flatnonzero(teach[:i] & (addr[:i] == int(pk["crc"][i])))
        lives_on_first += int(len(before) > 0 and not second[before].any())
    print("silence: %d packets, %s, %s; %d replies behind it live on teaches in front of it" % (len(pk), g, r, lives_on_first))
    assert (len(pk), g, r, lives_on_first) == (154, (50, 30, 71), (3, 0), 8)
    hold = []
    for depth in (3, 4):
        pipe = _capi.StreamPipe(rate, 7.0, True, depth=depth, lib=lib, device=0)
        pipe.set_address_gate(1, 60.0)
        pipe.set_address_repair(1)
        got = pipe.run(device_chunks(iq, even_cuts(len(iq), 10), pipe.front(), True, hold))
        assert sum(1 for x in got if len(x) == 0) >= 3 and pipe.redone() == 0
        assert np.concatenate(got).tobytes() == packets.tobytes()
        books = Books()
        books.add(g, r)
        books.check(pipe)
        pipe.close()
