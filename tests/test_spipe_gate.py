"""The address gate and the address repair for ONE stream with chunks in flight (am_spipe_set_address_gate / _repair; DESIGN.md
16), on the emulated library: the packets of all chunks, in order, are the oracle's packets filtered by the numpy definitions in
tests/gate_common.py and tests/aprepair_common.py -- whatever the chunk sizes, the depth, the memory layout, and whether a chunk
was redone -- and the counters are the definition's."""
import ctypes as C

import numpy as np
import pytest

import aprepair_common as ar
import gate_common as gc
import oracle
from air_modes import _capi

AP = gc.AP
RATE = 4e6
N = 2_000_000
SNR = (4.0, 14.0)
EVEN = list(range(0, N + 1, 250_000))
UNEVEN = [0, 300_001, 520_000, 1_000_003, 1_210_000, 1_500_000, 1_777_777, N]
# every setting (mode, ttl in seconds, repair) meets every depth on either chunking: the gate off, and modes 1 / 2 with either
# window, the repair off and on
SETTINGS = ((0, 60.0, 0),) + tuple((m, t, r) for t in (0.05, 60.0) for m in (1, 2) for r in (0, 1))
_cache = {}


def capture():
    """(iq, truth, fleet, the oracle's packets).  The project's own yield table pins this capture at ttl 60 s; the
    pins are checked before the library is asked."""
    if "main" not in _cache:
        oracle.build()
        iq, truth, fleet = gc.fleet_capture(RATE, N, 4000.0, 22, 40, snr=SNR)
        pk = oracle.demod(iq, RATE, 7.0)
        ttl = gc.ttl_samples(60.0, RATE)
        keep = gc.gate(pk, 1, ttl)
        isap = np.isin(pk["df"], AP)
        _, _, fixed, amb = ar.repair(pk, 1, ttl)
        assert (int(isap.sum()), int((isap & keep).sum()), int((~keep).sum()), int((fixed >= 0).sum()), amb) == (331, 174, 157, 11, 0)
        _cache["main"] = (iq, truth, fleet, pk)
    return _cache["main"]


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


def chunks_of(iq, edges, front, contiguous, hold):
    f32 = np.ascontiguousarray(iq.view(np.float32))
    hold.append(f32)
    if contiguous:
        return [(f32.ctypes.data + 8 * a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        buf = np.full(2 * (front + (b - a)), np.float32(7.0))     # (garbage in front: the library puts the tail there)
        buf[2 * front:] = f32[2 * a:2 * b]
        hold.append(buf)
        out.append((buf.ctypes.data + 8 * front, b - a))
    return out


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


def send(pipe, iq, edges, contiguous=True):
    hold = []
    for a, b in zip(edges[:-1], edges[1:]):
        assert b - a > pipe.front()
    got = pipe.run(chunks_of(iq, edges, pipe.front(), contiguous, hold))
    return got


def even_chunk_counts(lib):
    """how many of the oracle's packets each of the eight even chunks hands out (gate off: the pipe's packets are the oracle's)"""
    if "even" not in _cache:
        iq, _, _, pk = capture()
        pipe = _capi.StreamPipe(RATE, 7.0, True, depth=4, lib=lib)
        got = send(pipe, iq, EVEN)
        pipe.close()
        assert np.concatenate(got).tobytes() == pk.tobytes()
        _cache["even"] = [len(g) for g in got]
    return _cache["even"]


def in_flight_teaches(pk, per_chunk, depth, ttl):
    """Over the oracle's packets, cut into chunks as the pipe hands them out: (kept, dropped) address/parity replies whose fate
    hangs on chunks that were in flight, not yet collected, when the reply's chunk was submitted (StreamPipe.run: the depth - 1
    chunks in front of it).  kept: every teach of its address inside the window lies in such a chunk; dropped: the address was
    last taught in such a chunk, and that teach has expired."""
    chunk = np.repeat(np.arange(len(per_chunk)), per_chunk)
    assert len(chunk) == len(pk)
    keep = gc.gate(pk, 1, ttl)
    teach = np.isin(pk["df"], (11, 17)) & (pk["crc"] == 0) & (pk["reserved"][:, 1] == 0)
    addr = np.array([ar.address_of(p) for p in pk])
    kept = dropped = 0
    for i in np.flatnonzero(np.isin(pk["df"], AP)):
        j, s = chunk[i], int(pk["sample"][i])
        before = np.flatnonzero(teach[:i] & (addr[:i] == int(pk["crc"][i])))
        if not len(before):
            continue
        flying = (chunk[before] < j) & (chunk[before] > j - depth)
        alive = s - pk["sample"][before].astype(np.int64) <= ttl
        if keep[i] and alive.any() and flying[alive].all():
            kept += 1
        if not keep[i] and flying[-1]:
            dropped += 1
    return kept, dropped


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("cutting", ["even", "uneven"])
def test_pipe_as_defined(emu_lib, depth, cutting):
    """Byte for byte and counter for counter, stream after stream through one pipe (every stream starts with an empty map; the
    counters add up since create); the uneven cuts go through buffers of their own."""
    iq, _, _, pk = capture()
    edges = EVEN if cutting == "even" else UNEVEN
    pipe = _capi.StreamPipe(RATE, 7.0, True, depth=depth, lib=emu_lib)
    books = Books()
    for mode, ttl_s, repair in SETTINGS:
        want, g, r = expected(pk, RATE, mode, ttl_s, repair)
        pipe.set_address_gate(mode, ttl_s)
        pipe.set_address_repair(repair)
        got = np.concatenate(send(pipe, iq, edges, contiguous=(cutting == "even")))
        assert got.tobytes() == want.tobytes(), "mode %d ttl %g repair %d: %d vs %d packets" % (mode, ttl_s, repair, len(got), len(want))
        books.add(g, r)
        books.check(pipe)
    assert pipe.redone() == 0
    pipe.close()


def test_the_capture_puts_teaches_in_chunks_still_in_flight(emu_lib):
    """ttl 0.05 s is 200 000 samples, shorter than a chunk: with four chunks in flight and eight chunks, a teach expires inside the
    span of chunks that are in flight together, and every slot is used again while predecessors are in flight."""
    pk = capture()[3]
    kept, dropped = in_flight_teaches(pk, even_chunk_counts(emu_lib), 4, gc.ttl_samples(0.05, RATE))
    print("address/parity replies that hang on chunks in flight: %d kept, %d dropped" % (kept, dropped))
    assert kept >= 1 and dropped >= 1


def test_second_stream_starts_with_an_empty_map(emu_lib):
    """A second stream of the same fleet that holds address/parity replies only: nobody teaches, so none of them is kept -- not
    even with the repair on, which finds its addresses in the same map."""
    iq, _, fleet, pk = capture()
    mix = ((0, 0.2), (4, 0.2), (5, 0.2), (20, 0.2), (21, 0.2))
    iq2, _, _ = gc.fleet_capture(RATE, 600_000, 4000.0, 23, 40, snr=(10.0, 30.0), fleet=fleet, mix=mix)
    pk2 = oracle.demod(iq2, RATE, 7.0)
    isap2 = np.isin(pk2["df"], AP)
    assert isap2.sum() >= 100 and np.isin(pk2["crc"][isap2], fleet).sum() >= 100 and not np.isin(pk2["df"], (11, 17)).any()
    pipe = _capi.StreamPipe(RATE, 7.0, True, depth=3, lib=emu_lib)
    pipe.set_address_gate(1, 60.0)
    pipe.set_address_repair(1)
    books = Books()
    want, g, r = expected(pk, RATE, 1, 60.0, 1)
    assert np.concatenate(send(pipe, iq, EVEN)).tobytes() == want.tobytes()
    books.add(g, r)
    want2, g2, r2 = expected(pk2, RATE, 1, 60.0, 1)
    assert not np.isin(want2["df"], AP).any() and g2[1] == 0 and r2 == (0, 0)
    got2 = np.concatenate(send(pipe, iq2, [0, 200_000, 400_000, 600_000]))
    assert got2.tobytes() == want2.tobytes()
    books.add(g2, r2)
    books.check(pipe)
    pipe.close()


def quiet_then_busy():
    """the same fleet, quiet first and busy after: the capacity extrapolated from the quiet chunks does not suffice"""
    if "redo" not in _cache:
        oracle.build()
        quiet, _, fleet = gc.fleet_capture(64e6, 1_200_000, 300.0, 71, 12, snr=(6.0, 30.0))
        busy, _, _ = gc.fleet_capture(64e6, 1_200_000, 30000.0, 72, 12, snr=(6.0, 30.0), fleet=fleet)
        iq = np.concatenate([quiet, busy])
        _cache["redo"] = (iq, oracle.demod(iq, 64e6, 7.0))
    return _cache["redo"]


def test_redone_chunks_teach_and_count_once(emu_lib, monkeypatch):
    """A chunk that takes the synchronous path, and the chunks drained and submitted again behind it, teach nothing and count
    nothing from the attempt that was thrown away: packets and counters are the definition's."""
    monkeypatch.setenv("AIRMODES_SPEC_FLOOR", "0")
    mode, ttl_s, repair = 1, 60.0, 1
    iq, pk = quiet_then_busy()
    n = len(iq)
    want, g, r = expected(pk, 64e6, mode, ttl_s, repair)
    isap = np.isin(pk["df"], AP)
    assert g[0] >= 10 and g[1] >= 10 and (isap & ~gc.gate(pk, mode, gc.ttl_samples(ttl_s, 64e6))).sum() >= 10
    pipe = _capi.StreamPipe(64e6, 7.0, True, depth=3, lib=emu_lib)
    pipe.set_address_gate(mode, ttl_s)
    pipe.set_address_repair(repair)
    got = np.concatenate(send(pipe, iq, list(range(0, n + 1, n // 8))))
    assert pipe.redone() >= 1, "no chunk took the synchronous path: the test did not reach it"
    assert got.tobytes() == want.tobytes(), "%d vs %d packets" % (len(got), len(want))
    books = Books()
    books.add(g, r)
    books.check(pipe)
    pipe.close()


def test_setters_and_getters(emu_lib):
    L = emu_lib.L
    iq, _, _, pk = capture()
    pipe = _capi.StreamPipe(RATE, 7.0, True, depth=2, lib=emu_lib)
    assert pipe.get_address_gate() == (0, 60.0) and pipe.get_address_repair() == 0
    for mode, ttl in ((-1, 60.0), (3, 60.0), (1, 0.0), (1, -1.0), (1, float("nan")), (1, float("inf"))):
        assert L.am_spipe_set_address_gate(pipe._h, mode, ttl) == _capi.AM_EINVAL
    for bits in (-1, 2):
        assert L.am_spipe_set_address_repair(pipe._h, bits) == _capi.AM_EINVAL
    assert pipe.get_address_gate() == (0, 60.0) and pipe.get_address_repair() == 0
    pipe.set_address_gate(2, 0.25)
    pipe.set_address_repair(1)
    assert pipe.get_address_gate() == (2, 0.25) and pipe.get_address_repair() == 1
    assert L.am_spipe_get_address_gate(pipe._h, None, None) == _capi.AM_OK
    assert L.am_spipe_get_address_gate_stats(pipe._h, None, None, None, None) == _capi.AM_OK
    assert L.am_spipe_get_address_repair_stats(pipe._h, None, None) == _capi.AM_OK
    assert L.am_spipe_set_address_gate(None, 1, 60.0) == _capi.AM_EINVAL
    assert L.am_spipe_get_address_gate(None, None, None) == _capi.AM_EINVAL
    assert L.am_spipe_get_address_gate_stats(None, None, None, None, None) == _capi.AM_EINVAL
    assert L.am_spipe_set_address_repair(None, 1) == _capi.AM_EINVAL
    assert L.am_spipe_get_address_repair(None) == _capi.AM_EINVAL
    assert L.am_spipe_get_address_repair_stats(None, None, None) == _capi.AM_EINVAL
    # with a chunk in flight the setting may not change
    hold = []
    chunks = chunks_of(iq[:600_000], [0, 300_000, 600_000], pipe.front(), True, hold)
    pipe.submit_device(*chunks[0])
    assert L.am_spipe_set_address_gate(pipe._h, 1, 60.0) == _capi.AM_EINVAL
    assert L.am_spipe_set_address_repair(pipe._h, 0) == _capi.AM_EINVAL
    assert pipe.get_address_gate() == (2, 0.25) and pipe.get_address_repair() == 1
    pipe.collect()
    # ... between two collected chunks of one stream it may, and the map is kept
    pipe.set_address_gate(1, 60.0)
    pipe.set_address_repair(0)
    pipe.submit_device(*chunks[1], flush=True)
    pipe.collect()
    pipe.close()


def test_new_setting_between_collected_chunks_keeps_the_map(emu_lib):
    """Mode 2 for the first half of a stream, mode 1 for the second: the second half's replies live on the first half's teaches."""
    iq, _, _, pk = capture()
    ttl = gc.ttl_samples(60.0, RATE)
    pipe = _capi.StreamPipe(RATE, 7.0, True, depth=2, lib=emu_lib)
    hold = []
    chunks = chunks_of(iq, EVEN, pipe.front(), True, hold)
    pipe.set_address_gate(2, 60.0)
    got = []
    for k, ch in enumerate(chunks):
        if k == 4:
            while pipe.in_flight():
                got.append(pipe.collect())
            pipe.set_address_gate(1, 60.0)
        if pipe.in_flight() == pipe.depth():
            got.append(pipe.collect())
        pipe.submit_device(*ch, flush=(k == len(chunks) - 1))
    while pipe.in_flight():
        got.append(pipe.collect())
    k1, k2 = gc.gate(pk, 1, ttl), gc.gate(pk, 2, ttl)
    m = sum(even_chunk_counts(emu_lib)[:4])                     # packets of the oracle that the first four chunks hand out
    want = np.concatenate([pk[:m][k2[:m]], pk[m:][k1[m:]]])
    assert 0 < m < len(pk) and (k1[m:] & np.isin(pk["df"][m:], AP)).sum() > 20
    assert np.concatenate(got).tobytes() == want.tobytes()
    pipe.close()


def test_a_collect_that_did_not_fit_counts_once(emu_lib):
    """AM_ECAPACITY from am_spipe_collect leaves the packets behind; collecting the chunk again teaches and counts once."""
    L = emu_lib.L
    iq, _, _, pk = capture()
    want, g, r = expected(pk, RATE, 1, 60.0, 1)
    pipe = _capi.StreamPipe(RATE, 7.0, True, depth=3, lib=emu_lib)
    pipe.set_address_gate(1, 60.0)
    pipe.set_address_repair(1)
    hold = []
    chunks = chunks_of(iq, EVEN, pipe.front(), True, hold)
    out = np.zeros(4096, _capi.PACKET_DTYPE)
    got, refused = [], 0

    def collect():
        n = C.c_uint64(0)
        rc = L.am_spipe_collect(pipe._h, out.ctypes.data, 3, C.byref(n))
        assert rc == _capi.AM_ECAPACITY and n.value > 3 and pipe.in_flight() >= 1
        rc = L.am_spipe_collect(pipe._h, out.ctypes.data, 2, C.byref(n))
        assert rc == _capi.AM_ECAPACITY
        assert L.am_spipe_collect(pipe._h, out.ctypes.data, len(out), C.byref(n)) == _capi.AM_OK
        got.append(out[:n.value].copy())
        return 2

    for k, ch in enumerate(chunks):
        if pipe.in_flight() == pipe.depth():
            refused += collect()
        pipe.submit_device(*ch, flush=(k == len(chunks) - 1))
    while pipe.in_flight():
        refused += collect()
    assert refused == 16
    assert np.concatenate(got).tobytes() == want.tobytes()
    books = Books()
    books.add(g, r)
    books.check(pipe)
    pipe.close()


def test_public_shard_calls_still_refuse_the_gate(emu_lib):
    iq = capture()[0][:400_000]
    ctx = _capi.Context(RATE, 7.0, True, lib=emu_lib)
    ctx.set_address_gate(1, 60.0)
    with pytest.raises(_capi.AirModesError) as e:
        ctx.shard_scan(iq, 0, len(iq), len(iq))
    assert e.value.code == _capi.AM_ENOTSUP
    with pytest.raises(_capi.AirModesError) as e:
        ctx.shard_resolve(0)
    assert e.value.code == _capi.AM_ENOTSUP
    L = emu_lib.L
    buf = np.zeros(16 * 520, np.uint8)
    f32 = np.ascontiguousarray(iq.view(np.float32))
    assert L.am_shard_scan_async(ctx._h, f32.ctypes.data, 0, len(iq), len(iq), _capi.AM_F_DEVICE_IN, buf.ctypes.data, 512) == _capi.AM_ENOTSUP
    assert L.am_shard_resolve_submit(ctx._h, buf.ctypes.data, 1, 0, 512, None, None) == _capi.AM_ENOTSUP
    ctx.set_address_gate(0, 60.0)
    ctx.shard_scan(iq, 0, len(iq), len(iq))
    assert ctx.shard_resolve(0).tobytes() == oracle.demod(iq, RATE, 7.0).tobytes()
    ctx.close()
