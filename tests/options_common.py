"""The four opt-in decode options (fix_errors, long_formats, address_gate, address_repair) behind the three handle kinds
(Context = am_ctx, Pipe = am_pipe, StreamPipe = am_spipe): the setters' and getters' contract, handle kind by handle kind, and
that a setting given to a pipe reaches whichever context does the work.

tests/test_option_surface.py runs this against the emulated library, tests/test_gpu_options.py runs the second part on the
device."""
import ctypes as C

import numpy as np

import gate_common as gc
import longfmt_common as lf
from air_modes import _capi

RATE = 4e6
N = 1_000_000
CUT = 400_000
EINVAL = _capi.AM_EINVAL
# option -> (a value that is accepted and is not the default, values just outside each end of its range)
OPTIONS = {
    "fix_errors": ((2,), ((-1,), (3,))),
    "long_formats": ((3,), ((-1,), (4,))),
    "address_gate": ((2, 0.25), ((-1, 60.0), (3, 60.0), (1, 0.0), (1, -1.0), (1, float("nan")), (1, float("inf")))),
    "address_repair": ((1,), ((-1,), (2,))),
}
DEFAULTS = {"fix_errors": (0,), "long_formats": (0,), "address_gate": (0, 60.0), "address_repair": (0,)}
KINDS = {"am_": _capi.Context, "am_pipe_": _capi.Pipe, "am_spipe_": _capi.StreamPipe}
_cache = {}


def _get(L, prefix, option, handle):
    """(return code, value as a tuple) from the C getter"""
    f = getattr(L, prefix + "get_" + option)
    if option == "address_gate":
        mode, ttl = C.c_int(-7), C.c_double(-7.0)
        rc = f(handle, C.byref(mode), C.byref(ttl))
        return rc, (mode.value, ttl.value)
    rc = f(handle)
    return (rc if rc < 0 else _capi.AM_OK), (rc,)


def _last_error(L, prefix, handle):
    return getattr(L, prefix + "last_error")(handle).decode()


def check_surface(lib, prefix, option):
    """One handle kind, one option: null handle, values out of range, work in flight, and the same call after collecting."""
    L = lib.L
    good, bad = OPTIONS[option]
    setter = getattr(L, prefix + "set_" + option)
    assert setter(None, *good) == EINVAL and _get(L, prefix, option, None)[0] == EINVAL
    obj = KINDS[prefix](RATE, 7.0, True, lib=lib) if prefix == "am_" else KINDS[prefix](RATE, 7.0, True, depth=2, lib=lib)
    h = obj._h
    assert _get(L, prefix, option, h) == (_capi.AM_OK, DEFAULTS[option]) and _last_error(L, prefix, h) == ""
    range_texts = set()
    for v in bad:
        assert setter(h, *v) == EINVAL, (prefix, option, v)
        assert _get(L, prefix, option, h) == (_capi.AM_OK, DEFAULTS[option]), (prefix, option, v)
        assert _last_error(L, prefix, h) != "", (prefix, option, v)
        range_texts.add(_last_error(L, prefix, h))
    if prefix != "am_":
        rng = np.random.default_rng(3)
        f32 = (rng.standard_normal(2 * 100_000) * 0.01).astype(np.float32)      # (longer than StreamPipe.front(); noise only)
        if prefix == "am_pipe_":
            obj.submit(f32)
        else:
            assert len(f32) // 2 > obj.front()
            obj.submit_device(f32.ctypes.data, len(f32) // 2, flush=True)
        assert obj.in_flight() == 1
        assert setter(h, *good) == EINVAL
        assert _get(L, prefix, option, h) == (_capi.AM_OK, DEFAULTS[option])
        busy_text = _last_error(L, prefix, h)
        assert busy_text != "" and busy_text not in range_texts               # (a message of its own, not the last one left over)
        for v in bad:                                                         # out of range stays out of range
            assert setter(h, *v) == EINVAL
        obj.collect()
        assert obj.in_flight() == 0
    assert setter(h, *good) == _capi.AM_OK
    assert _get(L, prefix, option, h) == (_capi.AM_OK, good)
    for other in OPTIONS:                                                     # ... and no other option moved
        if other != option:
            assert _get(L, prefix, other, h) == (_capi.AM_OK, DEFAULTS[other])
    obj.close()


def capture():
    """4 Msps, 1 000 000 samples, two existing generators on top of each other: gate_common.fleet_capture -- DF11 / DF17 replies
    and address/parity replies of a fleet of 40 at SNR 4-14 dB (wrong bits of every kind; replies of aircraft that were and were
    not taught yet) -- and longfmt_common.capture: the edge formats with clean-PI DF18 / DF19 squitters at SNR 6-14 dB."""
    if "iq" not in _cache:
        fleet = gc.fleet_capture(RATE, N, 4000.0, 22, 40, (4.0, 14.0))[0]
        squitters = lf.capture(RATE, N, 2000.0, 33)[0]
        _cache["iq"] = (fleet + squitters).astype(np.complex64)
    return _cache["iq"]


def _configure(obj, fix=2, gate=1, repair=1, long_=3):
    obj.set_fix_errors(fix)
    obj.set_address_gate(gate)              # (the default ttl)
    obj.set_address_repair(repair)
    obj.set_long_formats(long_)


def check_options_reach_every_handle(lib, to_device):
    """All four options on.  What a Context hands out for the capture is what a Pipe hands out for it as either of two batches in
    flight and what a StreamPipe hands out for it cut in two, byte for byte -- and it is not what the Context hands out with any
    one of the options off, so an option that did not reach the contexts behind a pipe would show.
    to_device(float32 array) -> (pointer the library may read as device memory, what keeps it alive)."""
    iq = capture()
    assert len(iq) == N
    ctx = _capi.Context(RATE, 7.0, True, lib=lib)
    _configure(ctx)
    want = ctx.process_iq(iq, flush=True)
    r, ap, long_on = want["reserved"][:, 1], np.isin(want["df"], gc.AP), want["nbytes"] == 14
    counts = dict(packets=len(want), df18=int((long_on & (want["df"] == 18)).sum()), df19=int((long_on & (want["df"] == 19)).sum()),
                  fixed1=int((~ap & (r == 1)).sum()), fixed2=int((r == 2).sum()), ap_kept=int((ap & (r == 0)).sum()),
                  ap_repaired=int((ap & (r == 1)).sum()))
    print("all four options on:", counts)
    assert min(counts.values()) >= 1, counts
    for name, off in (("fix_errors", dict(fix=0)), ("address_gate", dict(gate=0)), ("address_repair", dict(repair=0)),
                      ("long_formats", dict(long_=0))):
        _configure(ctx, **off)
        other = ctx.process_iq(iq, flush=True)
        print("%s off: %d packets" % (name, len(other)))
        assert other.tobytes() != want.tobytes(), "%s makes no difference on this capture: the test would tell nothing" % name
    ctx.close()
    pipe = _capi.Pipe(RATE, 7.0, True, depth=2, lib=lib)
    _configure(pipe)
    pipe.submit(iq)
    pipe.submit(iq)
    assert pipe.in_flight() == 2
    for k in range(2):
        got = pipe.collect()
        assert got.tobytes() == want.tobytes(), "Pipe, batch %d: %d packets, the Context hands out %d" % (k, len(got), len(want))
    pipe.close()
    sp = _capi.StreamPipe(RATE, 7.0, True, depth=2, lib=lib)
    _configure(sp)
    base, hold = to_device(np.ascontiguousarray(iq.view(np.float32)))
    assert CUT > sp.front() and N - CUT > sp.front()
    sp.submit_device(base, CUT)
    sp.submit_device(base + 8 * CUT, N - CUT, flush=True)
    assert sp.in_flight() == 2
    got = np.concatenate([sp.collect(), sp.collect()])
    assert got.tobytes() == want.tobytes(), "StreamPipe: %d packets, the Context hands out %d" % (len(got), len(want))
    sp.close()
    del hold
