"""Native sample formats (sc16, cs8, cu8) on the CPU emulation of the kernels: the definition (air_modes/formats.py),
the unpack kernel against it bit for bit at every length and alignment, and the receive path fed raw samples against the
oracle on the converted capture.  The same checks run on the GPU in tests/test_gpu_formats.py."""
import ctypes as C

import numpy as np
import pytest

import formats_common as fc
from air_modes import _capi, formats
from air_modes.formats import to_cf32


def test_to_cf32_hand_written_values():
    def one(values, dtype):
        return to_cf32(np.array(values, dtype)).view(np.float32)
    assert one([-32768, 32767], np.int16).tolist() == [-1.0, 0.999969482421875]
    assert one([-128, 127], np.int8).tolist() == [-1.0, 0.9921875]
    assert one([0, 255, 128, 127], np.uint8).tolist() == [-0.99609375, 0.99609375, 0.00390625, -0.00390625]
    x = np.array([1.5, -2.25], np.float32)
    assert to_cf32(x).dtype == np.complex64 and to_cf32(x).view(np.float32).tolist() == [1.5, -2.25]
    assert to_cf32(np.array([[1, 2], [3, 4]], np.int8)).tolist() == [(1 + 2j) / 128, (3 + 4j) / 128]    # shape (n, 2)
    assert [formats.bytes_per_sample(f) for f in ("cf32", "sc16", "cs8", "cu8")] == [8, 4, 2, 2]
    for dt, name in ((np.int16, "sc16"), (np.int8, "cs8"), (np.uint8, "cu8"), (np.float32, "cf32"), (np.complex64, "cf32")):
        assert formats.format_of(np.zeros(4, dt)) == name
    with pytest.raises(TypeError):
        formats.format_of(np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        formats.bytes_per_sample("cs12")
    # every value of every integer format: exact in float32 (the float64 evaluation of the table gives the same numbers)
    for fmt, scale, offset in (("sc16", 2.0 ** -15, 0.0), ("cs8", 2.0 ** -7, 0.0), ("cu8", 2.0 ** -7, 127.5)):
        info = np.iinfo(formats.component_dtype(fmt))
        allv = np.arange(info.min, info.max + 1).astype(formats.component_dtype(fmt))
        allv = np.concatenate([allv, allv[:allv.size % 2]])
        got = to_cf32(allv, fmt).view(np.float32).astype(np.float64)
        assert np.array_equal(got, (allv.astype(np.float64) - offset) * scale)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_unpack_matches_definition_at_every_length_and_alignment(emu_lib, fmt):
    fc.check_unpack(emu_lib, fmt)


CASES = [(key, fmt, {}) for key in (2, 4, 20, 64) for fmt in fc.RAW_FORMATS]
CASES += [(4, "cu8", dict(use_dcblock=True)), (20, "sc16", dict(use_pmf=False)),
          (2, "cs8", dict(rx_time=(100_003, 1_600_000_000, 0.625))), (4, "sc16", dict(shape2=True))]


@pytest.mark.parametrize("key,fmt,opts", CASES, ids=lambda v: "-".join(sorted(v)) if isinstance(v, dict) else str(v))
def test_raw_chunks_give_the_packets_of_the_converted_capture(emu_lib, oracle_mod, key, fmt, opts):
    fc.check_packets(emu_lib, key, fmt, seed=7 * key + len(fmt), **opts)


def test_process_samples_entry_points(emu_lib, oracle_mod):
    L = emu_lib.L
    assert [L.am_sample_bytes(f) for f in (0, 1, 2, 3, 7, -1)] == [8, 4, 2, 2, 0, 0]
    assert (formats.CF32, formats.SC16, formats.CS8, formats.CU8) == (0, 1, 2, 3)
    rate, raw = fc.raw_capture(2, "cu8")
    iq = to_cf32(raw)
    a = _capi.Context(rate, 7.0, True, lib=emu_lib)
    b = _capi.Context(rate, 7.0, True, lib=emu_lib)
    half = len(iq) // 2 + 1
    want = np.concatenate([a.process_iq(iq[:half]), a.process_iq(iq[half:], flush=True)])
    got = np.concatenate([b.process_samples(iq[:half], "cf32"), b.process_samples(iq[half:].view(np.float32), flush=True)])
    assert len(want) >= 50 and np.array_equal(got, want)                     # AM_FMT_CF32 is am_process_iq
    assert np.array_equal(b.process_samples(raw, "cu8", flush=True), want)
    assert np.array_equal(b.process_samples_device(raw.ctypes.data, raw.size // 2, "cu8", flush=True), want)   # (emulation: host = device)
    out = np.zeros(64, _capi.PACKET_DTYPE)
    got_n = C.c_uint64(9)
    for args in ((raw.ctypes.data, 16, 7), (raw.ctypes.data, 16, -1), (None, 16, formats.CU8), (None, 16, formats.CF32)):
        rc = L.am_process_samples(b._h, args[0], args[1], args[2], 0, out.ctypes.data, 64, C.byref(got_n))
        assert rc == _capi.AM_EINVAL and L.am_last_error(b._h)
        fbuf = np.zeros(64, np.float32)
        assert L.am_unpack(b._h, args[0], args[1], args[2], 0, fbuf.ctypes.data) == _capi.AM_EINVAL and L.am_last_error(b._h)
    assert b"format" in L.am_last_error(b._h) or b"null" in L.am_last_error(b._h)
    assert L.am_unpack(b._h, raw.ctypes.data, 16, formats.CU8, 0, None) == _capi.AM_EINVAL
    assert L.am_process_samples(b._h, None, 0, formats.CU8, _capi.AM_F_FLUSH, out.ctypes.data, 64, C.byref(got_n)) == 0   # an empty chunk is fine
    with pytest.raises(TypeError):
        b.process_samples(raw, "cs8")                                           # the dtype says cu8
    with pytest.raises(ValueError):
        b.process_samples(raw[:3])
    # the stream after the failed calls is intact
    assert np.array_equal(b.process_samples(raw, flush=True), want)
    a.close(); b.close()


def test_uploader_start_bytes(emu_lib):
    up = _capi.Uploader(1000, nslots=2, lib=emu_lib)
    raw = fc.random_raw("cu8", 1000, 5)
    memoryview(up.buffer(1)).cast("B")[:raw.size] = raw.tobytes()
    up.start_bytes(1, raw.size)
    ptr = up.wait(1)
    assert bytes((C.c_ubyte * raw.size).from_address(ptr)) == raw.tobytes()
    up.start_bytes(0, 8000)
    with pytest.raises(_capi.AirModesError):
        up.start_bytes(0, 8001)                                                 # a slot holds capacity * 8 bytes
    up.close()


@pytest.mark.parametrize("fmt,rate,extra", [("cu8", 2e6, []), ("cu8", 2e6, ["--no-resample"]), ("sc16", 4e6, []), ("cs8", 2e6, [])])
def test_modes_rx_reads_native_formats(emu_lib, tmp_path, monkeypatch, fmt, rate, extra):
    """The command line on a raw file == on the .cf32 file written from to_cf32 of the same data; suffix and -f agree."""
    import io
    from conftest import EMU_LIB
    from air_modes import modes_rx
    _, raw = fc.raw_capture((rate, 300_000, 2500.0), fmt)
    monkeypatch.setenv("AIRMODES_HIP_LIB", EMU_LIB)
    by_suffix, plain, ref = tmp_path / ("cap." + fmt), tmp_path / "cap.bin", tmp_path / "cap.cf32"
    raw.tofile(by_suffix)
    with open(plain, "wb") as f:
        f.write(raw.tobytes() + b"\x01")                                        # a trailing partial sample is dropped
    to_cf32(raw).tofile(ref)
    outs = []
    for argv in (["-s", str(ref)], ["-s", str(by_suffix)], ["-s", str(plain), "-f", fmt]):
        o = io.StringIO()
        assert modes_rx.main(argv + ["-r", repr(rate), "--raw", "--chunk", "70001"] + extra, out=o) == 0
        outs.append(o.getvalue())
    assert len(outs[0].splitlines()) >= 50
    assert outs[1] == outs[0] and outs[2] == outs[0]
    assert modes_rx.source_format("x.CS16") == "sc16" and modes_rx.source_format("x.cu8", "cs8") == "cs8"
    assert modes_rx.source_format("x.dat") == "cf32"
