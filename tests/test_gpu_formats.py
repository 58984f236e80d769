"""Native sample formats (sc16, cs8, cu8) on the MI355X: am_k_unpack against its definition bit for bit (every length and
alignment, and a production-size stream), the receive path fed raw samples against the oracle on the converted capture,
and the command line on raw files.  CPU twin: tests/test_formats.py."""
import io

import numpy as np
import pytest

import formats_common as fc
from air_modes import _capi, formats
from air_modes.formats import to_cf32

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_unpack_matches_definition_at_every_length_and_alignment(hip_lib, fmt):
    assert not hip_lib.emulated
    fc.check_unpack(hip_lib, fmt)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_unpack_production_size(hip_lib, fmt):
    """64 M complex samples of seeded random integers, raw input resident on the device."""
    import torch
    n = 64 * 1024 * 1024
    raw = fc.random_raw(fmt, n, 64)
    ctx = _capi.Context(64e6, 7.0, True, lib=hip_lib)
    raw_dev = torch.from_numpy(raw.view(np.uint8)).cuda()
    guard = 4                                                        # float32 words either side
    out = torch.full((2 * n + 2 * guard,), float("inf"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert ctx.unpack(raw_dev.data_ptr(), fmt, out.data_ptr() + 4 * guard, n_complex=n) == n
    ctx.synchronize()
    got = out.cpu().numpy()
    ctx.close()
    assert np.all(np.isinf(got[:guard])) and np.all(np.isinf(got[-guard:]))
    want = to_cf32(raw, fmt)
    assert np.array_equal(fc.u32(got[guard:-guard]), fc.u32(want))


# 64 Msps with 8 000 000 samples: am_k_fe3 walks several steps per workgroup
GPU_CAPTURES = {2: 2, 20: 20, 64: (64e6, 8_000_000, 5000.0)}


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("key", [2, 20, 64])
def test_raw_chunks_give_the_packets_of_the_converted_capture(hip_lib, oracle_mod, key, fmt):
    fc.check_packets(hip_lib, GPU_CAPTURES[key], fmt, seed=7 * key + len(fmt))


@pytest.mark.parametrize("opts", [dict(use_dcblock=True), dict(use_pmf=False), dict(rx_time=(100_003, 1_600_000_000, 0.625))],
                         ids=lambda o: "-".join(sorted(o)))
def test_raw_chunks_with_options(hip_lib, oracle_mod, opts):
    fc.check_packets(hip_lib, 20, "cu8", seed=99, **opts)


def test_raw_samples_resident_on_the_device(hip_lib, oracle_mod):
    """rx_path.work_device(fmt=...): zero host copies, chunked, against the host-input result."""
    import torch
    import air_modes
    rate, raw = fc.raw_capture(20, "sc16")
    n = raw.size // 2
    want = air_modes.rx_path(rate, 7.0, air_modes.msg_queue(), use_pmf=True, lib=hip_lib).work(to_cf32(raw), flush=True)
    dev = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    rx = air_modes.rx_path(rate, 7.0, air_modes.msg_queue(), use_pmf=True, lib=hip_lib)
    edges = [0] + fc.cut_points(n, 5) + [n]
    got = np.concatenate([rx.work_device(dev.data_ptr() + 4 * a, b - a, flush=(b == n), fmt="sc16")
                          for a, b in zip(edges[:-1], edges[1:])])
    assert len(want) >= 50 and np.array_equal(got, want)


@pytest.mark.parametrize("fmt,rate,n,extra", [("cu8", 2e6, 400_000, []), ("cu8", 2e6, 400_000, ["--no-resample"]),
                                               ("sc16", 20e6, 2_000_000, [])])
def test_modes_rx_reads_native_formats(hip_lib, tmp_path, fmt, rate, n, extra):
    """stdout of the command line on a raw file == on the .cf32 file written from to_cf32 of the same data."""
    from air_modes import modes_rx
    assert _capi.default_library().path == hip_lib.path
    _, raw = fc.raw_capture((rate, n, 2500.0), fmt)
    by_suffix, plain, ref = tmp_path / ("x." + fmt), tmp_path / "x.bin", tmp_path / "x.cf32"
    raw.tofile(by_suffix)
    raw.tofile(plain)
    to_cf32(raw).tofile(ref)
    outs = []
    for argv in (["-s", str(ref)], ["-s", str(by_suffix)], ["-s", str(plain), "-f", fmt]):
        o = io.StringIO()
        assert modes_rx.main(argv + ["-r", repr(rate), "--raw", "--chunk", "150001"] + extra, out=o) == 0
        outs.append(o.getvalue())
    assert len(outs[0].splitlines()) >= 50
    assert outs[1] == outs[0] and outs[2] == outs[0]
