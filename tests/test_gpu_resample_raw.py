"""The resampler's raw entry on the MI355X: am_k_resample_raw<FMT> against arb_resampler.work_samples bit for bit (the checks of
tests/resample_raw_common.py), the interpolator and the receive path behind one another on one stream without a host wait,
and the command line on raw files below 4 Msps.  CPU twin: tests/test_resample_raw.py."""
import numpy as np
import pytest

import resample_raw_common as rc
from air_modes import _capi
from air_modes.resample import arb_resampler, gpu_resampler

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ratio", rc.RATIOS, ids=lambda r: "%.3f" % r)
@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_formats_ratios_and_history(hip_lib, fmt, ratio):
    assert not hip_lib.emulated
    rc.check_formats_ratios_history(hip_lib, fmt, ratio)


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_alignment(hip_lib, fmt):
    rc.check_alignment(hip_lib, fmt)


@pytest.mark.parametrize("check", rc.CHECKS, ids=lambda c: c.__name__[6:])
def test_resample_raw(hip_lib, check):
    check(hip_lib)


def test_resampler_and_receive_path_on_one_stream(hip_lib, oracle_mod):
    """Raw cu8 samples on the device -> work_device_samples -> rx_path's scan, the resampler on the context's stream and no
    host wait between the two: the packets are the oracle's on the definition's output."""
    import torch
    import synth
    import formats_common as fc
    iq, _ = synth.synth_capture(2e6, 400_000, 2500.0, seed=2024)
    raw = fc.quantise(iq, "cu8")
    dev = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    ctx = _capi.Context(4e6, 7.0, True, lib=hip_lib)
    rs = gpu_resampler(2.0, lib=hip_lib)
    rs.set_stream(ctx.stream())
    got = []
    cuts = [0, 150_001, 150_004, 300_000, 400_000]
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        last = c1 == cuts[-1]
        ptr, m = rs.work_device_samples(dev.data_ptr() + 2 * c0, c1 - c0, "cu8", flush=last)
        got.append(ctx.process_iq_device(ptr, m, flush=last))
    got = np.concatenate(got)
    want = oracle_mod.demod(arb_resampler(2.0).work_samples(raw, "cu8", flush=True), 4e6, 7.0, True)
    assert len(want) >= 50 and np.array_equal(got, want)
    rs.set_stream(None)
    rs.close()
    ctx.close()


@pytest.mark.parametrize("fmt,rate", [("cu8", 2e6), ("cu8", 2.4e6), ("sc16", 2e6), ("sc16", 2.4e6)])
def test_modes_rx_resamples_raw_files_in_place(hip_lib, oracle_mod, tmp_path, monkeypatch, fmt, rate):
    assert _capi.default_library().path == hip_lib.path
    rc.check_modes_rx(oracle_mod, tmp_path, monkeypatch, fmt, rate)
