"""The resampler's raw entry on the CPU emulation of its kernel: sc16, cs8, cu8 (and cf32) samples resampled in one launch per
call, against arb_resampler.work_samples bit for bit, and the command line on raw files below 4 Msps.  The checks are
tests/resample_raw_common.py's; GPU twin: tests/test_gpu_resample_raw.py."""
import numpy as np
import pytest

import resample_raw_common as rc
from air_modes.resample import TAPS_PER_PHASE, arb_resampler


def test_definition_of_work_samples():
    """work_samples is work on formats.to_cf32 of the samples, the flush eight zero samples in the same call, then a reset."""
    from air_modes.formats import to_cf32
    raw = rc.samples("cu8", 3000, 3)
    a, b = arb_resampler(1.25), arb_resampler(1.25)
    x = to_cf32(raw, "cu8")
    want = b.work(np.concatenate([x, np.zeros(TAPS_PER_PHASE, np.complex64)]))
    got = np.concatenate([a.work_samples(raw[:2000], "cu8"), a.work_samples(raw[2000:], flush=True)])
    assert rc.same(got, want) and want.size > x.size
    assert rc.same(a.work_samples(raw, "cu8", flush=True), want)                # a new stream started
    assert a.work_samples(raw[:0], "cu8").size == 0


@pytest.mark.parametrize("ratio", rc.RATIOS, ids=lambda r: "%.3f" % r)
@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_formats_ratios_and_history(emu_lib, fmt, ratio):
    rc.check_formats_ratios_history(emu_lib, fmt, ratio)


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_alignment(emu_lib, fmt):
    rc.check_alignment(emu_lib, fmt)


@pytest.mark.parametrize("check", rc.CHECKS, ids=lambda c: c.__name__[6:])
def test_resample_raw(emu_lib, check):
    check(emu_lib)


@pytest.mark.parametrize("fmt,rate", [("cu8", 2e6), ("cu8", 2.4e6), ("sc16", 2e6), ("sc16", 2.4e6)])
def test_modes_rx_resamples_raw_files_in_place(emu_lib, oracle_mod, tmp_path, monkeypatch, fmt, rate):
    from conftest import EMU_LIB
    monkeypatch.setenv("AIRMODES_HIP_LIB", EMU_LIB)
    rc.check_modes_rx(oracle_mod, tmp_path, monkeypatch, fmt, rate)
