"""Boundary vectors for the preamble detector on the GPU: the checks of tests/test_detector.py (tests/detector_common.py) against
the real library at every whole-chip rate, and against the test build that runs the rate-generic and the tile kernels."""
import numpy as np
import pytest
import torch

import detector_common as dc
import parity_common as pc

pytestmark = pytest.mark.gpu

RATES = (2e6, 4e6, 8e6, 10e6, 16e6, 20e6, 32e6, 40e6, 64e6)
PLAN = dc.stream_plan(RATES)
_id = dc.case_id


@pytest.mark.parametrize("thr", [0.0, 7.0, 20.0], ids=_id)
@pytest.mark.parametrize("rate", RATES, ids=_id)
def test_block_vectors(hip_lib, oracle_mod, rate, thr):
    assert dc.check_block(hip_lib, rate, int(rate / 1e6) + int(thr), thr) > 100


@pytest.mark.parametrize("rate,pmf,thr", PLAN, ids=_id)
def test_stream_vectors(hip_lib, oracle_mod, rate, pmf, thr):
    npk, iq = dc.check_streams(hip_lib, rate, pmf, int(rate / 1e6), thr)
    assert npk > 30
    if rate == 64e6 and thr == 7.0:
        pc.check_stream_pipe(hip_lib, rate, len(iq), 0.0, 5, thr=thr, pmf=pmf, iq=np.array(iq), device=torch.device("cuda", 0))


@pytest.mark.parametrize("knob", [("AIRMODES_GENERIC", "1", 1), ("AIRMODES_FE", "2", 2), ("AIRMODES_FUSED_REFINE", "0", 3)], ids=lambda k: k[0])
@pytest.mark.parametrize("rate,pmf,thr", [(2e6, True, 7.0), (20e6, False, 7.0), (64e6, True, 7.0), (64e6, False, 20.0), (64e6, True, 0.0)], ids=_id)
def test_stream_vectors_other_kernels(hip_knobs_lib, oracle_mod, monkeypatch, capfd, rate, pmf, thr, knob):
    """The same vectors through the rate-generic kernels, the tile front end and the unfused 64 Msps refinement (test build with
    the knobs compiled in)."""
    monkeypatch.setenv(knob[0], knob[1])
    monkeypatch.setenv("AIRMODES_TRACE_SPEC", "1")
    npk, _ = dc.check_streams(hip_knobs_lib, rate, pmf, int(rate / 1e6), thr, want_fe=knob[2] if rate == 64e6 or knob[2] == 1 else None)
    assert npk > 30
    # (the fused refinement names itself on stderr under AIRMODES_TRACE_SPEC in the test builds: it must not have run here)
    assert "am_k_refine_seg" not in capfd.readouterr().err


def test_the_default_path_runs_the_fused_refinement(hip_knobs_lib, oracle_mod, monkeypatch, capfd):
    """The witness the cases above rely on: without a knob the 64 Msps scan goes through am_k_refine_seg and says so."""
    monkeypatch.setenv("AIRMODES_TRACE_SPEC", "1")
    dc.check_streams(hip_knobs_lib, 64e6, False, 64, 20.0, want_fe=3)
    assert "am_k_refine_seg" in capfd.readouterr().err


@pytest.mark.parametrize("pmf", [True, False], ids=_id)
@pytest.mark.parametrize("rate", RATES, ids=_id)
def test_lattice_ties(hip_lib, oracle_mod, rate, pmf):
    assert dc.check_lattice(hip_lib, rate, pmf) > 10


@pytest.mark.parametrize("rate", [2e6, 64e6], ids=_id)
def test_lattice_ties_other_kernels(hip_knobs_lib, oracle_mod, monkeypatch, rate):
    monkeypatch.setenv("AIRMODES_GENERIC", "1")
    assert dc.check_lattice(hip_knobs_lib, rate, True, want_fe=1) > 10
    monkeypatch.delenv("AIRMODES_GENERIC")
    monkeypatch.setenv("AIRMODES_FE", "2")
    assert dc.check_lattice(hip_knobs_lib, rate, False, want_fe=2) > 10


@pytest.mark.parametrize("rate", RATES, ids=_id)
def test_constant_plateaus(hip_lib, oracle_mod, rate):
    assert dc.check_plateaus(hip_lib, rate, 30000 * int(rate / 2e6)) > 10


@pytest.mark.parametrize("rate", [5e6, 6.25e6, 4.8e6], ids=_id)
def test_lattice_fractional_rates(hip_lib, oracle_mod, rate):
    assert dc.check_lattice_cuts(hip_lib, rate, 60000) > 10


@pytest.mark.parametrize("rate", [2e6, 20e6], ids=_id)
def test_lattice_dc_blocker(hip_lib, oracle_mod, rate):
    assert dc.check_lattice_cuts(hip_lib, rate, 30000 * int(rate / 2e6), dcblock=True) > 10
