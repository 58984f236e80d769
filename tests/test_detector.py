"""Boundary vectors for the preamble detector on the CPU emulation of the kernels (tests/detector_common.py): a sample on
the edge of every rule of lib/preamble_impl.cc:172-216, the census that proves it, then the comparison with the oracle and the
reference's own C++.  The same checks run on the GPU in tests/test_gpu_detector.py; tests/MUTANTS.md lists the one-line kernel
faults these cases were aimed at."""
import numpy as np
import pytest

import detector_common as dc
import oracle
import parity_common as pc
import synth

RATES = (2e6, 4e6, 8e6, 20e6, 64e6)
PLAN = dc.stream_plan(RATES)
_id = dc.case_id


def test_census_restates_the_scan(oracle_mod):
    """The census is only worth something if it is the reference's scan: its hits are the oracle's tags, its candidate
    records the oracle's, on ordinary captures and on lattice ones."""
    for rate, pmf, thr in ((2e6, True, 7.0), (8e6, False, 0.0), (20e6, True, 20.0)):
        spc = int(rate / 2e6)
        for iq in (synth.synth_capture(rate, 20000 * spc, 6000.0, 3)[0], dc.lattice_capture(rate, 20000 * spc, 6000.0, 4)):
            bb, avg = oracle.frontend(iq, spc, pmf)
            assert float(dc.threshold_lin(thr)) == oracle.threshold_lin(thr)
            c = dc.boundary_census(bb, avg, spc, thr, rate)
            _, ot = oracle.preamble_scan(bb, avg, spc, thr, rate)
            assert len(ot) > 3 and [int(s) for s in ot["sample"]] == c["hits"]
            by_e = {k: hl for k0, k, hl, st, ok in c["cands"] if ok}
            assert [by_e[int(s)] for s in ot["sample"]] == [int(h) for h in ot["how_late"]]
            c = dc.boundary_census(bb, avg, spc, thr, rate, greedy=False)
            pos, ref_, val, _ = oracle.candidates(bb, avg, spc, thr, rate=rate)
            assert [x[0] for x in c["cands"]] == pos.tolist() and [x[1] for x in c["cands"]] == ref_.tolist()
            assert [int(x[4]) for x in c["cands"]] == val.tolist()


@pytest.mark.parametrize("thr", [0.0, 7.0, 20.0], ids=_id)
@pytest.mark.parametrize("rate", RATES, ids=_id)
def test_block_vectors(emu_lib, oracle_mod, rate, thr):
    assert dc.check_block(emu_lib, rate, int(rate / 1e6) + int(thr), thr) > 100


@pytest.mark.parametrize("rate,pmf,thr", PLAN, ids=_id)
def test_stream_vectors(emu_lib, oracle_mod, monkeypatch, capfd, rate, pmf, thr):
    monkeypatch.setenv("AIRMODES_TRACE_SPEC", "1")
    npk, iq = dc.check_streams(emu_lib, rate, pmf, int(rate / 1e6), thr)
    assert npk > 30
    # (the fused 64 Msps refinement names itself on stderr under AIRMODES_TRACE_SPEC in the test builds: the witness the
    # unfused cases below rely on)
    assert ("am_k_refine_seg" in capfd.readouterr().err) == (rate == 64e6)
    if rate == 64e6 and pmf and thr == 7.0:
        pc.check_stream_pipe(emu_lib, rate, len(iq), 0.0, 5, thr=thr, pmf=pmf, iq=np.array(iq))


KNOBS = [("AIRMODES_GENERIC", "1", 1), ("AIRMODES_FE", "2", 2), ("AIRMODES_FUSED_REFINE", "0", 3)]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: k[0])
@pytest.mark.parametrize("pmf,thr", [(True, 7.0), (False, 20.0)], ids=_id)
def test_stream_vectors_other_kernels(emu_lib, oracle_mod, monkeypatch, capfd, pmf, thr, knob):
    """64 Msps through the kernels the default path does not run: the rate-generic ones, the tile front end, and the
    unfused refinement behind the streaming front end (am_k_refine_late with chip rows)."""
    monkeypatch.setenv(knob[0], knob[1])
    monkeypatch.setenv("AIRMODES_TRACE_SPEC", "1")
    npk, _ = dc.check_streams(emu_lib, 64e6, pmf, 64, thr, want_fe=knob[2])
    assert npk > 30
    # (the fused refinement names itself on stderr under AIRMODES_TRACE_SPEC in the test builds: it must not have run here)
    assert "am_k_refine_seg" not in capfd.readouterr().err


@pytest.mark.parametrize("pmf", [True, False], ids=_id)
@pytest.mark.parametrize("rate", RATES, ids=_id)
def test_lattice_ties(emu_lib, oracle_mod, rate, pmf):
    assert dc.check_lattice(emu_lib, rate, pmf) > 10


@pytest.mark.parametrize("rate", RATES, ids=_id)
def test_constant_plateaus(emu_lib, oracle_mod, rate):
    assert dc.check_plateaus(emu_lib, rate, 30000 * int(rate / 2e6)) > 10


@pytest.mark.parametrize("rate", [5e6, 6.25e6, 4.8e6], ids=_id)
def test_lattice_fractional_rates(emu_lib, oracle_mod, rate):
    assert dc.check_lattice_cuts(emu_lib, rate, 60000) > 10


@pytest.mark.parametrize("rate", [2e6, 20e6], ids=_id)
def test_lattice_dc_blocker(emu_lib, oracle_mod, rate):
    assert dc.check_lattice_cuts(emu_lib, rate, 30000 * int(rate / 2e6), dcblock=True) > 10
