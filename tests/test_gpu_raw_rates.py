"""The raw front end at 2 .. 40 Msps on the MI355X: with am_set_raw_front_end at level 2 a stream of sc16 / cs8 / cu8 samples is
scanned as it is (am_k_fe4<SPC, G, NW, FMT>, am_k_extract_slice_iq<SPC, ..., 1>) and gives what the same stream
gives when it is widened first, record for record, and the packets of the oracle on to_cf32(raw).  CPU twin:
tests/test_raw_rates.py; the checks themselves are in tests/rawrates_common.py."""
import pytest

import formats_common as fc
import rawrates_common as rr

pytestmark = pytest.mark.gpu


def test_native_route_is_taken_only_where_promised(hip_lib):
    assert not hip_lib.emulated
    rr.check_route(hip_lib)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.RATES)
def test_packets_level_2_level_1_and_oracle(hip_lib, oracle_mod, msps, fmt, device):
    rr.check_packets(hip_lib, msps, fmt, seed=11 + len(fmt) + msps, device=device)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.RATES)
def test_candidate_records_of_the_capture(hip_lib, oracle_mod, msps, fmt):
    rr.check_stage(hip_lib, msps, rr.capture(msps, fmt)[0], fmt, at_least=400)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.NOISE_RATES)
def test_candidate_records_of_full_range_noise(hip_lib, msps, fmt):
    # (at 2 .. 10 Msps full-range noise gives 9 .. 40 records: too few to be a test)
    rr.check_stage(hip_lib, msps, fc.random_raw(fmt, 400_000, 21), fmt, at_least=50)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.SOME_RATES)
def test_bursts_and_tags(hip_lib, oracle_mod, msps, fmt):
    rr.check_extraction(hip_lib, msps, fmt)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.SOME_RATES)
def test_device_buffer_at_byte_offsets_and_odd_length(hip_lib, oracle_mod, msps, fmt):
    rr.check_alignment(hip_lib, msps, fmt)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.SOME_RATES)
def test_short_first_chunks(hip_lib, oracle_mod, msps, fmt, device):
    rr.check_first_chunk(hip_lib, msps, fmt, device=device)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.SOME_RATES)
def test_streams_shorter_than_a_step(hip_lib, oracle_mod, msps, fmt):
    rr.check_short_streams(hip_lib, msps, fmt)


def test_decode_options_ride_along(hip_lib, oracle_mod):
    rr.check_options(hip_lib, seed=5)


def test_format_change_in_mid_stream(hip_lib, oracle_mod):
    rr.check_changes(hip_lib)
