"""The raw front end at 64 Msps on the MI355X: a stream of sc16 / cs8 / cu8 samples scanned as it is (am_k_fe3<FMT>,
am_k_refine_seg<PMF, FMT>, am_k_extract_slice_iq<32, ..., 1>) gives what the same stream gives when it is widened
first, record for record, and the packets of the oracle on to_cf32(raw) -- on a capture of several am_k_fe3 steps per
workgroup.  CPU twin: tests/test_raw_front_end.py; the checks themselves are in tests/rawfe_common.py."""
import pytest

import formats_common as fc
import rawfe_common as rc

pytestmark = pytest.mark.gpu

KEY = rc.GPU_CAPTURE


def test_native_route_is_taken_only_where_promised(hip_lib):
    assert not hip_lib.emulated
    rc.check_route(hip_lib)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_packets_switch_on_switch_off_and_oracle(hip_lib, oracle_mod, fmt, device):
    rc.check_packets(hip_lib, KEY, fmt, seed=11 + len(fmt), device=device)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_candidate_records_of_the_capture(hip_lib, oracle_mod, fmt):
    rc.check_stage(hip_lib, rc.capture(KEY, fmt)[0], fmt, at_least=1000)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_candidate_records_of_full_range_noise(hip_lib, fmt):
    raw = fc.random_raw(fmt, 400_000, 21)
    assert len(set(raw.tolist())) == 2 ** (8 * raw.itemsize) or fmt == "sc16"       # every component value occurs (8-bit formats)
    # (uniform noise seldom looks like four pulses: a few hundred first-stage candidates in 400 000 samples; a hundred records,
    # each compared field by field, are what makes the comparison worth its name)
    rc.check_stage(hip_lib, raw, fmt, at_least=100)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_bursts_and_tags(hip_lib, oracle_mod, fmt):
    rc.check_extraction(hip_lib, KEY, fmt)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_device_buffer_at_byte_offsets(hip_lib, oracle_mod, fmt):
    rc.check_alignment(hip_lib, KEY, fmt, rc.offsets_of(fmt))


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_short_first_chunks(hip_lib, oracle_mod, fmt):
    rc.check_first_chunk(hip_lib, KEY, fmt, device=True)


def test_decode_options_ride_along(hip_lib, oracle_mod):
    rc.check_options(hip_lib, KEY, seed=5)


def test_format_change_and_switch_change_in_mid_stream(hip_lib, oracle_mod):
    rc.check_changes(hip_lib, KEY)
