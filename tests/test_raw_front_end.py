"""The raw front end at 64 Msps on the CPU emulation of the kernels: a stream of sc16 / cs8 / cu8 samples scanned as it is
(am_k_fe3<FMT>, am_k_refine_seg<PMF, FMT>, am_k_extract_slice_iq<32, ..., 1>) gives what the same stream gives
when it is widened first, record for record, and the packets of the oracle on to_cf32(raw).  The same checks run on the GPU in
tests/test_gpu_raw_front_end.py; the checks themselves are in tests/rawfe_common.py."""
import pytest

import formats_common as fc
import rawfe_common as rc

KEY = rc.CPU_CAPTURE


def test_native_route_is_taken_only_where_promised(emu_lib):
    rc.check_route(emu_lib)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_packets_switch_on_switch_off_and_oracle(emu_lib, oracle_mod, fmt, device):
    rc.check_packets(emu_lib, KEY, fmt, seed=11 + len(fmt), device=device)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_candidate_records_of_the_capture(emu_lib, oracle_mod, fmt):
    rc.check_stage(emu_lib, rc.capture(KEY, fmt)[0], fmt, at_least=1000)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_candidate_records_of_full_range_noise(emu_lib, fmt):
    raw = fc.random_raw(fmt, 400_000, 21)
    assert len(set(raw.tolist())) == 2 ** (8 * raw.itemsize) or fmt == "sc16"       # every component value occurs (8-bit formats)
    # (uniform noise seldom looks like four pulses: a few hundred first-stage candidates in 400 000 samples; a hundred records,
    # each compared field by field, are what makes the comparison worth its name)
    rc.check_stage(emu_lib, raw, fmt, at_least=100)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_bursts_and_tags(emu_lib, oracle_mod, fmt):
    rc.check_extraction(emu_lib, KEY, fmt)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_device_buffer_at_byte_offsets(emu_lib, oracle_mod, fmt):
    offs = rc.offsets_of(fmt)
    rc.check_alignment(emu_lib, KEY, fmt, (offs[0], offs[1], 8))


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
def test_short_first_chunks(emu_lib, oracle_mod, fmt):
    rc.check_first_chunk(emu_lib, KEY, fmt, device=False)


def test_decode_options_ride_along(emu_lib, oracle_mod):
    rc.check_options(emu_lib, KEY, seed=5)


def test_format_change_and_switch_change_in_mid_stream(emu_lib, oracle_mod):
    rc.check_changes(emu_lib, KEY)
