"""The raw front end at 2 .. 40 Msps on the CPU emulation of the kernels: with am_set_raw_front_end at level 2 a stream of sc16 /
cs8 / cu8 samples is scanned as it is (am_k_fe4<SPC, G, NW, FMT>, am_k_extract_slice_iq<SPC, ..., 1>) and gives
what the same stream gives when it is widened first, record for record, and the packets of the oracle on to_cf32(raw).  The checks
themselves are in tests/rawrates_common.py; tests/test_gpu_raw_rates.py runs them on the GPU over the whole matrix of rates,
formats, byte offsets and chunk lengths.  Here a scan costs 0.4 s at 2 Msps and 9 s at 40 Msps (the whole matrix: 21 minutes), so
every check runs at every rate it is meant for, on all three formats at the rates that are quick to emulate and on one format,
taken in turn, with the fewest offsets and lengths that still reach every path, at the slow ones."""
import pytest

import formats_common as fc
import rawfe_common as rc
import rawrates_common as rr

QUICK = (2, 4, 8, 10)                            # Msps: at most a second per emulated scan of the capture
# the checks of many scans per case: 4 Msps stands in for 40 here (the other rate at which 48 lanes of a wave own a unit, LU = 48;
# 40 Msps itself runs in the packet and candidate checks below, and in every check on the GPU)
SOME_RATES = (2, 4, 10, 20)


def formats_at(msps):
    """All three formats at the quick rates; one at the others, a different one from rate to rate."""
    if msps in QUICK:
        return fc.RAW_FORMATS
    return (fc.RAW_FORMATS[rr.RATES.index(msps) % 3],)


def cases(rates):
    return [pytest.param(m, f, id="%d-%s" % (m, f)) for m in rates for f in formats_at(m)]


def test_native_route_is_taken_only_where_promised(emu_lib):
    rr.check_route(emu_lib)


@pytest.mark.parametrize("msps,fmt", cases(rr.RATES))
def test_packets_level_2_level_1_and_oracle(emu_lib, oracle_mod, msps, fmt):
    rr.check_packets(emu_lib, msps, fmt, seed=11 + len(fmt) + msps, device=False)


@pytest.mark.parametrize("msps,fmt", cases((2, 10)))
def test_packets_from_a_device_buffer(emu_lib, oracle_mod, msps, fmt):
    rr.check_packets(emu_lib, msps, fmt, seed=11 + len(fmt) + msps, device=True)


@pytest.mark.parametrize("msps,fmt", cases(rr.RATES))
def test_candidate_records_of_the_capture(emu_lib, oracle_mod, msps, fmt):
    # (the emulation finds 524 .. 5 707 records on the 24 captures: every rate and format was run once, at_least=400 holds on all)
    rr.check_stage(emu_lib, msps, rr.capture(msps, fmt)[0], fmt, at_least=400)


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.NOISE_RATES)
def test_candidate_records_of_full_range_noise(emu_lib, msps, fmt):
    # (at 2 .. 10 Msps full-range noise gives 9 .. 40 records: too few to be a test)
    rr.check_stage(emu_lib, msps, fc.random_raw(fmt, 400_000, 21), fmt, at_least=50)


@pytest.mark.parametrize("msps,fmt", cases(SOME_RATES))
def test_bursts_and_tags(emu_lib, oracle_mod, msps, fmt):
    rr.check_extraction(emu_lib, msps, fmt)


@pytest.mark.parametrize("msps,fmt", cases(SOME_RATES))
def test_device_buffer_at_byte_offsets_and_odd_length(emu_lib, oracle_mod, msps, fmt):
    if msps in QUICK:
        rr.check_alignment(emu_lib, msps, fmt)
    else:
        # an offset that is no multiple of a sample (8-bit formats) or of a pair, and the odd length from the device
        rr.check_alignment(emu_lib, msps, fmt, offsets=(rc.offsets_of(fmt)[1],), odd_sources=("device",))


@pytest.mark.parametrize("msps,fmt", cases(SOME_RATES))
def test_short_first_chunks(emu_lib, oracle_mod, msps, fmt):
    if msps in QUICK:
        rr.check_first_chunk(emu_lib, msps, fmt, device=False)
        rr.check_first_chunk(emu_lib, msps, fmt, device=True, lengths=rr.first_chunks(msps)[2:4])
    else:
        # one chunk that ends short of the first carried tail, one that makes the next view start at the rounded-down C0
        T = rr.STEP[msps]
        rr.check_first_chunk(emu_lib, msps, fmt, device=False, lengths=(7, T + 1))


@pytest.mark.parametrize("fmt", fc.RAW_FORMATS)
@pytest.mark.parametrize("msps", rr.SOME_RATES)
def test_streams_shorter_than_a_step(emu_lib, oracle_mod, msps, fmt):
    rr.check_short_streams(emu_lib, msps, fmt)


def test_decode_options_ride_along(emu_lib, oracle_mod):
    rr.check_options(emu_lib, seed=5)


def test_format_change_in_mid_stream(emu_lib, oracle_mod):
    rr.check_changes(emu_lib)
