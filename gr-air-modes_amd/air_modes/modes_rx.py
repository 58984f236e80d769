"""File-source subset of the reference's command-line receiver (apps/modes_rx:32-110,
python/radio.py:90-118,221-234):

    python -m air_modes.modes_rx -s capture.cf32 -r 2e6 [-T 7.0] [--no-pmf] [--fix-errors N] [--address-gate M] [--address-ttl S] [--address-repair N] [--long-formats 18,19] [-l lat,lon] [-n] [--raw]
    python -m air_modes.modes_rx -s rtlsdr.cu8 -r 2.4e6            (-f cu8 when the name does not say it)

Reads a gr_complex file (interleaved little-endian float32 I,Q -- what
blocks.file_source(gr.sizeof_gr_complex, path) reads), pushes it through air_modes.rx_path on
the GPU chunk by chunk, and prints one line per decoded report in the reference's format
(python/msprint.py), or the slicer's raw messages with --raw.

-f / --format: the file holds a radio's native samples instead -- sc16 (USRP, Airspy, most recorders), cs8 (HackRF),
cu8 (RTL-SDR); little-endian I,Q pairs, no header.  The reference's sources widen them on the host
(python/radio.py:164-231); here the raw bytes go through the pinned buffer to the device and are widened there
(air_modes/formats.py is the definition): 2 or 4 times fewer bytes read, pinned and sent over PCIe.

Input slower than 4 Msps is resampled to 4 Msps first, as modes_radio does (python/radio.py:49-53) -- with this
package's own polyphase interpolator (air_modes/resample.py: GNU Radio's taps are not reproducible here, so that
stage is compared by packet recall, not bit for bit); `--no-resample` processes at the rate given, which is what
"through rx_path directly" means for the 2 Msps capture of BASELINE.json configs[0..1].  A raw file (sc16, cs8, cu8) is
resampled from the raw samples: one kernel launch per chunk on the receive path's stream, no float32 copy of the input and
no host wait between the interpolator and the scan (resample.gpu_resampler.work_device_samples).

A reader thread keeps one chunk ahead of the GPU (file read and resampling of chunk k+1 run under the GPU call of
chunk k).  Differences from modes_radio, all of them outside the demodulator: no live sources (UHD / osmocom /
UDP) and no ZeroMQ relay (the parser is called directly).
"""
import argparse
import sys

import numpy as np

from . import formats, resample


def _long_formats(text):
    """'18', '19' or '18,19' -> the formats as a tuple (argparse type of --long-formats)."""
    try:
        formats = tuple(int(t) for t in text.split(",") if t.strip())
    except ValueError:
        raise argparse.ArgumentTypeError("expected 18, 19 or 18,19, not %r" % text)
    if not formats or any(f not in (18, 19) for f in formats):
        raise argparse.ArgumentTypeError("expected 18, 19 or 18,19, not %r" % text)
    return formats


def build_parser():
    ap = argparse.ArgumentParser(prog="modes_rx", description=__doc__.split("\n\n")[0])
    ap.add_argument("-s", "--source", required=True, help="sample file: gr_complex (cf32), or see -f")   # radio.py:94
    ap.add_argument("-f", "--format", choices=["cf32", "sc16", "cs8", "cu8"], default=None,
                    help="sample format of the file [default: by suffix .cu8 .cs8 .sc16 .cs16, else cf32]")
    ap.add_argument("-r", "--rate", type=float, default=4e6, help="sample rate [default=%(default)s]")   # :112
    ap.add_argument("-T", "--threshold", type=float, default=7.0,
                    help="pulse detection threshold above noise in dB [default=%(default)s]")            # :114
    ap.add_argument("-p", "--pmf", action="store_true", default=True, help="use pulse matched filtering")  # :116
    ap.add_argument("--no-pmf", dest="pmf", action="store_false")
    ap.add_argument("-d", "--dcblock", action="store_true", default=False,
                    help="use a DC blocking filter (best for HackRF Jawbreaker)")                         # :118
    ap.add_argument("--fix-errors", type=int, choices=[0, 1, 2], default=0,
                    help="repair DF11 / DF17 replies with up to this many wrong bits (DF17 only for two) instead of "
                    "dropping them as slicer_impl.cc:179-182 does [default=%(default)s]")
    ap.add_argument("--address-gate", type=int, choices=[0, 1, 2], default=0,
                    help="believe a DF0/4/5/16/20/21 reply only if a parity-clean DF11 / DF17 reply was heard from its address "
                    "within --address-ttl (slicer_impl.cc:170-182 checks none of them); 2 also drops reserved formats "
                    "[default=%(default)s]")
    ap.add_argument("--address-ttl", type=float, default=60.0, metavar="SECONDS",
                    help="how long a heard address is believed [default=%(default)s]")
    ap.add_argument("--address-repair", type=int, choices=[0, 1], default=0,
                    help="with --address-gate: keep a reply the gate drops if flipping exactly one of its bits gives it the "
                    "address of an aircraft heard within --address-ttl [default=%(default)s]")
    ap.add_argument("--long-formats", type=_long_formats, default=(), metavar="18,19",
                    help="slice these downlink formats (18: non-transponder extended squitter, 19: military extended "
                    "squitter) as 112 bits and check their parity, instead of cutting them to 56 bits as "
                    "slicer_impl.cc:140 does [default: none]")
    ap.add_argument("--raw-front-end", type=int, choices=[0, 1, 2], default=None,
                    help="sc16 / cs8 / cu8 input scanned as it is, without the float32 copy: 0 = never, 1 = at 64 Msps, "
                    "2 = at 2, 4, 8, 10, 16, 20, 32, 40 and 64 Msps (input below 4 Msps goes through the resampler first, which "
                    "reads the raw samples itself and hands the scan float32, unless --no-resample) [default: the library's, 1]")
    ap.add_argument("-l", "--location", default=None, help="receiver position as lat,lon (enables range/bearing "
                    "and surface positions)")                                                            # modes_rx:40
    ap.add_argument("-n", "--no-print", action="store_true", help="do not print decoded reports")       # modes_rx:45
    ap.add_argument("--raw", action="store_true", help="print the slicer's raw messages instead of parsed reports")
    ap.add_argument("--chunk", type=int, default=1 << 22, help="complex samples per GPU call")
    ap.add_argument("--no-resample", action="store_true", help="process input below 4 Msps at its own rate")
    return ap


def source_format(path, fmt=None):
    """The format of a sample file: the one given, else by the name's suffix, else cf32."""
    if fmt:
        return fmt
    for suffix, name in formats.SUFFIXES.items():
        if path.lower().endswith(suffix):
            return name
    return "cf32"


def main(argv=None, out=None):
    args = build_parser().parse_args(argv)
    out = out or sys.stdout
    fmt = source_format(args.source, args.format)
    from . import cpr_decoder, make_parser, msg_queue, output_print, pubsub, rx_path

    queue = msg_queue()
    rx_rate, resampler = args.rate, None
    if args.rate < 4e6 and not args.no_resample:                      # radio.py:49-53
        # on the GPU, bit-identical to resample.arb_resampler (its definition); the output stays on the device
        rx_rate, resampler = 4e6, resample.gpu_resampler(4e6 / args.rate)
    rx = rx_path(rx_rate, args.threshold, queue, use_pmf=args.pmf, use_dcblock=args.dcblock, fix_errors=args.fix_errors,
                 address_gate=args.address_gate, address_ttl=args.address_ttl,
                 address_repair=args.address_repair, long_formats=args.long_formats,
                 raw_front_end=args.raw_front_end)                   # (below 4 Msps: the window runs at 4 Msps too)
    publisher = pubsub()
    feed = make_parser(publisher, long_formats=args.long_formats)
    my_position = [float(n) for n in args.location.split(",")] if args.location else None
    if not args.no_print and not args.raw:
        output_print(cpr_decoder(my_position), publisher, callback=lambda line: print(line, file=out))
    print("Using file source %s" % args.source, file=sys.stderr)
    print("Rate is %i" % int(args.rate), file=sys.stderr)

    # File -> pinned host buffer -> device, two buffers in flight (python/radio.py:221-234's file source): the reader thread
    # fills one pinned buffer from the file and starts its copy to the device while the GPU still works on the chunk before
    # it; the receive path (and the interpolator in front of it) take device pointers, so a sample crosses PCIe once and
    # never comes back.
    import queue as _queue
    import threading
    from . import _capi
    nslots = 2
    bps = formats.bytes_per_sample(fmt)
    raw = fmt != "cf32"
    # a cf32 file in front of the interpolator carries its drain zeros in the slot; a raw file does not (a raw zero byte is not
    # a zero sample): its last chunk is flushed by the interpolator itself
    drain = resample.TAPS_PER_PHASE if resampler is not None and not raw else 0
    # a slot holds a chunk at its raw width, and nothing else
    up = _capi.Uploader((args.chunk * bps + 7) // 8 + drain, nslots=nslots)
    if raw and resampler is not None:
        # the interpolator reads the raw samples where they lie (one launch, no float32 copy) on the receive path's stream:
        # the scan behind it is ordered by the stream, nothing waits on the host between the two
        resampler.set_stream(rx.context().stream())
    ready = _queue.Queue()                    # (slot, samples, last) in stream order, or an exception
    free = _queue.Queue()
    for k in range(nslots):
        free.put(k)

    def reader():
        try:
            with open(args.source, "rb") as f:
                while True:
                    slot = free.get()
                    buf = up.buffer(slot)
                    want = bps * args.chunk
                    got = f.readinto(memoryview(buf).cast("B")[:want])
                    n = got // bps                                    # whole complex samples
                    last = got < want
                    if raw:
                        up.start_bytes(slot, n * bps)
                    else:
                        if last and drain:
                            # drain: the interpolator holds its last outputs back until it has seen what follows them
                            buf[2 * n:2 * (n + drain)] = 0.0
                            n += drain
                        up.start(slot, n)
                    ready.put((slot, n, last))
                    if last:
                        return
        except Exception as err:                                      # surfaces in the consumer
            ready.put((err, 0, True))

    th = threading.Thread(target=reader, daemon=True)
    th.start()
    while True:
        slot, n, last = ready.get()
        if isinstance(slot, Exception):
            raise slot
        ptr = up.wait(slot)
        if raw and resampler is not None:
            ptr, n = resampler.work_device_samples(ptr, n, fmt, flush=last)   # (python/radio.py:49-53) from the raw samples
            rx.work_device(ptr, n, flush=last)
        else:
            if resampler is not None:
                ptr, n = resampler.work_device_in(ptr, n)             # (python/radio.py:49-53) 2 -> 4 Msps on the GPU
            rx.work_device(ptr, n, flush=last, fmt=fmt)               # (raw samples are widened straight behind the carried tail)
        free.put(slot)                                                # (the call returned: the device is done with the slot)
        while not queue.empty_p():
            text = queue.delete_head().to_string()
            if args.raw:
                if not args.no_print:
                    print(text, file=out)
            else:
                try:
                    feed(text)
                except (IndexError, KeyError, ValueError) as err:
                    # table lookups the reference does unguarded (e.g. emitter category 7 in category
                    # set B, python/parse.py:274-280): there the exception ends the subscriber thread,
                    # here the report is skipped and the receiver keeps going
                    print("skipped %s: %r" % (text.split()[0], err), file=sys.stderr)
        if last:
            break
    th.join()
    up.close()
    if resampler is not None:
        resampler.close()                     # (before the receive path whose stream it may run on)
    print("%d samples, %d packets" % (rx.samples, rx.packets), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
