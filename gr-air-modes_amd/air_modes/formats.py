"""Native SDR sample formats in front of the receive path: raw integer I,Q -> float32 I,Q.

The reference never sees a raw sample: its GNU Radio source blocks (python/radio.py:164-231:
uhd.stream_args(cpu_format="fc32"), osmosdr.source) convert on the host before rx_path.  This package has no such
blocks; the raw pairs go to the GPU as they are and are widened there (csrc/am_resample.hip: am_k_unpack, C ABI
am_unpack / am_process_samples).  This module is the DEFINITION of that stage, operation by operation:

    name   raw element (little-endian, I then Q)   float32 value of a component x
    cf32   float32                                 x
    sc16   int16                                   float32(x) * 2^-15
    cs8    int8                                    float32(x) * 2^-7
    cu8    uint8                                   (float32(x) - 127.5f) * 2^-7

Every operation is exact in float32 -- an integer below 2^16 converted to float, 127.5 subtracted from an integer
below 256 (127.5 is the midpoint of the unsigned range and exactly representable), a scale by a power of two -- so the
result does not depend on rounding mode, contraction or evaluation order, and the kernel is compared with `to_cf32`
bit for bit (as uint32).  The packets of a raw stream are DEFINED as the packets of the float32 stream `to_cf32`
gives.

gr-osmosdr's own offset and scale constants for the 8-bit formats are not part of the reference tree, and no parity
with them is claimed: the detection threshold is relative to the moving average of the same samples, so a common
scale or offset convention only shows in the reference level printed with each message.
"""
import numpy as np

CF32, SC16, CS8, CU8 = 0, 1, 2, 3                      # AM_FMT_* of include/airmodes_hip.h
FORMATS = {"cf32": CF32, "sc16": SC16, "cs8": CS8, "cu8": CU8}
_DTYPE = {"cf32": np.dtype("<f4"), "sc16": np.dtype("<i2"), "cs8": np.dtype("i1"), "cu8": np.dtype("u1")}
_BYTES = {"cf32": 8, "sc16": 4, "cs8": 2, "cu8": 2}
# file suffixes modes_rx recognises (".cs16" is what some recorders call sc16)
SUFFIXES = {".cf32": "cf32", ".cu8": "cu8", ".cs8": "cs8", ".sc16": "sc16", ".cs16": "sc16"}


def _name(fmt):
    if fmt not in FORMATS:
        raise ValueError("unknown sample format %r (one of %s)" % (fmt, ", ".join(sorted(FORMATS))))
    return fmt


def code(fmt):
    """AM_FMT_* value of a format name."""
    return FORMATS[_name(fmt)]


def bytes_per_sample(fmt):
    """Bytes of one complex sample: 8 / 4 / 2 / 2."""
    return _BYTES[_name(fmt)]


def component_dtype(fmt):
    """numpy dtype of one component (I or Q) of the raw stream."""
    return _DTYPE[_name(fmt)]


def format_of(array):
    """The format an array's dtype stands for: int16 / int8 / uint8 / float32 / complex64."""
    dt = np.asarray(array).dtype
    if dt == np.complex64 or dt == np.float32:
        return "cf32"
    for name in ("sc16", "cs8", "cu8"):
        if dt == _DTYPE[name]:
            return name
    raise TypeError("no sample format for dtype %s (int16, int8, uint8, float32 or complex64)" % dt)


def raw_components(raw, fmt=None):
    """`raw` as a flat contiguous array of components, I,Q interleaved (shape (n, 2) or flat in; complex64 as float32)."""
    a = np.ascontiguousarray(raw)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    name = format_of(a)
    if fmt is not None and _name(fmt) != name:
        raise TypeError("dtype %s is not format %s" % (a.dtype, fmt))
    a = a.reshape(-1)
    if a.size % 2:
        raise ValueError("an odd number of components: I,Q pairs are expected")
    return a, name


def to_cf32(raw, fmt=None):
    """The table above in numpy float32 arithmetic: raw components (flat interleaved or shape (n, 2)) -> complex64."""
    a, name = raw_components(raw, fmt)
    if name == "cf32":
        f = a.astype(np.float32, copy=True)
    elif name == "sc16":
        f = a.astype(np.float32) * np.float32(2.0 ** -15)
    elif name == "cs8":
        f = a.astype(np.float32) * np.float32(2.0 ** -7)
    else:
        f = (a.astype(np.float32) - np.float32(127.5)) * np.float32(2.0 ** -7)
    assert f.dtype == np.float32
    return f.view(np.complex64)
