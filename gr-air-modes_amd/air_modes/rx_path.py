"""air_modes.rx_path -- the receive hier block (python/rx_path.py:25-88), MI355X edition.

The reference wires five CPU blocks (complex_to_mag_squared, two moving_average_ff,
preamble, slicer) inside a gr.hier_block2 and lets the GNU Radio scheduler stream through
them.  Here the whole chain is ONE batched GPU sink: work(iq) pushes a chunk of the complex
stream through am_process_iq and posts the resulting messages to the queue.  Constructor
signature, setter/getter names and the message format are the reference's.
"""
import numpy as np

from . import _capi
from .blocks import slicer as _slicer


class rx_path(object):
    def __init__(self, rate, threshold, queue, use_pmf=False, use_dcblock=False, device=-1, lib=None, fix_errors=0,
                 address_gate=0, address_ttl=60.0, address_repair=0, long_formats=0, raw_front_end=None):
        """raw_front_end: None leaves the library's default; 0, 1 or 2 sets the level (Context.set_raw_front_end: 2 = sc16 /
        cs8 / cu8 input is scanned as it is at 2 .. 40 Msps too, not only at 64)."""
        self._rate = int(rate)
        self._threshold = threshold
        self._queue = queue
        self._spc = int(rate / 2e6)
        self._use_pmf = bool(use_pmf)
        self._ctx = _capi.Context(float(self._rate), float(threshold), use_pmf=use_pmf,
                                  use_dcblock=use_dcblock, device=device, lib=lib)
        self._slicer = _slicer(queue, _ctx=self._ctx)
        self.packets = 0
        self.repaired = 0             # ... of them repaired (set_fix_errors, and set_address_repair: both leave reserved[1] != 0)
        self._gate_used = False
        self.gated = 0                # packets the address gate dropped so far (set_address_gate); they are not in `packets`
        self.samples = 0
        # (through this object's own setters: set_address_gate notes that `gated` has to be kept)
        _capi.apply_decode_options(self, fix_errors, address_gate, address_ttl, address_repair, long_formats)
        if raw_front_end is not None:
            if raw_front_end not in (0, 1, 2):
                raise ValueError("raw_front_end: None, 0, 1 or 2")
            self._ctx.set_raw_front_end(int(raw_front_end))

    # --- reference surface: python/rx_path.py:67-87 ---
    def set_rate(self, rate):
        self._ctx.set_rate(float(int(rate)))
        self._rate = int(rate)
        self._spc = int(rate / 2e6)

    def set_threshold(self, threshold):
        self._ctx.set_threshold(float(threshold))
        self._threshold = threshold

    def set_pmf(self, pmf):
        # the reference's setter is a no-op too ("must be done when top block is stopped")
        pass

    def get_pmf(self, pmf=None):
        return self._ctx.get_pmf()

    def get_threshold(self):
        return self._ctx.get_threshold()

    # --- beyond the reference: it drops every DF11 / DF17 reply that fails parity (lib/slicer_impl.cc:179-182) ---
    def set_fix_errors(self, max_bits):
        """Repair replies with up to max_bits (0 = off, 1, 2) wrong bits from the next work() on (am_set_fix_errors)."""
        self._ctx.set_fix_errors(max_bits)

    def get_fix_errors(self):
        return self._ctx.get_fix_errors()

    # --- beyond the reference: it cuts DF18 / DF19 squitters, 112 bits on the air, to 56 (lib/slicer_impl.cc:140) ---
    def set_long_formats(self, formats):
        """From the next work() on, slice DF18 and / or DF19 as 112 bits and check their parity as DF17's (am_set_long_formats):
        an int mask (1 = DF18, 2 = DF19) or an iterable of 18 / 19; 0 = off."""
        self._ctx.set_long_formats(formats)

    def get_long_formats(self):
        return self._ctx.get_long_formats()

    # --- beyond the reference: it believes every address/parity reply, whatever its syndrome (lib/slicer_impl.cc:170-182) ---
    def set_address_gate(self, mode, ttl=60.0):
        """From the next work() on, hand out a DF0/4/5/16/20/21 reply only if a parity-clean DF11 / DF17 reply taught its address
        at most ttl seconds of samples before it; mode 2 also drops every other format but 11 and 17 (am_set_address_gate)."""
        self._ctx.set_address_gate(mode, ttl)
        self._gate_used = self._gate_used or bool(mode)

    def get_address_gate(self):
        return self._ctx.get_address_gate()

    def set_address_repair(self, max_bits):
        """From the next work() on, keep an address/parity reply the gate drops if flipping exactly one of its bits gives it the
        address of an aircraft that is alive (am_set_address_repair; 0 = off, 1).  Inert while the gate is off.  `repaired`
        counts these packets too: it counts reserved[1] != 0."""
        self._ctx.set_address_repair(max_bits)

    def get_address_repair(self):
        return self._ctx.get_address_repair()

    # --- what the scheduler does for the reference: push samples through ---
    def set_rx_time(self, offset, secs, frac):
        """What an "rx_time" stream tag does in the reference (lib/preamble_impl.cc:165-170): item
        `offset` of the stream was received at (secs, frac); later packets are stamped from it."""
        self._ctx.set_rx_time(offset, secs, frac)

    def work(self, iq, flush=False, rx_time=()):
        """Consume a chunk of the stream: complex64 / interleaved float32 (the gr_complex stream), or raw samples in a
        radio's native format -- int16 (sc16), int8 (cs8) or uint8 (cu8) components, I,Q interleaved flat or shape (n, 2);
        the format follows from the dtype (air_modes/formats.py) and the widening runs on the GPU.
        flush=True marks the end of the stream.  rx_time: the (offset, secs, frac) "rx_time" tags that
        fall into this chunk, offsets counted over the whole stream.  Returns the accepted packets
        (structured array) after posting their messages to the queue."""
        for tag in rx_time:
            self._ctx.set_rx_time(*tag)
        a = np.asarray(iq)
        if a.dtype in (np.int16, np.int8, np.uint8):
            pk = self._ctx.process_samples(a, flush=flush)
            return self._account(pk, a.size // 2)
        pk = self._ctx.process_iq(iq, flush=flush)
        return self._account(pk, (a.size // (1 if np.iscomplexobj(iq) else 2)))

    def work_device(self, dev_ptr, n_complex, flush=False, fmt="cf32"):
        """Same with the samples already resident in this GPU's memory (interleaved f32, or raw samples of format fmt)."""
        if fmt == "cf32":
            pk = self._ctx.process_iq_device(dev_ptr, n_complex, flush=flush)
        else:
            pk = self._ctx.process_samples_device(dev_ptr, n_complex, fmt, flush=flush)
        return self._account(pk, n_complex)

    def _account(self, pk, n):
        self._slicer.post(pk)
        self.packets += len(pk)
        self.repaired += int(np.count_nonzero(pk["reserved"][:, 1])) if len(pk) else 0
        if self._gate_used:
            self.gated = self._ctx.address_gate_stats(not_learned=False)["dropped"]
        self.samples += int(n)
        return pk

    def context(self):
        return self._ctx


class rx_path_bank(object):
    """K receivers of one kind on one GPU: what K rx_path instances (python/rx_path.py:25-88) give on K finite captures, from
    ONE scan per call (am_process_multi: the captures lie behind one another in one buffer, zeros between them).  queues: one
    gr.msg_queue per receiver -- receiver j's messages go to queues[j], formatted as its own slicer would (the first message of
    every receiver carries the six significant digits of a fresh ostringstream, lib/slicer_impl.cc:186-192).  Every call is a set
    of WHOLE streams (item counts and time stamps start at 0): the batch form of rx_path.work(capture, flush=True)."""

    def __init__(self, rate, threshold, queues, use_pmf=False, device=-1, lib=None, fix_errors=0, address_gate=0,
                 address_ttl=60.0, address_repair=0, long_formats=0):
        self._ctx = _capi.Context(float(int(rate)), float(threshold), use_pmf=use_pmf, device=device, lib=lib)
        # (every receiver's capture is a stream of its own: a gate map per receiver, and receiver j's replies are searched in
        # receiver j's map only)
        _capi.apply_decode_options(self._ctx, fix_errors, address_gate, address_ttl, address_repair, long_formats)
        self._slicers = [_slicer(q, _ctx=self._ctx) for q in queues]
        self.packets = [0] * len(queues)

    def work(self, captures):
        """captures: K complex64 (or interleaved float32) arrays, one per receiver; returns the K packet arrays."""
        assert len(captures) == len(self._slicers)
        buf, n = self._ctx.multi_pack(captures)
        return self._post(self._ctx.process_multi(buf, n))

    def work_device(self, dev_ptr, lengths):
        """The same with the packed buffer (layout: context().multi_layout(lengths), zeros between the streams) already on the GPU."""
        return self._post(self._ctx.process_multi(None, lengths, device_ptr=dev_ptr))

    def set_address_repair(self, max_bits):
        """As rx_path.set_address_repair, from the next work() on."""
        self._ctx.set_address_repair(max_bits)

    def _post(self, per_stream):
        for j, pk in enumerate(per_stream):
            self._slicers[j].post(pk)
            self.packets[j] += len(pk)
        return per_stream

    def context(self):
        return self._ctx
