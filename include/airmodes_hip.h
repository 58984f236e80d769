/*
 * airmodes_hip.h -- C ABI of libairmodes_hip.so, the MI355X (gfx950) implementation of the
 * gr-air-modes receive hot path:  IQ -> |.|^2 -> moving-average threshold -> Mode-S preamble
 * detection -> PPM bit slicing with confidence -> CRC-24 syndrome -> packet list.
 *
 * This header is the drop-in boundary.  Each entry point names the reference interface it
 * replaces (paths relative to the gr-air-modes tree).  Plain pointers and sizes only; no
 * C++ or torch types; no exceptions cross the boundary.  All functions returning int return
 * AM_OK (0) or a negative AM_E* code; am_last_error() gives the text.
 *
 * Threading: a context is NOT thread-safe (one context per stream per GPU, as a GNU Radio
 * block instance is single-threaded inside work()); setters take effect at the next call.
 * Ownership: the caller owns every buffer it passes; the context owns its device buffers
 * and the carry-over stream state and is released by am_destroy().
 */
#ifndef AIRMODES_HIP_H
#define AIRMODES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AM_ABI_VERSION 5

/* Export marker.  The library is built with -fvisibility=hidden: only what carries AM_API leaves the
 * shared object (the role AIR_MODES_API plays in the reference: include/gr_air_modes/api.h:27-31,
 * CMakeLists.txt:65 -- hidden by default, exported by annotation). */
#if defined(_WIN32)
#  define AM_API
#elif defined(__GNUC__) || defined(__clang__)
#  define AM_API __attribute__((visibility("default")))
#else
#  define AM_API
#endif

/* error codes */
#define AM_OK          0
#define AM_EINVAL     (-1)   /* bad argument (null pointer, rate below 2 MHz, ...)           */
#define AM_ENODEV     (-2)   /* no usable HIP device                                        */
#define AM_ENOMEM     (-3)   /* host or device allocation failed                            */
#define AM_EHIP       (-4)   /* a HIP runtime call failed (see am_last_error)               */
#define AM_ECAPACITY  (-5)   /* output did not fit; *n_out holds the required count         */
#define AM_ENOTSUP    (-6)   /* option not implemented (time shards with the address gate)  */

/* flags for the *_work / am_process_iq calls */
#define AM_F_DEVICE_IN  0x1u  /* input pointers are device memory on the context's GPU      */
#define AM_F_FLUSH      0x2u  /* end of stream: examine the tail under the reference's
                                 end-of-buffer rule (preamble_impl.cc:150,212)              */
#define AM_F_DEVICE_OUT 0x4u  /* am_frontend_work only: bb/avg are device pointers          */
#define AM_F_MORE       0x10u /* am_shard_scan / am_shard_scan_async: the stream goes on beyond total_n (= the samples so
                                 far): no end-of-stream rule; the chunk must come with its whole right halo            */
#define AM_F_ZERO_GAPS  0x20u /* am_process_multi: the library writes the zeros between the streams into the caller's buffer  */
#define AM_F_KEEP_TAGS  0x8u  /* am_process_iq / am_submit_iq: also keep what the preamble block hands the slicer for
                                 this call's hits -- 240-float bursts + "preamble_found" tags (lib/preamble_impl.cc:
                                 219-232) -- for am_fetch_tags                                  */

/* One accepted Mode-S reply: what slicer_impl.cc:186-194 serialises into its text message
 * (data, crc, reference_level, timestamp) plus the integer sample count behind the
 * timestamp.  56 bytes, little endian, natural alignment.
 * Replaces: struct modes_packet (include/gr_air_modes/types.h:29-40). */
typedef struct am_packet {
    uint8_t  data[14];     /* payload bits, MSB first; bytes beyond nbytes are zero        */
    uint8_t  nbytes;       /* 7 = short (56 bit), 14 = long (112 bit)                      */
    uint8_t  df;           /* downlink format = data[0] >> 3  (modes_packet.message_type)  */
    uint8_t  numlowconf;   /* number of low-confidence bits, saturating at 24              */
    uint8_t  reserved[3];  /* [1]: bits flipped by the opt-in repair (am_set_fix_errors): 0 = as sliced, 1 or 2; then */
                           /* data holds the repaired bits and crc is 0.  [0], [2]: zero                           */
    uint32_t crc;          /* 24-bit syndrome: crc(data[0..nbytes-3)) ^ last 3 bytes       */
    float    ref;          /* reference_level (mean of the four preamble chips)            */
    uint32_t reserved2;
    uint64_t sample;       /* preamble item count: stream index + 2*spc - 1                */
    uint64_t secs;         /* sample / rate                (tag_to_timestamp, :124)        */
    double   frac;         /* (sample % rate) / rate       (tag_to_timestamp, :125); both   */
                           /* relative to the rx_time tag in force (am_set_rx_time)         */
} am_packet;

/* One preamble hit: the "preamble_found" stream tag (preamble_impl.cc:224-232) whose value
 * is the (uint64 secs, double frac) tuple, attached to sample 0 of a 240-float burst. */
typedef struct am_tag {
    uint64_t sample;
    uint64_t secs;
    double   frac;
    float    inavg;        /* reference level subtracted from the burst (:220)             */
    uint32_t how_late;     /* late-peak shifts applied (:184-192)                          */
} am_tag;

typedef struct am_ctx am_ctx;

AM_API uint32_t am_abi_version(void);

/* ---- context = the rx_path hier block ------------------------------------------------
 * Replaces: rx_path.__init__(rate, threshold, queue, use_pmf, use_dcblock)
 *           (python/rx_path.py:27-65) and the two block factories
 *           gr::air_modes::preamble::make(float channel_rate, float threshold_db)
 *           (include/gr_air_modes/preamble.h:39), gr::air_modes::slicer::make(queue)
 *           (include/gr_air_modes/slicer.h:41).
 * rate: samples per second, a whole number >= 2e6.  It need not be a multiple of 2 MHz: the reference keeps
 * d_samples_per_chip = channel_rate / 2e6 as a FLOAT and truncates every product with int() (lib/preamble_impl.cc:57,150,
 * 158-162,185,192,205-208,212,220,237), the flowgraph in front of it runs its moving averages at int(rate / 2e6) samples per
 * chip (python/rx_path.py:35) -- e.g. 5 Msps is 2.5 samples per chip for the preamble block and 2 for the filters.  That
 * geometry is reproduced as it is (pinned against the reference's own C++).  Multiples of 2 MHz up to 64 Msps (and 40) run the
 * specialised kernels, everything else the rate-generic ones.
 * use_dcblock != 0 puts filter.dc_blocker_cc(100*spc, False) in front of the path
 * (python/rx_path.py:39-41; default off, python/radio.py:118): two cascaded 100-chip moving
 * averages subtracted from the input delayed by 100*spc - 1 samples -- so, as in the reference,
 * every timestamp is later by that delay.  GNU Radio's gr-filter source is not part of the
 * reference tree (parity unpinned): the window sums use the canonical order of DESIGN.md section 3.
 * device < 0 selects the current HIP device.  Returns NULL on failure; *err (optional)
 * receives the code. */
AM_API am_ctx *am_create(int device, double rate, float threshold_db, int use_pmf, int use_dcblock,
                  int *err);
AM_API void am_destroy(am_ctx *ctx);

/* Replaces: preamble::set_rate / set_threshold / get_rate / get_threshold
 *           (include/gr_air_modes/preamble.h:41-44; lib/preamble_impl.cc:56-76) and
 *           rx_path.set_rate / set_threshold / get_threshold / get_pmf (rx_path.py:67-87).
 * am_set_rate also drops the carried stream state (window lengths change). */
AM_API int    am_set_rate(am_ctx *ctx, double rate);
AM_API int    am_set_threshold(am_ctx *ctx, float threshold_db);
/* Replaces: the "rx_time" stream tag a live source (UHD, osmosdr) attaches to the sample stream and
 *           preamble_impl::general_work latches (lib/preamble_impl.cc:165-170); tag_to_timestamp
 *           (lib/preamble_impl.cc:100-137) then stamps each preamble with
 *           (secs, frac) + (item - offset) / rate.
 * offset is the tag's item offset in the input stream (tags pass the front-end blocks 1:1), counted
 * from the first sample after am_create / am_reset / am_set_rate.  Call it before the am_process_iq
 * (am_preamble_work, am_shard_scan) call whose samples the tag belongs to, with non-decreasing offsets
 * (AM_EINVAL otherwise; a second tag at the same offset replaces the first, as .back() does).  The tag
 * is in force for every preamble whose item count (am_packet.sample) is >= offset, until the next tag;
 * before any tag the reference's default applies (offset 0, time 0: a file source).  In the reference a
 * tag is latched as soon as the scheduler's current window contains it, i.e. up to a buffer early
 * (the unsigned difference :124 then wraps for preambles in front of it); that scheduler-dependent
 * early latch is not reproduced.  am_reset and am_set_rate drop the pending tags. */
AM_API int    am_set_rx_time(am_ctx *ctx, uint64_t offset, uint64_t secs, double frac);
AM_API double am_get_rate(const am_ctx *ctx);
AM_API float  am_get_threshold(const am_ctx *ctx);
AM_API int    am_get_pmf(const am_ctx *ctx);
/* ---- opt-in repair of DF11 / DF17 replies with one or two wrong bits -------------------------------------------------
 * Replaces: the drop at lib/slicer_impl.cc:179-182 ("we forget about them") and puts to use what modes_packet's
 *           lowconfbits[24] / numlowconf were declared for, "for error correction" (include/gr_air_modes/types.h:29-40;
 *           filled at slicer_impl.cc:157, never read): the reference meant to repair such replies and never did.
 * max_bits = 0 (default): the reference's behaviour -- every packet, message text and kernel is what it is without this call.
 * max_bits = 1, 2: a burst is sliced as always (reference level, length from the first five bits, decisions, low-confidence
 * count, the all-zero test, the two low-confidence drops :162-171, syndrome S :173-177).  Only where :182 drops it -- S != 0
 * and DF 11 or 17 -- with syn(j) = x^(nbits-1-j) mod G the syndrome of a wrong bit j, candidates j = 5 .. nbits-1 (the five DF
 * bits are never touched: format and length stay what the slicer chose):
 *   1. DF11 and DF17: if some a has syn(a) == S, bit a is flipped;
 *   2. otherwise, max_bits == 2 and DF17 only: if some a < b have syn(a) ^ syn(b) == S, both are flipped;
 *   3. otherwise the packet is dropped as before.
 * For 56 and for 112 bits all one-bit and two-bit syndromes are distinct and non-zero and no three-bit pattern shares one, so
 * the repair is unique when it exists and three wrong bits are never turned into another frame (tests/test_fix_errors.py).
 * A repaired packet is handed out like any other: data = the repaired bits, crc = 0, reserved[1] = bits flipped (1 or 2),
 * nbytes, df, numlowconf, ref, sample, secs, frac as the slicer formed them before the repair; am_format_message makes
 * "<repaired hex> 000000 <level> <secs> <frac>" of it.  Pinned to the reference: its own slicer, given the burst with the two
 * chips of every repaired bit exchanged (slicer_impl.cc:74-98: the decision flips, the confidence stays), emits that packet.
 * Known and accepted: a DF11 reply to an all-call with interrogator code 1, 2, 4, ..., 64 carries the code as its syndrome,
 * which is also that of one wrong bit among the last seven parity bits: with the repair on it comes out with crc 0 (address
 * intact, interrogator code lost).
 * The setting belongs to the context, survives am_reset and am_set_rate, takes effect with the next call and covers every
 * call that slices (am_process_iq / am_process_samples, am_submit_iq, am_process_multi / am_submit_multi, am_slicer_work,
 * the am_shard_resolve* calls).  AM_EINVAL for max_bits outside 0..2. */
AM_API int    am_set_fix_errors(am_ctx *ctx, int max_bits);
AM_API int    am_get_fix_errors(const am_ctx *ctx);
/* ---- opt-in address gate for address/parity replies (DF0/4/5/16/20/21) ------------------------------------------------
 * Replaces: lib/slicer_impl.cc:170-182, which checks parity for DF11 and DF17 only.  In every other format the 24 parity
 *           bits are overlaid with the aircraft's address, so the syndrome handed on as "ecc" IS the address and any bit
 *           pattern passes (:170 filters only the short ones by confidence): a false preamble whose first five bits slice to
 *           16, 20 or 21 becomes a fictitious aircraft, a real reply with one wrong bit a reply of the wrong aircraft.
 * mode = 0 (default): the reference's behaviour -- every packet, message text and kernel is what it is without this call.
 * mode = 1, 2: the packets of a stream are formed exactly as always (all drops of :162-182, the repair if it is on).  Then, in
 * stream order, with a map last[address] -> item count that is empty when a stream starts, for a packet p at item count
 * s = p.sample and ttl_samples = max(1, (uint64)(ttl_seconds * rate)):
 *   1. teach:  p.df is 11 or 17, p.crc == 0 and p.reserved[1] == 0 (as sliced, not repaired):
 *              last[data[1..3], big-endian] = s.  The packet is kept.  (A repaired DF11 / DF17 packet is kept and teaches nothing.)
 *   2. test:   p.df in {0, 4, 5, 16, 20, 21}: kept iff last[p.crc] exists and s - last[p.crc] <= ttl_samples.  A kept reply does
 *              not teach: noise must not be able to keep itself alive.
 *   3. others: DF1-3, 6-10, 12-15, 18, 19, 22-31 (reserved formats, and 18 / 19 / 24.., which are long on the air but which
 *              :140 slices as 56 bits): mode 1 keeps them, mode 2 drops them.
 * A dropped packet is simply not handed out; a kept one is byte for byte what it is with the gate off.  Item counts are used,
 * not secs / frac: "rx_time" tags do not move the window.  The result does not depend on how the stream is cut into calls,
 * and the packets with the gate on are a subsequence of those with it off (tests/gate_common.py restates this in numpy).
 * am_reset, am_set_rate and AM_F_FLUSH empty the map (item counts restart); the setting survives them.  A new mode or ttl takes
 * effect with the next call and keeps the map.  The map holds 196 608 addresses; one that does not fit is not learned (the gate
 * fails closed) and not_learned counts it.  Only parity-clean replies teach: noise enters at 2^-24 per false DF11 / DF17.
 * Covered: am_process_iq / am_process_samples (any chunking, AM_F_DEVICE_IN or not, AM_ECAPACITY + am_fetch_packets),
 * am_submit_iq / am_collect and am_pipe_* (every batch is a whole stream with a map of its own), am_process_multi /
 * am_submit_multi / am_pipe_submit_multi (stream j of the K has a map of its own), am_slicer_work (the block alone: bursts in
 * ascending item counts; the context's map carries over from call to call until am_reset).  am_fetch_tags / am_last_num_tags
 * are about preamble hits and do not change.  am_spipe_* (one stream, chunks in flight: the map is the pipe's) through
 * am_spipe_set_address_gate below.
 * NOT covered: the time shards (the map would have to cross ranks): with the gate on, am_shard_scan* / am_shard_resolve*
 * return AM_ENOTSUP.
 * AM_EINVAL: mode outside 0..2, ttl_seconds not finite or <= 0.
 * Stats: since am_create, over all streams, of scans the library accepted (a speculative scan that had to be repeated counts
 * once): replies that taught, address/parity replies kept, packets dropped by the gate, addresses not learned.  Any pointer
 * may be null; asking for not_learned waits for the context's stream. */
AM_API int    am_set_address_gate(am_ctx *ctx, int mode, double ttl_seconds);
AM_API int    am_get_address_gate(const am_ctx *ctx, int *mode, double *ttl_seconds);
AM_API int    am_get_address_gate_stats(const am_ctx *ctx, uint64_t *taught, uint64_t *passed, uint64_t *dropped,
                                        uint64_t *not_learned);
/* ---- opt-in repair of one wrong bit in an address/parity reply, from the addresses the gate has learned ----------------
 * Replaces: nothing in the reference, which checks no parity here (lib/slicer_impl.cc:170-182).  The gate above drops "a real
 *           reply with one wrong bit", because it reads as a reply of another aircraft; the gate also holds what recovers it.
 * max_bits = 0 (default): the gate as it is above -- every packet, message text and kernel launch is what it is without this call.
 * max_bits = 1: the packets of a stream are formed and gated exactly as above.  Repair is considered only for a packet p with
 * p.df in {0, 4, 5, 16, 20, 21} that step 2 of the gate drops, while the gate is on (mode 1 or 2).  For such a packet, with
 * nbits = 8 * nbytes and syn(j) = x^(nbits-1-j) mod G the syndrome of a wrong bit j (the table the slicer and am_set_fix_errors
 * use; for j in the last 24 bits it is the single bit 1 << (nbits-1-j)):
 *   the candidates are j = 5 .. nbits-1 with A_j = p.crc ^ syn(j)   (for an address/parity reply of aircraft A with bit j
 *   wrong the syndrome is A ^ syn(j));
 *   A_j is live if last[A_j] exists and s - last[A_j] <= ttl_samples: the map and the window rule the gate's own test sees at p;
 *   exactly one live j:  the packet is kept -- bit j of data flipped, crc = A_j, reserved[1] = 1, every other field as sliced;
 *                        am_format_message makes "<repaired hex> <A_j as %06x> <level> <secs> <frac>" of it;
 *   no live j, or more than one: the packet is dropped as above; the second case is counted as `ambiguous`.
 * The five DF bits are never touched: format, length and the extraction shortcut stay what the slicer chose.  A repaired reply
 * does not teach (neither does a repaired DF11 / DF17 reply).  With max_bits 0, with the gate off, and for every packet the gate
 * keeps, nothing changes; the packets with the repair off are a subsequence of those with it on, up to the repaired ones; the
 * result does not depend on how the stream is cut into calls (tests/aprepair_common.py restates this in numpy).  Pinned to the
 * reference: its own slicer, given the burst with the two chips of bit j exchanged, emits the repaired packet with crc = A_j.
 * KNOWN LIMIT: a frame nobody transmitted finds a live address with probability about (nbits - 5) * fleet / 2^24 per dropped
 * address/parity packet -- 2.6e-4 for 40 aircraft alive and a long reply, one in six for 25 000 -- so the repair is useless near
 * the map's capacity.  Nothing guards against it: the setting is for a receiver that hears a modest fleet.
 * The setting belongs to the context, survives am_reset and am_set_rate, takes effect with the next call and is inert while the
 * gate is off.  Covered: what the gate covers (am_spipe_*: am_spipe_set_address_repair).  NOT covered: the time shards, as for
 * the gate.
 * AM_EINVAL for max_bits outside 0..1.
 * Stats: since am_create, of scans the library accepted: packets repaired, packets dropped as ambiguous.  The gate's `dropped`
 * does not include a repaired packet; `passed` keeps its meaning (kept by step 2 as sliced).  Either pointer may be null. */
AM_API int    am_set_address_repair(am_ctx *ctx, int max_bits);
AM_API int    am_get_address_repair(const am_ctx *ctx);
AM_API int    am_get_address_repair_stats(const am_ctx *ctx, uint64_t *repaired, uint64_t *ambiguous);
/* ---- opt-in 112-bit slicing and parity check for DF18 / DF19 squitters ------------------------------------------------
 * Replaces: lib/slicer_impl.cc:140, which takes a reply for long iff its first five bits read 16, 17, 20 or 21.  DF18 (the
 *           extended squitter of everything that is not a transponder: TIS-B, ADS-R, ground vehicles, obstacles) and DF19 (the
 *           military extended squitter) are 112 bits on the air; the reference cuts them to 56, and what is left usually dies
 *           at :170 or prints "No handler for message type 18".
 * mask = 0 (default): the reference's behaviour -- every packet, message text and kernel is what it is without this call.
 * mask = OR of AM_LF_DF18, AM_LF_DF19: with E the enabled formats and hdr the five header bits as sliced (:135-139),
 *   length:  long iff hdr is 16, 17, 20, 21 or in E.  Everything from :142 to :171 runs with that length: all 112 decisions are
 *            taken, the low-confidence count runs over 112 bits, and :170 (short packets only) does not apply to a format in E.
 *   parity:  (:182) the packet is dropped if the syndrome is non-zero and DF is 11, 17 or in E: DF18 and DF19 carry a plain PI
 *            field like DF17.  A DF19 whose application field uses another parity FAILS CLOSED: it is dropped, not handed out
 *            unchecked.
 *   repair:  with am_set_fix_errors a format in E gets exactly what DF17 gets -- one bit, and two bits at max_bits = 2, candidates
 *            5..111, the DF bits never touched.
 *   gate:    a kept packet of a format in E takes no part in the address gate: it is kept in mode 1 and in mode 2, teaches
 *            nothing (non-transponders send no address/parity replies, and TIS-B addresses need not be ICAO) and is not
 *            tested -- the class a repaired DF17 has.  A format not in E stays with the "others" of step 3 there.  The address
 *            repair is unaffected.
 *   packet:  nbytes = 14, df = 18 or 19, crc = 0; reserved[1] as for DF17.
 * The preamble scan does not depend on any of this (it skips 240 chips after a hit whatever the length): hits, tags and
 * am_fetch_tags are unchanged, and the packets of every format outside E are byte for byte what they are with mask 0
 * (tests/longfmt_common.py restates the definition in numpy).
 * The setting belongs to the context, survives am_reset and am_set_rate, takes effect with the next call and covers every call
 * that slices (the list at am_set_fix_errors, the am_shard_resolve* calls included).  AM_EINVAL for a mask outside 0..3. */
#define AM_LF_DF18 1
#define AM_LF_DF19 2
AM_API int    am_set_long_formats(am_ctx *ctx, int mask);
AM_API int    am_get_long_formats(const am_ctx *ctx);
/* ---- batches in flight ---------------------------------------------------------------------------------------
 * Under GNU Radio every block of rx_path runs in its own thread, so the slicer works on burst k while the preamble
 * block scans ahead (thread-per-block scheduler; python/rx_path.py wires five blocks).  The counterpart here: the
 * launch-latency-bound tail of one batch (greedy chain, extraction, slicer) overlaps the streaming front end of the
 * next.  A context works on one batch at a time, so the overlap is between contexts:
 *
 * am_submit_iq   first half of am_process_iq: copies and kernels of one INDEPENDENT batch (AM_F_FLUSH is required: it
 *                is a whole stream) are enqueued, nothing is waited for.  The samples must stay valid until am_collect.
 * am_collect     second half: waits for the batch, returns its packets (same contract as am_process_iq, incl.
 *                AM_ECAPACITY + am_fetch_packets) and resets the stream state.
 * am_pipe_*      `depth` contexts behind one handle, used round-robin by ONE host thread: submit up to `depth`
 *                batches, collect them in submission order.  Results are those of am_process_iq on each batch. */
AM_API int am_submit_iq(am_ctx *ctx, const float *iq, uint64_t n_complex, uint32_t flags);
AM_API int am_collect(am_ctx *ctx, am_packet *out, uint64_t cap, uint64_t *n_out);
typedef struct am_pipe am_pipe;
AM_API am_pipe *am_pipe_create(int device, double rate, float threshold_db, int use_pmf, int use_dcblock, int depth, int *err);
AM_API void am_pipe_destroy(am_pipe *pipe);
AM_API int am_pipe_depth(const am_pipe *pipe);
AM_API int am_pipe_in_flight(const am_pipe *pipe);
/* AM_ECAPACITY when `depth` batches are already in flight (collect one first) */
AM_API int am_pipe_submit(am_pipe *pipe, const float *iq, uint64_t n_complex, uint32_t flags);
/* packets of the OLDEST batch in flight; AM_EINVAL when there is none */
AM_API int am_pipe_collect(am_pipe *pipe, am_packet *out, uint64_t cap, uint64_t *n_out);
/* K whole streams in ONE scan of the next free context (am_submit_multi's arguments); am_pipe_collect hands the packets out stream by
 * stream, am_pipe_multi_counts the number each stream of the scan collected LAST got.  (rx_path.py:35: one receiver chain per
 * stream -- here eight of them share a scan, and several scans are in flight behind one handle.) */
AM_API int am_pipe_submit_multi(am_pipe *pipe, float *iq, uint32_t k, const uint64_t *n_complex, uint32_t flags);
AM_API int am_pipe_multi_counts(am_pipe *pipe, uint64_t *count, uint32_t k);
AM_API const char *am_pipe_last_error(const am_pipe *pipe);
AM_API float am_pipe_last_kernel_ms(const am_pipe *pipe);   /* dominant-kernel time of the batch collected last */
/* Replaces: lib/slicer_impl.cc:179-182 / include/gr_air_modes/types.h:29-40 as am_set_fix_errors, for every context behind
 * the handle.  AM_EINVAL while batches are in flight (a batch may be sliced again when it is collected). */
AM_API int am_pipe_set_fix_errors(am_pipe *pipe, int max_bits);
AM_API int am_pipe_get_fix_errors(const am_pipe *pipe);
/* Replaces: lib/slicer_impl.cc:170-182 as am_set_address_gate, for every context behind the handle (every batch is a whole
 * stream: its own empty map).  AM_EINVAL while batches are in flight, and for what am_set_address_gate refuses. */
AM_API int am_pipe_set_address_gate(am_pipe *pipe, int mode, double ttl_seconds);
AM_API int am_pipe_get_address_gate(const am_pipe *pipe, int *mode, double *ttl_seconds);
/* am_set_address_repair for every context behind the handle.  AM_EINVAL while batches are in flight, and for max_bits
 * outside 0..1. */
AM_API int am_pipe_set_address_repair(am_pipe *pipe, int max_bits);
AM_API int am_pipe_get_address_repair(const am_pipe *pipe);
/* Replaces: lib/slicer_impl.cc:140 as am_set_long_formats, for every context behind the handle.  AM_EINVAL while batches are
 * in flight, and for a mask outside 0..3. */
AM_API int am_pipe_set_long_formats(am_pipe *pipe, int mask);
AM_API int am_pipe_get_long_formats(const am_pipe *pipe);

/* ---- ONE continuing stream with several of its chunks in flight ---------------------------------------------------
 * The reference's preamble block is a streaming block: general_work() resumes where the last call stopped (lib/preamble_impl.cc:
 * 139-246; consume_each at :213,237,244).  am_process_iq is that, one chunk at a time.  am_spipe_* keeps `depth` consecutive
 * chunks of ONE stream in flight on one GPU: a chunk's scan (everything that does not depend on where the greedy scan enters the
 * chunk) is enqueued when it is submitted, on a context and stream of its own; the position at which the scan enters it travels on
 * the device, from the word the chunk before it leaves it in -- nothing between two chunks waits for the host.  The packets of all
 * chunks, concatenated in submission order, are those of one am_process_iq over the whole stream (item counts and time stamps keep
 * counting).
 *   am_spipe_front   samples of the stream that must lie IN FRONT of every chunk but the first, in the same allocation (the tail of
 *                    the chunk before it: reference-level history + the positions it takes over).  Where the stream is not
 *                    contiguous in memory the library copies them there from the chunk submitted before (device to device, on the
 *                    chunk's stream): a chunk buffer needs that much writable room in front of it.
 *   am_spipe_submit  iq: DEVICE pointer to the chunk's n_complex samples (n_complex > front); they, and the chunk submitted before
 *                    it, must stay valid until the chunk has been collected.  AM_F_FLUSH: the stream's last chunk (end-of-stream
 *                    rule); the next stream starts once every chunk has been collected.  AM_ECAPACITY: `depth` chunks in flight.
 *   am_spipe_collect the packets of the oldest chunk in flight.
 *   am_spipe_redone  chunks that had to take the synchronous path (exit table larger than its message, more candidates than the
 *                    capacity the scan was launched for): results are the same, the chunks behind such a chunk are scanned twice.
 *   am_spipe_set_rx_time  as am_set_rx_time (stream-absolute offsets), with no chunk in flight. */
typedef struct am_spipe am_spipe;
AM_API am_spipe *am_spipe_create(int device, double rate, float threshold_db, int use_pmf, int use_dcblock, int depth, int *err);
AM_API void am_spipe_destroy(am_spipe *pipe);
AM_API int am_spipe_depth(const am_spipe *pipe);
AM_API int am_spipe_in_flight(const am_spipe *pipe);
AM_API int am_spipe_front(const am_spipe *pipe, uint64_t *front);
AM_API int am_spipe_set_rx_time(am_spipe *pipe, uint64_t offset, uint64_t secs, double frac);
AM_API int am_spipe_submit(am_spipe *pipe, const float *iq, uint64_t n_complex, uint32_t flags);
AM_API int am_spipe_collect(am_spipe *pipe, am_packet *out, uint64_t cap, uint64_t *n_out);
AM_API uint64_t am_spipe_redone(const am_spipe *pipe);
AM_API const char *am_spipe_last_error(const am_spipe *pipe);
AM_API float am_spipe_last_kernel_ms(const am_spipe *pipe);   /* dominant-kernel time of the chunk collected last */
/* Replaces: lib/slicer_impl.cc:179-182 / include/gr_air_modes/types.h:29-40 as am_set_fix_errors, for the whole stream.
 * AM_EINVAL while chunks are in flight (as am_spipe_set_rx_time). */
AM_API int am_spipe_set_fix_errors(am_spipe *pipe, int max_bits);
AM_API int am_spipe_get_fix_errors(const am_spipe *pipe);
/* Replaces: lib/slicer_impl.cc:140 as am_set_long_formats, for the whole stream.  AM_EINVAL while chunks are in flight, and
 * for a mask outside 0..3. */
AM_API int am_spipe_set_long_formats(am_spipe *pipe, int mask);
AM_API int am_spipe_get_long_formats(const am_spipe *pipe);
/* Replaces: lib/slicer_impl.cc:170-182 as am_set_address_gate, for the pipe's ONE stream.  The packets of all chunks,
 * concatenated in submission order, are those the pipe hands out with the gate off, filtered by the definition at
 * am_set_address_gate (steps 1-3): whatever the chunk sizes, the depth, the memory layout, and whether a chunk had to be redone
 * (am_spipe_redone) -- a redone chunk and the chunks submitted again behind it teach and count nothing from the attempt that was
 * thrown away.  One stream, one map: it belongs to the pipe, is empty when a stream starts (first chunk after create, or after
 * the AM_F_FLUSH chunk of the stream before has been collected), and item counts are the stream's.  A new mode or ttl keeps the
 * map.  With mode 0 (default) the pipe allocates nothing for the gate and launches what it launches without it.
 * AM_EINVAL: what am_set_address_gate refuses, and while chunks are in flight.
 * Stats: since am_spipe_create, of the chunks collected (an AM_ECAPACITY from am_spipe_collect leaves the packets behind;
 * collecting them later counts nothing twice).  Any pointer may be null; asking for not_learned waits for the pipe's streams. */
AM_API int am_spipe_set_address_gate(am_spipe *pipe, int mode, double ttl_seconds);
AM_API int am_spipe_get_address_gate(const am_spipe *pipe, int *mode, double *ttl_seconds);
AM_API int am_spipe_get_address_gate_stats(const am_spipe *pipe, uint64_t *taught, uint64_t *passed, uint64_t *dropped,
                                           uint64_t *not_learned);
/* Replaces: nothing in the reference (lib/slicer_impl.cc:170-182 checks no parity here), as am_set_address_repair, for the
 * pipe's stream and against the pipe's map; inert while the gate is off, and then nothing more is launched than the gate needs.
 * AM_EINVAL for max_bits outside 0..1, and while chunks are in flight.  Stats as above: packets repaired, dropped as ambiguous. */
AM_API int am_spipe_set_address_repair(am_spipe *pipe, int max_bits);
AM_API int am_spipe_get_address_repair(const am_spipe *pipe);
AM_API int am_spipe_get_address_repair_stats(const am_spipe *pipe, uint64_t *repaired, uint64_t *ambiguous);

/* Run the context's device work on the caller's HIP stream (hipStream_t passed as a pointer; NULL: back to the
 * context's own stream).  For callers whose input is produced on a stream of their own -- e.g. halo samples that
 * arrive by an RCCL receive on a PyTorch stream: work enqueued here is then ordered behind it without a host
 * synchronisation.  The stream must outlive the context or be replaced before it is destroyed.  (No counterpart in
 * the reference: GNU Radio blocks have no device streams.) */
AM_API int am_set_stream(am_ctx *ctx, void *hip_stream);
/* The stream the context's device work runs on now (its own, or the one am_set_stream gave it), as a hipStream_t: for
 * stages that feed the context and want to be ordered in front of it without an event, e.g. am_resampler_set_stream.
 * NULL on a null context. */
AM_API void *am_get_stream(const am_ctx *ctx);
/* Order the context's stream behind everything enqueued so far on another stream of the same device (NULL = the legacy
 * default stream, PyTorch's current stream unless the caller changed it): an event recorded there and waited for here,
 * the host does not block.  For inputs another stream produces -- e.g. boundary samples an RCCL receive is still
 * writing (air_modes/sharded.py). */
AM_API int am_wait_for_stream(am_ctx *ctx, void *hip_stream);

/* start a new stream: sample counter, carry-over samples and greedy-scan state are cleared */
AM_API int    am_reset(am_ctx *ctx);

/* ---- the fused hot path ---------------------------------------------------------------
 * Replaces, for one chunk of the input stream, everything rx_path wires together
 * (python/rx_path.py:38-65): complex_to_mag_squared -> moving_average_ff(spc) ->
 * moving_average_ff(48*spc) -> preamble::general_work (lib/preamble_impl.cc:139-246) ->
 * slicer::work (lib/slicer_impl.cc:102-198) -> modes_check_crc (lib/modes_crc.cc:55-63).
 *
 * iq: n_complex interleaved (I,Q) float32 pairs = what blocks.file_source(gr_complex)
 * delivers (python/radio.py:231); host memory, or device memory with AM_F_DEVICE_IN.
 * Chunks may have any length; results do not depend on how the stream is chunked.
 * Decisions that need look-ahead are deferred to a later call; AM_F_FLUSH ends the stream.
 * out/cap: caller's packet array (host).  *n_out = packets produced by this call, in
 * stream order.  AM_ECAPACITY if cap is too small (nothing is lost: call
 * am_fetch_packets with a larger array). */
AM_API int am_process_iq(am_ctx *ctx, const float *iq, uint64_t n_complex, uint32_t flags,
                  am_packet *out, uint64_t cap, uint64_t *n_out);
AM_API int am_fetch_packets(am_ctx *ctx, am_packet *out, uint64_t cap, uint64_t *n_out);

/* K independent streams in ONE scan (many receivers / channels on one GPU: at 2 and 20 Msps one second of one receiver is too
 * small a job for the chip, the scan's launches are what it costs).  Every stream is a WHOLE stream, as am_process_iq(...,
 * AM_F_FLUSH) takes it -- rx_path.work over one finite capture (python/rx_path.py:27-65) -- and gets exactly the packets that call
 * gives (bit for bit; item counts and time stamps are the stream's own, from its item 0).
 * am_multi_layout   where the streams go in the ONE buffer the scan reads: offset[j] (in complex samples) for stream j of n[j]
 *                   samples, *total = samples up to the end of the last one.  The samples between the streams must be ZERO (the
 *                   caller writes them once, or passes AM_F_ZERO_GAPS and the library writes them on every call).
 * am_process_multi  iq: that buffer (host, or device with AM_F_DEVICE_IN); out/cap/n_out as am_process_iq; the packets come
 *                   stream by stream, in stream order inside each; count[j] (may be NULL) = packets of stream j.
 *                   Not with use_dcblock; "rx_time" tags do not apply (every stream starts at 0 s);
 *                   the context's stream state is reset before and after. */
AM_API int am_multi_layout(am_ctx *ctx, uint32_t k, const uint64_t *n, uint64_t *offset, uint64_t *total);
AM_API int am_process_multi(am_ctx *ctx, float *iq, uint32_t k, const uint64_t *n, uint32_t flags,
                            am_packet *out, uint64_t cap, uint64_t *count, uint64_t *n_out);
/* The same in two halves (as am_submit_iq / am_collect): am_submit_multi enqueues the scan and returns (the buffer must stay valid
 * until the scan is collected); am_collect -- the call that collects a single-stream batch -- waits for it and hands out the
 * packets, stream by stream; am_multi_counts(count, k) then gives the packets per stream of the scan just collected. */
AM_API int am_submit_multi(am_ctx *ctx, float *iq, uint32_t k, const uint64_t *n, uint32_t flags);
AM_API int am_multi_counts(am_ctx *ctx, uint64_t *count, uint32_t k);
/* preamble hits (tags) seen by the last am_process_iq call, accepted or not */
AM_API uint64_t am_last_num_tags(const am_ctx *ctx);
/* The inter-block stream of the last am_process_iq / am_collect call that ran with AM_F_KEEP_TAGS: one 240-float burst
 * and one tag per preamble hit, in stream order, exactly what gr::air_modes::preamble would have produced for the
 * slicer (lib/preamble_impl.cc:219-232), from the SAME kernels that produced the call's packets.  bursts: cap*240
 * floats; tags: cap entries; either may be NULL to skip it.  AM_ECAPACITY (*n_out = needed) if cap is too small. */
AM_API int am_fetch_tags(am_ctx *ctx, float *bursts, am_tag *tags, uint64_t cap, uint64_t *n_out);

/* ---- block-level entry points (for block-by-block parity tests) -------------------------
 * am_frontend_work: the three third-party blocks in front of the preamble detector
 *   (rx_path.py:38,49,54) on a whole stream that starts at sample 0: bb = pulse-matched
 *   power, avg = reference level, n floats each.
 * am_preamble_work: gr::air_modes::preamble_impl::general_work run to completion over the
 *   two float streams `in` and `inavg` (n items each, stream starts at item 0; the block's
 *   history of 2*spc-1 zeros is implied).  bursts: cap*240 floats; tags: cap entries.
 * am_slicer_work: gr::air_modes::slicer_impl::work over nbursts tagged bursts.
 *   Only accepted packets are written to out. */
AM_API int am_frontend_work(am_ctx *ctx, const float *iq, uint64_t n_complex, uint32_t flags,
                     float *bb, float *avg);
AM_API int am_preamble_work(am_ctx *ctx, const float *in, const float *inavg, uint64_t n,
                     uint32_t flags, float *bursts, am_tag *tags, uint64_t cap,
                     uint64_t *n_out);
/* The preamble block as a STREAM: what gr::air_modes::preamble is under the scheduler (include/gr_air_modes/preamble.h:36-46;
 * general_work is called again and again on the next items, lib/preamble_impl.cc:139-246).  Consecutive calls on consecutive pieces
 * of the two input streams give, together, what ONE am_preamble_work over the concatenation gives: decisions wait for (240 + 4)
 * samples-per-chip items of look-ahead, the undecided tail of both inputs is carried inside the context, the greedy scan resumes
 * where it stopped (consume_each, :213,237,244), item counts and time stamps keep counting.  AM_F_FLUSH: these are the stream's last
 * items (end-of-buffer rule :150,212); the next call starts a new stream at item 0.  am_reset() drops the carried state.
 * bursts / tags: this call's hits, cap entries; AM_ECAPACITY with *n_out = the number needed if they do not fit (nothing is lost,
 * the stream has moved on: am_fetch_tags hands them out).  With AM_F_DEVICE_IN both inputs are device pointers. */
AM_API int am_preamble_stream(am_ctx *ctx, const float *in, const float *inavg, uint64_t n, uint32_t flags,
                              float *bursts, am_tag *tags, uint64_t cap, uint64_t *n_out);
AM_API int am_slicer_work(am_ctx *ctx, const float *bursts, const am_tag *tags, uint64_t nbursts,
                   uint32_t flags, am_packet *out, uint64_t cap, uint64_t *n_out);

/* ---- host-side helpers ------------------------------------------------------------------
 * am_crc24: modes_check_crc(data, length) (lib/modes_crc.cc:55-63): CRC-24, generator
 *   0xFFF409, zero initial value, over the first nbytes bytes.
 * am_format_message: the text slicer_impl.cc:186-192 posts to the gr::msg_queue:
 *   "<hex payload> <crc %06x> <reference_level> <secs> <frac>".  first != 0 formats the
 *   reference level with 6 significant digits (the first message a slicer instance emits),
 *   otherwise 10 (every later one) -- the member ostringstream keeps setprecision(10).
 *   Returns the length written (excluding NUL) or AM_ECAPACITY. */
AM_API uint32_t am_crc24(const uint8_t *data, int nbytes);
AM_API int am_format_message(const am_packet *pkt, int first, char *buf, size_t cap);
/* The same for n packets in one call (a binding posts a batch per call instead of crossing the FFI per packet): text k is
 * the NUL-terminated string at buf + offsets[k]; offsets has n + 1 entries, offsets[n] = bytes used.  `first` applies to
 * packet 0 only -- the stream's precision is sticky (slicer_impl.cc:186-194; the ostringstream is a member,
 * slicer_impl.h:43).  AM_ECAPACITY when cap is too small: *need (optional) then holds the bytes required (a text is at most
 * 96 bytes with its terminator: 28 hex digits, 6 of the syndrome, two %.10g numbers of up to 16 characters, a 20-digit count of
 * seconds, separators; typical ones take 55-65) and nothing beyond cap was written. */
AM_API int am_format_messages(const am_packet *pkts, uint64_t n, int first, char *buf, size_t cap, uint64_t *offsets,
                              uint64_t *need);

/* ---- time-sharded operation (one context per GPU, one contiguous time chunk each) -------
 * The reference's preamble scan is sequential, but the only state that crosses a chunk
 * boundary is ONE number: the position at which the scan resumes ("cur": after a hit at e the
 * scan skips to e + 240*spc, lib/preamble_impl.cc:237; after a rejected candidate to e + 1,
 * :209).  That position can reach at most 241*spc samples into the next chunk, so a chunk's
 * result depends on its predecessor only through which of its first few candidates (those in
 * its first 241*spc samples, the "lead-in") the scan enters at.  Protocol per step:
 *   1. every rank attaches its neighbours' boundary samples (am_shard_halo) and runs
 *      am_shard_scan on its chunk: front end, detection, refinement, successor array and block
 *      exits of its own greedy chain -- and an EXIT TABLE: for each lead-in candidate (plus the first candidate
 *      after the lead-in, if any) the position at which the scan would leave the chunk if it
 *      entered at that candidate;
 *   2. the small tables are exchanged (all-gather, a few KB), every rank composes them
 *      (am_shard_entry) to learn the position at which the scan enters ITS chunk;
 *   3. am_shard_resolve marks the chain from that entry and extracts + slices the chunk's hits.
 * The concatenation of all chunks' packets equals the single-stream result.
 *
 * am_shard_scan: iq holds samples [abs_start - left, abs_end + right) of the global stream
 *   (left/right from am_shard_halo, clipped to [0, total_n)); AM_F_DEVICE_IN if on the GPU.
 *   table/cap: caller's host array; *n_table entries written (AM_ECAPACITY if cap is too small,
 *   *n_table = needed).
 * am_shard_entry: tables[r] / counts[r] for r = 0..nranks-1 in chunk order, starts[r] = abs_start of
 *   chunk r; writes entry[r] = scan position when it reaches chunk r (entry[0] = 0). Host only.
 * am_shard_resolve: cur_in = entry of this rank's chunk. */
#define AM_SHARD_MSG_HEADER 2   /* header entries of a device message (am_shard_scan_async) */
typedef struct am_shard_exit {
    uint64_t pos;          /* absolute position of the candidate                            */
    uint64_t exit;         /* scan position after the chunk's last visited candidate, if the
                              scan enters the chunk at this candidate                       */
} am_shard_exit;

AM_API int am_shard_halo(const am_ctx *ctx, uint64_t *left, uint64_t *right);
AM_API int am_shard_scan(am_ctx *ctx, const float *iq, uint64_t abs_start, uint64_t abs_end,
                  uint64_t total_n, uint32_t flags, am_shard_exit *table, uint64_t cap,
                  uint64_t *n_table);
AM_API int am_shard_entry(const am_shard_exit *const *tables, const uint64_t *counts, const uint64_t *starts,
                   uint32_t nranks, uint64_t *entry);
AM_API int am_shard_resolve(am_ctx *ctx, uint64_t cur_in, am_packet *out, uint64_t cap, uint64_t *n_out);
/* A receiver, not a batch (round 4): the scan position crosses STEPS as it crosses chunks (lib/preamble_impl.cc:213,237,244:
 * consume_each -- the reference's scan resumes where the last general_work left off, for ever).  Step k covers the samples
 * [k W n, (k + 1) W n); rank r owns the POSITIONS [k W n + r n - H, k W n + (r + 1) n - H), H = `right` of am_shard_halo (the
 * look-ahead a decision needs), so its chunk needs left + H samples of the rank before it (of the last rank's previous
 * step for rank 0) and none of the rank after it; it scans with AM_F_MORE and total_n = the samples so far, and the last
 * step of the stream without the flag and with the true length.
 * am_shard_entry2: am_shard_entry with the position at which the scan left the last chunk of the step before (cur_in; 0 at
 *   the start of a stream); also writes leave[r] = where the scan leaves chunk r (either array may be NULL).
 * am_shard_get_exit / am_shard_set_exit: where the scan left THIS context's chunk in its last resolved step -- the word the
 *   host-free step keeps on the device and sends along in the next step's message header (below); a step that ran on the
 *   synchronous path sets it (leave[rank]), a caller that falls back to that path reads it. */
AM_API int am_shard_entry2(const am_shard_exit *const *tables, const uint64_t *counts, uint32_t nranks, uint64_t cur_in,
                    uint64_t *entry, uint64_t *leave);
/* The samples the NEXT step needs in front of a chunk are this step's last ones, and the caller is about to overwrite them:
 * am_shard_keep_tail registers a device-to-device copy (nbytes from src to dst; 0: none) that every following
 * am_shard_resolve / am_shard_resolve_async enqueues behind its slicing -- which still reads the samples -- and in front of
 * its completion, so that it is done when the call returns (a host-side copy after the call costs a launch and an event on
 * the critical path of the next step).  dst must not be part of what a repeated step would scan.
 * am_stream_copy: a device-to-device copy on the context's stream, ordered with its scans (e.g. the kept tail into the halo
 * in front of the chunk, before the next am_shard_scan_async). */
AM_API int am_shard_keep_tail(am_ctx *ctx, void *dst, const void *src, uint64_t nbytes);
AM_API int am_stream_copy(am_ctx *ctx, void *dst, const void *src, uint64_t nbytes);
/* (am_shard_get_exit / am_shard_set_exit, the exit word of the synchronous fallback: airmodes_hip_debug.h) */

/* The same step without a host round trip in the middle (round 3): the exit table stays on the device.
 * am_shard_scan_async: as am_shard_scan, but everything is only ENQUEUED and the table goes to the device message
 *   msg_dev = AM_SHARD_MSG_HEADER + msg_cap entries: entry 0 = {count, overflow} (count = msg_cap + 1: the table did not
 *   fit; overflow = 1: the scan met more candidates than the capacity it was launched for), entry 1 = {where the scan left
 *   this context's chunk in the step before, -} (how the scan position reaches the next step: every rank reads the last
 *   rank's), then the table.
 * The caller all-gathers the messages (device to device, e.g. torch.distributed over RCCL: am_signal_stream makes the
 *   collective's stream wait for the table, am_wait_for_stream the context for the collective) and hands all `world`
 *   of them, in chunk order, to
 * am_shard_resolve_async: composes the entry position of chunk `rank` on the device (am_shard_entry as a kernel), marks the
 *   chain from there, extracts and slices -- ONE completion wait per step.  *redo != 0: a table did not fit its message,
 *   or some rank's scan met more candidates than the capacity it was launched for (both rare, both read from the message
 *   headers: *redo is the same on every rank): no packets were delivered, repeat the step with am_shard_scan /
 *   am_shard_entry / am_shard_resolve. */
AM_API int am_shard_scan_async(am_ctx *ctx, const float *iq, uint64_t abs_start, uint64_t abs_end, uint64_t total_n,
                        uint32_t flags, am_shard_exit *msg_dev, uint64_t msg_cap);
AM_API int am_shard_resolve_async(am_ctx *ctx, const am_shard_exit *msgs_dev, uint32_t world, uint32_t rank, uint64_t msg_cap,
                           am_packet *out, uint64_t cap, uint64_t *n_out, int *redo);
/* another stream of the context's device (NULL: the legacy default stream) waits, on the device, for what the context has
 * enqueued so far (the counterpart of am_wait_for_stream) */
AM_API int am_signal_stream(am_ctx *ctx, void *hip_stream);

/* The resolve step in two halves (round 6: STEPS of the time-sharded receiver in flight -- the scan and the all-gather of step k + 1
 * are enqueued before step k is resolved, so that the collectives of one step hide behind the kernels of the next).
 * am_shard_resolve_submit only enqueues; am_shard_resolve_collect waits for the step's one completion ticket and hands the packets
 * out (*redo as am_shard_resolve_async).  cur_in_dev (device word, may be NULL): where the scan left the LAST chunk of the step
 * before, read when the entry is composed -- instead of the last rank's message header, which was written before that step was
 * resolved.  carry_out_dev (device word, may be NULL, may be the same word): where the scan leaves THIS step's last chunk, composed
 * by every rank for itself from everybody's tables -- the next step's cur_in. */
AM_API int am_shard_resolve_submit(am_ctx *ctx, const am_shard_exit *msgs_dev, uint32_t world, uint32_t rank, uint64_t msg_cap,
                                   const uint64_t *cur_in_dev, uint64_t *carry_out_dev);
AM_API int am_shard_resolve_collect(am_ctx *ctx, am_packet *out, uint64_t cap, uint64_t *n_out, int *redo);

/* ---- resampling in front of the path (python/radio.py:49-53) ------------------------------------------------
 * modes_radio resamples anything slower than 4 Msps to 4 Msps with pfb.arb_resampler_ccf before rx_path.  GNU Radio's
 * block and tap design are not in the reference tree (parity unpinned); this is the package's own 32-phase x 8-tap
 * polyphase interpolator, DEFINED operation by operation in air_modes/resample.py and repeated bit for bit on the GPU.
 * taps: 32 x 8 doubles [phase][tap] (air_modes.resample.design_taps).  ratio = f_out / f_in >= 1.
 * am_resampler_work: n complex input samples (host, or device with AM_F_DEVICE_IN) -> *n_out complex output samples,
 *   copied to `out` (host, or device with AM_F_DEVICE_OUT; cap complex samples) or, when out is NULL, left in the
 *   handle's device buffer (am_resampler_device_output, valid until the next call: hand it to am_process_iq with
 *   AM_F_DEVICE_IN).  The read position and the last 8 input samples carry over from call to call. */
typedef struct am_resampler am_resampler;
AM_API am_resampler *am_resampler_create(int device, double ratio, const double *taps, int *err);
AM_API void am_resampler_destroy(am_resampler *h);
AM_API int am_resampler_reset(am_resampler *h);
AM_API int am_resampler_work(am_resampler *h, const float *iq, uint64_t n_complex, uint32_t flags, float *out, uint64_t cap,
                      uint64_t *n_out);
AM_API const float *am_resampler_device_output(const am_resampler *h);
AM_API const char *am_resampler_last_error(const am_resampler *h);
/* The same stage for a radio's native samples (python/radio.py:164-231's sources in front of python/radio.py:49-53's
 * resampler), in ONE kernel launch per call and without a float32 copy of the input: the kernel reads the AM_FMT_* samples
 * (declared below) where they lie and widens them as am_unpack would.  DEFINITION: arb_resampler.work_samples of
 * air_modes/resample.py -- the outputs are am_resampler_work's on am_unpack's output, bit for bit, whatever the chunking.
 *   raw        n_complex samples of format fmt: host memory, or device memory with AM_F_DEVICE_IN; aligned to a component.
 *   AM_F_FLUSH the stream ends with this call: eight zero SAMPLES follow the call's own in the same call (the drain: the
 *              interpolator holds its last outputs back until it has seen what follows them), then position and carried samples
 *              are cleared as by am_resampler_reset.  With n_complex == 0 it drains only.
 *   out / cap / AM_F_DEVICE_OUT / am_resampler_device_output as for am_resampler_work.  *n_out is computed on the host before
 *              anything runs and is always written (AM_ECAPACITY: the count needed; the output is in the handle's buffer).
 * With AM_F_DEVICE_IN and (out == NULL or AM_F_DEVICE_OUT) the call returns WITHOUT waiting: the output is ordered on the
 * handle's stream.  With host input it returns once the raw bytes have left the caller's buffer, with host output when the
 * output is there.  AM_EINVAL for an unknown format, a null pointer with n_complex > 0, and n_complex > 2^31.
 * AM_FMT_CF32 gives am_resampler_work's result.  Calls of both kinds may be mixed on one handle: they carry one state.
 * am_resampler_work itself still returns only when its output is complete. */
AM_API int am_resampler_work_samples(am_resampler *h, const void *raw, uint64_t n_complex, int fmt, uint32_t flags, float *out,
                                     uint64_t cap, uint64_t *n_out);
/* Run the handle's device work on the caller's HIP stream (NULL: back to the handle's own), as am_set_stream does for a
 * context.  On the receive context's stream (am_get_stream) the am_process_iq(..., AM_F_DEVICE_IN) behind an
 * am_resampler_work_samples call is ordered by the stream, and nothing waits on the host between python/radio.py:49-53's
 * resampler and rx_path.  The stream must outlive the handle or be replaced before it is destroyed. */
AM_API int am_resampler_set_stream(am_resampler *h, void *hip_stream);

/* ---- pinned staging for a host source (apps/modes_rx's file source, python/radio.py:221-234) --------------------
 * nslots pinned host buffers of capacity_complex samples each, with a device twin and a copy stream: the reader fills
 * am_uploader_host(slot), am_uploader_start begins the copy and returns, am_uploader_wait blocks until that slot's
 * samples are on the device and returns the device pointer (for am_process_iq / am_resampler_work with
 * AM_F_DEVICE_IN) -- the transfer of chunk k+1 overlaps the scan of chunk k.  start and wait may be called from
 * different threads (one producer, one consumer); a slot is reused only after its consumer is done with it. */
typedef struct am_uploader am_uploader;
AM_API am_uploader *am_uploader_create(int device, uint64_t capacity_complex, int nslots, int *err);
AM_API void am_uploader_destroy(am_uploader *u);
AM_API float *am_uploader_host(am_uploader *u, int slot);
AM_API int am_uploader_start(am_uploader *u, int slot, uint64_t n_complex);
AM_API const float *am_uploader_wait(am_uploader *u, int slot);

/* the same for raw bytes (native sample formats below; the host side of what replaces python/radio.py:164-231's converting
 * sources): the pinned slots hold capacity_complex * 8 bytes; start a copy of nbytes raw bytes, am_uploader_wait as before */
AM_API int am_uploader_start_bytes(am_uploader *u, int slot, uint64_t nbytes);

/* ---- native sample formats (python/radio.py:164-231) ----------------------------------------------------------
 * The reference's sources hand rx_path float32 whatever the radio delivers: uhd.stream_args(cpu_format="fc32") and
 * osmosdr.source convert on the host (python/radio.py:164-231).  This package has no such blocks; instead the raw
 * little-endian integer pairs (I then Q) cross PCIe as they are and are widened on the device, in the context's stream, in
 * front of the front end.  DEFINITION (air_modes/formats.py; every operation exact in float32, so bit for bit):
 *   AM_FMT_CF32  float32  x
 *   AM_FMT_SC16  int16    float(x) * 2^-15
 *   AM_FMT_CS8   int8     float(x) * 2^-7
 *   AM_FMT_CU8   uint8    (float(x) - 127.5f) * 2^-7
 * The packets of a raw stream are the packets of the float32 stream this conversion produces. */
#define AM_FMT_CF32 0   /* replaces python/radio.py:164-231's host-side conversion: nothing to convert */
#define AM_FMT_SC16 1   /* python/radio.py:164-231: what a USRP sends over the wire (otw sc16) before uhd widens it */
#define AM_FMT_CS8  2   /* python/radio.py:164-231: HackRF through osmosdr.source */
#define AM_FMT_CU8  3   /* python/radio.py:164-231: RTL-SDR through osmosdr.source */
/* bytes per complex sample; 0 for an unknown format (in place of the item sizes of python/radio.py:164-231's blocks) */
AM_API size_t am_sample_bytes(int fmt);
/* The conversion alone (what python/radio.py:164-231's source blocks do before rx_path): raw (host, or device with
 * AM_F_DEVICE_IN; aligned to its component) -> out_dev (device, 2 * n_complex floats, 8-byte aligned), enqueued on the
 * context's stream.  With host input the call returns once the raw bytes have left the caller's buffer; with device input
 * it returns at once, and what follows on the context's stream (am_process_iq with AM_F_DEVICE_IN, ...) is ordered behind
 * it; a consumer on another stream orders itself with am_signal_stream, or the host waits with am_synchronize.
 * This is also how callers of the pipes (am_pipe_*, am_spipe_*), of am_process_multi and of the shard calls feed raw data:
 * they own float32 device buffers already, and those calls take no format argument. */
AM_API int am_unpack(am_ctx *ctx, const void *raw, uint64_t n_complex, int fmt, uint32_t flags, float *out_dev);
/* the host waits for everything enqueued on the context's stream so far (am_unpack's output for am_resampler_work, which
 * runs on a stream of its own: python/radio.py:164-231's source in front of :49-53's resampler) */
AM_API int am_synchronize(am_ctx *ctx);
/* am_process_iq on am_unpack's output (rx_path behind python/radio.py:164-231's sources): same flags, same chunking
 * rules, same results.  Host input: the RAW bytes are copied to a staging buffer of the context and unpacked straight
 * behind the carried tail, so a sample crosses PCIe once, at its raw width.  AM_FMT_CF32 is am_process_iq itself.
 * (At 64 Msps nothing is unpacked: the kernels of the scan read the raw samples themselves and the carried tail stays at raw
 * width -- DESIGN.md 12; the packets are the same by definition, and nothing here changes for the caller.)
 * AM_EINVAL for an unknown format or a null pointer with n_complex > 0. */
AM_API int am_process_samples(am_ctx *ctx, const void *raw, uint64_t n_complex, int fmt, uint32_t flags,
                              am_packet *out, uint64_t cap, uint64_t *n_out);

/* The raw front end: a switch and a diagnostic for tests and measurement, not part of the drop-in surface
 * (they stand in this header because the list of airmodes_hip_debug.h is pinned by tests/test_capi_host.py).
 * At 64 Msps a stream of AM_FMT_SC16 / CS8 / CU8 samples (am_process_samples) is scanned as it is: am_k_fe3<FMT>,
 * am_k_refine_seg<PMF, FMT> and am_k_extract_slice_iq<32, ..., 1> read the integers, the carried tail stays at raw width and
 * am_k_unpack does not run.  Packets are the same either way (they are DEFINED as those of the converted stream).  The
 * switch is the A/B lever, not a user option: default 1; it survives am_reset and am_set_rate; a new value takes effect when
 * the next stream starts (after am_create, am_reset, am_set_rate or AM_F_FLUSH).  Every other configuration -- other rates,
 * the DC blocker, am_submit_iq, pipes, K streams, shards -- widens first, whatever the switch says; so does the rest of a
 * stream whose calls change format.
 * The switch has a second level.  AM_RAW_FE_ALL adds the rates am_k_fe4 serves: am_k_fe4<SPC, G, NW, FMT> stages the integers and
 * am_k_extract_slice_iq<SPC, ..., 1> reads them; fractional rates, the DC blocker and the calls named above still widen first.
 * am_set_raw_front_end stores 2 for 2 and 1 for every other non-zero value; am_get_raw_front_end returns the stored level.
 * Level 2 is opt-in: it becomes the default only in a later change that edits tests/rawfe_common.py::check_route (which pins
 * that the default widens a 20 Msps stream) and that brings the hardware measurement DESIGN.md 12 asks for. */
#define AM_RAW_FE_OFF 0   /* widen first, everywhere                                             */
#define AM_RAW_FE_64  1   /* default, as today: native at 64 Msps only                           */
#define AM_RAW_FE_ALL 2   /* native at every rate the streaming front ends serve:                */
                          /* 2, 4, 8, 10, 16, 20, 32, 40 and 64 Msps                             */
AM_API int am_set_raw_front_end(am_ctx *ctx, int on);
AM_API int am_get_raw_front_end(const am_ctx *ctx);
/* Diagnostic: the AM_FMT_* the front end of the last scan read -- AM_FMT_CF32 for float32 input and for a raw stream that was
 * widened first (also before any scan); negative on a null context. */
AM_API int am_last_scan_format(const am_ctx *ctx);

/* last error text of the context (or of am_create when ctx == NULL) */
AM_API const char *am_last_error(const am_ctx *ctx);

/* Diagnostics, test hooks and the time-shard path's exit word (am_last_timing, am_last_num_candidates, am_last_frontend,
 * am_fetch_candidates, am_is_emulated, am_shard_get_exit, am_shard_set_exit) are declared in airmodes_hip_debug.h: they are
 * exported by the same library but are not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* AIRMODES_HIP_H */
