// am_internal.h -- kernel launch interface between am_capi.hip (host logic) and the gfx950 kernels with their launchers:
// am_kernels.hip, am_fe2.hip (test builds), am_fe3.hip, am_fe4.hip, am_refine_seg.hip, am_dcblock.hip, am_resample.hip.
// Not part of the public ABI.
//
// How a launcher is called: what several launches share travels as one small struct, built where the context knows it --
//   am_records      the resident candidate records and their count (every refinement, the chain, the extraction)
//   am_emit_args    what the chain does with the candidates it visits; the marking kernels take it by value
//   am_slice_out    what a slicing launch writes and which <FIX, GATE, LF> instantiation runs (all three slicing launches)
//   am_stamp        the time tags of the two extraction launches
// -- and a launcher has a struct of its own only for what is its alone (am_walk_req, am_dense_src, am_iq_src, ...).  A launcher that
// takes one of them has no default arguments: an option nobody wants is written out as null or 0 at the call.  The launchers unpack the
// structs into kernel arguments; no __global__ function's parameter list depends on them, except where it always did
// (am_emit_args, am_entry_src, am_fe_args, am_geom).  The words of the context's two scalar blocks have names
// (am_scalar_word, am_pinned_word) that host and kernels share; which template instantiation a run-time value selects is
// decided in am_dispatch.h.
#ifndef AM_INTERNAL_H
#define AM_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "airmodes_hip.h"
#include "airmodes_hip_debug.h"

#ifndef AM_WITH_TILE_KERNEL
#define AM_WITH_TILE_KERNEL 0   /* 1 in TEST builds (tests/gpu_variants, tests/emu): the tile kernel am_k_fe2 and the split refinement behind it */
#endif
#define AM_CHIPS_AVG 48    /* reference level window in chips  (python/rx_path.py:54)      */
#define AM_BURST 240       /* chips handed to the slicer       (lib/preamble_impl.cc:219)  */
#define AM_WAVE 64

int am_device_cus(void);   /* compute units of the current device (cached)                  */

/* ---- the two scalar blocks of a context ------------------------------------------------------
 * Every context has a small block of 32-bit words in device memory (`scalars`, zero when allocated) and one in pinned host
 * memory (`pin_scalars`) that the last kernels of a scan write for the host.  Host and kernels address both by these names only. */
enum am_scalar_word {            /* device block */
    AM_SW_RESUME = 0,            /* where the greedy scan resumes: cleared by am_k_cblk_exit, raised by the walk and the marking  */
    AM_SW_NBURSTS = AM_SW_RESUME,/* INTENDED ALIAS: am_slicer_work, which runs no chain, keeps its burst count (n_ptr) here       */
    AM_SW_HIT = 1,               /* cleared with AM_SW_RESUME                                                                     */
    AM_SW_ENTRY = 4,             /* time shards: the array coordinate at which the scan enters the chunk (am_k_shard_entry)       */
    AM_SW_ENTRY_FLAG = 5,        /* ... 1: some exit table did not fit its message, the step is repeated                          */
    AM_SW_CHAIN_ERR = 9,         /* a chained scan or the fused walk gave up waiting (am_chain_prefix, am_cblk_mark_body)         */
    AM_SW_TICKET_SCAN = 10,      /* ticket counter of am_k_exscan_chain (am_chain_place)                                          */
    AM_SW_TICKET_MARK = 11,      /* ... of the marking kernels                                                                    */
    AM_SW_LONG_FMT = 12,         /* am_set_long_formats: bit 18 = DF18, bit 19 = DF19 is 112 bits long (am_slice_wave<.., .., 1>)  */
    AM_SW_GATE_REC = 14,         /* 64 bits, words 14..15: the address of the gate's record array (am_slice_wave<FIX, 1 or 2>)    */
    AM_SW_WORDS = 16
};
enum am_pinned_word {            /* pinned block */
    AM_PW_HITS = 0,              /* the slicing launch: hits, ...                                                                 */
    AM_PW_RESUME = 1,            /* ... scalars[AM_SW_RESUME], ...                                                                */
    AM_PW_CANDIDATES = 2,        /* ... *Mp, the candidate count of a capacity launch (0 without one)                             */
    AM_PW_SHARD_COUNT = 3,       /* am_shard_scan's ticket: the same count, before any tail runs                                  */
    AM_PW_FLAG = 4,              /* a time shard's ticket: scalars[AM_SW_ENTRY_FLAG]                                              */
    AM_PW_CHAIN_ERR = 5,         /* the extraction launches: scalars[AM_SW_CHAIN_ERR]                                             */
    AM_PW_TICKET = 8,            /* the completion ticket the host polls (wait_for_ticket)                                        */
    AM_PW_GATE_TAUGHT = 9,       /* am_k_gate_ticket: taught, ...                                                                 */
    AM_PW_GATE_PASSED = 10,      /* ... passed, ...                                                                               */
    AM_PW_GATE_DROPPED = 11,     /* ... dropped                                                                                   */
    AM_PW_EXIT = 12,             /* 64 bits, words 12..13: where the scan left a time chunk (am_k_ticket's word_dst)              */
    AM_PW_REPAIRED = 14,         /* am_k_gate_repair_ticket: address/parity replies repaired, ...                                 */
    AM_PW_AMBIGUOUS = 15,        /* ... and left alone because two addresses fitted                                               */
    AM_PW_WORDS = 16
};
/* (AM_SW_NBURSTS above is the only alias; every other name of a block has a word, or an aligned pair of words, to itself) */
constexpr bool am_word_map_ok(std::initializer_list<int> words, int size)   /* every word inside the block, no word twice */
{
    for (const int *a = words.begin(); a != words.end(); ++a) {
        if (*a < 0 || *a >= size) return false;
        for (const int *b = words.begin(); b != a; ++b)
            if (*a == *b) return false;
    }
    return true;
}
static_assert(am_word_map_ok({AM_SW_RESUME, AM_SW_HIT, AM_SW_ENTRY, AM_SW_ENTRY_FLAG, AM_SW_CHAIN_ERR, AM_SW_TICKET_SCAN,
                              AM_SW_TICKET_MARK, AM_SW_LONG_FMT, AM_SW_GATE_REC, AM_SW_GATE_REC + 1}, AM_SW_WORDS), "device block");
static_assert(am_word_map_ok({AM_PW_HITS, AM_PW_RESUME, AM_PW_CANDIDATES, AM_PW_SHARD_COUNT, AM_PW_FLAG, AM_PW_CHAIN_ERR,
                              AM_PW_TICKET, AM_PW_GATE_TAUGHT, AM_PW_GATE_PASSED, AM_PW_GATE_DROPPED, AM_PW_EXIT, AM_PW_EXIT + 1,
                              AM_PW_REPAIRED, AM_PW_AMBIGUOUS}, AM_PW_WORDS), "pinned block");
static_assert(AM_SW_GATE_REC % 2 == 0 && AM_PW_EXIT % 2 == 0, "the 64-bit slots are 8-byte aligned (the blocks themselves are)");
static_assert(AM_PW_GATE_PASSED == AM_PW_GATE_TAUGHT + 1 && AM_PW_GATE_DROPPED == AM_PW_GATE_TAUGHT + 2,
              "the gate's three counters are consecutive (chain_collect adds them up in a loop)");

/* Geometry of the preamble block for one sample rate, in the reference's own arithmetic: d_samples_per_chip is a FLOAT
 * (lib/preamble_impl.cc:57) and every use of it is a float product truncated by int() -- for a rate that is not a multiple
 * of 2 MHz (5 Msps: 2.5 samples per chip) that gives a slightly crooked but well-defined geometry.  With whole samples per
 * chip all of it reduces to multiples of spc (o1 = 2 spc, za0 = 3 spc, ..., B = 240 spc, chip j at j spc). */
struct am_geom {
    int S;              /* int(samples per chip): granularity of ninputs (:150), correlation window (:90-98, :185)  */
    int hist0;          /* history items in front of the stream: set_history(d_samples_per_symbol) - 1 (:62)       */
    int o1, o2, o3;     /* pulse offsets int(2 spc), int(7 spc), int(9 spc) (:158-162)                              */
    int late_max;       /* the late-peak loop runs while how_late < d_samples_per_chip (:192): at most this many     */
    int za0, za1;       /* quiet zone 1: j = int(1.5 sps) .. j <= 3 sps, inclusive (:205)                            */
    int zb0, zb1;       /* quiet zone 2: j = int(5 sps) .. j <= 7.5 sps, inclusive (:207)                            */
    int B;              /* items consume_each() skips after a hit: int(240 spc) (:237)                               */
    int room;           /* a hit needs `ninputs - i < 240 spc` to be false (:212): at least this many items          */
    int span;           /* int(239 spc): offset of the last soft chip (:220)                                         */
};

/* ---- the resident records ----------------------------------------------------------------
 * One flat record per candidate, in position order: what a refinement writes and the greedy chain and the extraction read.
 * The context builds the struct in one place (am_ctx::records); every launcher takes it as `const am_records &` -- the
 * pointers are not const because the refinements write through them -- and unpacks it into its kernel's arguments.
 * M is the number of records, or the capacity they were launched for when the count is only known on the device: then
 * Mp points at it and the kernels use min(M, *Mp), so that the host may launch without knowing the count. */
struct am_records {
    uint32_t *pos;         /* position where the first-stage test fired                                   */
    uint32_t *e;           /* shifted preamble start                                                      */
    uint32_t *tgt;         /* where the scan resumes after this candidate                                 */
    float *inavg;          /* reference level at e                                                        */
    uint8_t *valid;
    uint32_t *jump0;       /* M + 1 successors of the greedy chain (null where no launch reads them)      */
    uint32_t M;
    const uint32_t *Mp;    /* null: M is exact                                                            */
};
/* what the refinements behind a front end read: bb (dense, or the rows around candidates), the reference level (likewise),
 * the threshold, and the first array coordinate without a sample */
struct am_refine_in {
    const float *bb, *avg;
    float thr_lin;
    uint32_t end_j;
};

/* ---- front end ---------------------------------------------------------------------- */
#define AM_FE_THREADS 512
#define AM_FE_LDS_BUDGET (80 * 1024)

struct am_fe_args {
    const float *iq;      /* interleaved I,Q; element 0 is absolute sample src_abs0        */
    long long src_abs0;   /* absolute index of the first sample present in iq              */
    long long src_abs1;   /* absolute end (exclusive) of the samples present               */
    long long out_abs0;   /* absolute index of bb[0]/avg[0]; multiple of 48*spc            */
    long long out_n;      /* number of outputs wanted                                      */
    float *bb;
    float *avg;
    int spc;
    int use_pmf;
    int tile;             /* outputs per workgroup; multiple of 48*spc                     */
    float s1;             /* float(1.0/spc)                                                */
    float sL;             /* float(1.0/(48*spc))                                           */
};
size_t am_fe_lds_bytes(int spc, int tile);
int am_fe_pick_tile(int spc);                  /* largest tile within AM_FE_LDS_BUDGET, 0 if none */
hipError_t am_launch_frontend(const am_fe_args &a, hipStream_t s);

/* fused front end + detection, specialised per samples-per-chip (am_fe2.hip).
 * am_fe2_tile(spc): tile length of the specialisation, 0 if spc has none (generic kernels). */
unsigned am_fe2_tile(int spc);
hipError_t am_launch_fe2(int spc, const float *iq, long long src_abs0, long long src_abs1, long long out_abs0,
                         long long out_n, float *bb, float *avg, uint32_t j0, uint32_t j1, int use_pmf, float s1,
                         float sL, float thr_lin, uint32_t *seg_pos, float *avg_sparse, uint32_t *blk_cnt,
                         unsigned *ntiles, unsigned *tile_len, hipStream_t s);
/* ---- streaming fused front ends (am_fe4.hip; am_fe3.hip at 64 Msps) and what reads their bitmap -------------------------------
 * Persistent workgroups, LDS rings, sparse outputs.  A lane takes a unit of G chips = am_fe4_unit(spc) samples (one 32-sample
 * chip at 64 Msps).  Candidates leave as a bitmap, a word per unit; a step has am_fe4_waves(spc) x am_fe4_words(spc) words
 * (waves of 64 words at 20, 10 and 2 Msps, of 48 otherwise).  wg_cnt[g] = candidates workgroup g found; wg_max[g] (nsteps + 8
 * floats are enough) = the largest bb workgroup g formed, +inf if one was not finite.
 * (64 Msps: am_k_fe3 -- one 32-sample chip per lane, 16-byte LDS rows, two segments of 48 words per step, lag 288) */
int am_fe4_supported(int spc);
unsigned am_fe4_unit(int spc);              /* positions per bitmap word                                        */
unsigned am_fe4_words(int spc);             /* bitmap words per step and wave                                   */
unsigned am_fe4_waves(int spc);             /* segments (waves) per step                                        */
unsigned am_fe4_tile(int spc);              /* positions per step                                               */
unsigned am_fe4_lag(int spc);
unsigned am_fe4_steps(long long out_n, int spc);
int am_fe4_uses_fe3(int spc);               /* am_launch_fe4 runs am_k_fe3<FMT> at this rate (64 Msps, product configuration) */
int am_fe4_reads_raw(int spc);              /* am_launch_fe4 runs am_k_fe4<SPC, G, NW, FMT> at this rate (2 .. 40 Msps) */
unsigned am_fe3_waves(void);                /* am_k_fe3's segments (48 chips = 48 bitmap words each) per step   */

/* The bitmap a streaming front end leaves and who made which part of it: workgroup g took a contiguous run of steps and formed
 * the bb of their array coordinates (and some before them).  Computed ONCE, by am_fe_plan: the front-end launchers launch from
 * it, everything behind them reads it. */
struct am_fe_layout {
    uint32_t wbits = 32;      /* positions per bitmap word                                                       */
    uint32_t lag = 0;         /* bit b of word w = array coordinate w * wbits + b - lag                          */
    uint32_t wps = 0;         /* bitmap words per step                                                           */
    uint32_t tile = 0;        /* positions per step (= wps * wbits)                                              */
    uint32_t nsteps = 0;
    uint32_t nwg = 0;         /* workgroups (the front end's grid)                                               */
    uint32_t spw = 1;         /* steps per workgroup (of the long ones)                                          */
    uint32_t n_long = 0;      /* LEVELLED segments: the first n_long workgroups take spw steps, the others spw - 1 */
    bool alike() const { return n_long >= nwg; }               /* n_long == nwg: one segment length                   */
    uint32_t steps_short() const { return alike() ? spw : spw - 1u; }
    uint32_t words_per_wg() const { return spw * wps; }
    uint32_t words_short() const { return steps_short() * wps; }
    uint32_t nwords() const { return nsteps * wps; }
    uint32_t vspan() const { return spw * tile; }              /* array coordinates per workgroup: wg_max[coordinate / vspan] */
    uint32_t vspan_short() const { return steps_short() * tile; }
    uint32_t nv() const { return nwg; }                        /* entries of wg_cnt / wg_max                          */
};
/* Pure arithmetic.  resident: workgroups that run at once -- the launchers' business (occupancy, wgs_per_cu, test knobs).
 * Unlevelled: ceil(nsteps / resident) steps per workgroup, at least 4, or force_spw (tuning builds).  levelled (honoured where
 * am_k_fe3 runs; asked for by the caller whose later kernel places two segment lengths too: am_k_refine_seg): min(resident,
 * nsteps / 4) workgroups, the steps dealt out as evenly as they go. */
am_fe_layout am_fe_plan(int spc, long long out_n, unsigned resident, bool levelled, unsigned force_spw = 0);

/* what a streaming front end is launched for (the fields am_fe3_args / am_fe4_args describe) */
struct am_fe_stream_req {
    const void *iq;                       /* samples of format fmt: am_k_fe3<FMT> and am_k_fe4<..., FMT> read them as they are */
    int fmt;
    long long src_abs0, src_abs1, out_abs0, out_n;
    float *bb_sparse, *avg_sparse;        /* (bb_sparse null: am_k_fe3 writes no rows)                       */
    uint32_t j0, j1;
    int use_pmf;
    float s1, sL, thr_lin;
    uint32_t *bits, *wg_cnt;
    float *wg_max;
};
/* ... and what it left, for the kernels that read it */
struct am_fe_marks {
    const uint32_t *bits, *wg_cnt;
    const float *wg_max;
};
/* *layout: what was launched (nsteps == 0: nothing).  wgs_per_cu: 0 = as many persistent workgroups as are resident at once;
 * n > 0 = at most n per CU -- am_pipe leaves room on every CU for the small kernels of the other batches in flight. */
hipError_t am_launch_fe3(const am_fe_stream_req &r, am_fe_layout *layout, hipStream_t s, int wgs_per_cu, bool levelled);
hipError_t am_launch_fe4(int spc, const am_fe_stream_req &r, am_fe_layout *layout, hipStream_t s, int wgs_per_cu, bool levelled);
/* flat candidate positions from the bitmap, one workgroup per front-end workgroup: workgroup g owns the words
 * [g * words_per_wg, (g + 1) * words_per_wg) (nwords in all) and starts its part of pos[] at the sum of wg_cnt[0 .. g)
 * -- no scan launch, no chain.  Entries at or beyond Mcap are dropped; *total_out = the number of candidates. */
/* rows != null && rows->iq (64 Msps: am_k_fe3 no longer writes them): the same launch also forms, from the samples, the bb rows
 * the refinement reads -- the 17 chips from every candidate's chip on, canonical order (am_rows_segment32). */
struct am_rows_args {
    const void *iq;                       /* null: no rows (the front end wrote them: am_k_fe4 rates)        */
    int fmt;                              /* AM_FMT_* of iq (am_k_refine_seg<PMF, FMT>; am_k_gather_wg: AM_FMT_CF32 only) */
    long long src_abs0, src_abs1;         /* absolute range of samples present in iq                        */
    long long out_abs0;                   /* absolute index of array coordinate 0                           */
    long long out_n;                      /* array coordinates with data (nothing is stored at or beyond)   */
    float *bb_sparse;
    float *bb_max;                        /* [array chip] the largest bb of every row formed (what am_k_refine_late takes for a chip that
                                             lies inside a quiet zone as a whole) */
    int use_pmf;
    float s1;
};
hipError_t am_launch_gather_wg(const uint32_t *bits, const uint32_t *wg_cnt, const am_fe_layout &l, uint32_t Mcap, uint32_t *pos,
                               uint32_t *total_out, hipStream_t s, const am_rows_args *rows = nullptr);
/* 64 Msps (round 6): candidate list + bb rows + refinement in ONE launch, one workgroup per front-end workgroup, the rows in LDS
 * (am_refine_seg.hip): what am_launch_gather_wg(rows) + am_launch_refine_late(bb_max) leave in pos / e / tgt / inavg / valid / jump0,
 * bit for bit, without the bb rows ever reaching memory.  rows: the samples (bb_sparse / bb_max are not used).  Places the
 * layout's two segment lengths. */
hipError_t am_launch_refine_seg(const am_fe_marks &m, const am_fe_layout &l, const am_rows_args &rows, const am_refine_in &in,
                                const am_records &r, uint32_t *total_out, hipStream_t s);   /* (in.bb is not read; r.M: the capacity) */
/* split refinement (after the fused kernel in split mode): flat candidate positions, one energy per
 * reachable position (deduplicated across neighbouring candidates), then one lane per candidate */
hipError_t am_launch_gather_pos(const uint32_t *seg_pos, uint32_t seg_stride, const uint32_t *blk_off,
                                uint32_t nseg, uint32_t M, int spc, uint32_t *pos, uint32_t *dcount,
                                hipStream_t s, const uint32_t *Mp = nullptr);
hipError_t am_launch_energy(const float *bb, const uint32_t *pos, const uint32_t *dcount,
                            const uint32_t *off_local, const uint32_t *blk_base, uint32_t M, int spc,
                            double *energy, hipStream_t s, const uint32_t *Mp = nullptr);
hipError_t am_launch_cand(const am_refine_in &in, const uint32_t *dcount, const uint32_t *off_local, const uint32_t *blk_base,
                          const double *energy, int spc, const am_records &r, hipStream_t s);   /* (r.pos is read, the rest written) */
/* behind the streaming front ends: late-peak decisions + per-candidate test + record + successor in one launch (the
 * decisions stay in LDS; no dcount / compact offsets).  r.pos is read, the rest of r written.
 * vmax[array coordinate / l.vspan()] (l.nv() entries) bounds the samples */
hipError_t am_launch_refine_late(const am_refine_in &in, int spc, const am_records &r, const float *vmax, const am_fe_layout &l,
                                 const float *bb_max, hipStream_t s);
/* (bb_max, 32 samples per chip only, null elsewhere: bb_max[c] = the largest bb of array chip c for every chip whose row exists --
 * am_k_gather_wg<1> writes it with the rows; a quiet zone's whole chips are then judged by six numbers instead of 192 samples) */
/* exclusive scan of n counts in ONE launch (2048 per workgroup, chained through slots[]: am_chain_prefix);
 * slots: one 64-bit word per workgroup, zero at allocation; epoch: a value no earlier launch on these slots used */
hipError_t am_launch_exscan_chain(const uint32_t *in, uint32_t *out, uint32_t n, unsigned long long *slots, uint32_t epoch,
                                  uint32_t *total_out, uint32_t *err, uint32_t *ticket, uint32_t *ticket_base, hipStream_t s,
                                  const uint32_t *Mp = nullptr);   /* *err = 1: the chain gave up; ticket: device counter,
                                  *ticket_base: the value it has when this launch starts (advanced by the grid size) */
hipError_t am_launch_ticket(uint32_t *host_word, uint32_t seq, hipStream_t s, const uint32_t *count_src = nullptr,
                            uint32_t *count_dst = nullptr, const uint64_t *word_src = nullptr, uint64_t *word_dst = nullptr);

/* ---- optional DC blocker in front of the path (am_dcblock.hip) ---------------------------- */
#define AM_DC_CHIPS 100              /* rx_path.py:40  dc_blocker_cc(100*spc, False) */
unsigned long long am_dcblock_history(int spc);
hipError_t am_launch_dcblock(const float *raw, long long raw_abs0, long long raw_abs1, long long y_abs0, long long y_n,
                             int spc, float *m1, float *y, hipStream_t s);

/* ---- native sample formats (am_resample.hip): n complex samples of AM_FMT_SC16 / CS8 / CU8 at raw (device, aligned to its
 * component) -> 2 n floats at out (device, 8-byte aligned) */
hipError_t am_launch_unpack(int fmt, const void *raw, uint64_t n, float *out, hipStream_t s);

/* ---- preamble detection / refinement / greedy chain ----------------------------------- */
#define AM_DET_THREADS 256
#define AM_DET_PER_THREAD 8
#define AM_DET_PER_BLOCK (AM_DET_THREADS * AM_DET_PER_THREAD)

hipError_t am_launch_detect(const float *bb, const float *avg, uint32_t j0, uint32_t j1, const am_geom &g,
                            float thr_lin, uint32_t *cand_seg, uint32_t *blk_cnt, uint32_t nblk,
                            hipStream_t s);
/* exclusive scan of n counts into off[0..n]; off[n] = total */
hipError_t am_launch_scan_u32(const uint32_t *cnt, uint32_t *off, uint32_t n, hipStream_t s);
/* (in.end_j is not read; r.M exact, r.jump0 not written) */
hipError_t am_launch_refine(const am_refine_in &in, const am_geom &g, const uint32_t *cand_seg, uint32_t seg_stride,
                            const uint32_t *blk_off, uint32_t nblk, const am_records &r, hipStream_t s);
/* greedy chain (am_kernels.hip): step 1 is independent of where the scan starts */
size_t am_chain_scratch_bytes(uint32_t M);
/* have_succ: r.jump0[] was written by the refinement; scalars (or null): its words AM_SW_RESUME and AM_SW_HIT are cleared (what
 * the one-launch form of am_launch_chain_visit starts from) */
hipError_t am_launch_chain_prepare(const am_records &r, uint32_t *scratch, int want_last, int have_succ, uint32_t *scalars,
                                   hipStream_t s);
/* where the greedy scan of a time shard starts: composed on the device from everybody's exit tables (am_k_cblk_walk) */
struct am_entry_src {
    const am_shard_exit *msgs = nullptr;      // null: the start position comes from the host
    uint32_t world = 0, rank = 0, cap = 0;
    uint64_t base_abs = 0;          // absolute index of the chunk's array coordinate 0
    uint32_t *flags = nullptr;      // flags[0] = 1: repeat the step
    uint64_t *exit_out = nullptr;   // where the scan leaves this chunk (absolute): the next step's message carries it
    uint64_t *carry_out = nullptr;  // non-null: where the scan leaves the step's LAST chunk (composed through all ranks' tables), for the next step
    const uint64_t *cur_in = nullptr;   // non-null: where the scan left the chunk BEFORE this one, read when the entry is composed (am_spipe)
};

/* What the scan does with the candidates it visits (preamble_impl.cc:209-237).  The marking kernels take this struct BY VALUE: its
 * layout is part of their signature.  The caller of am_launch_chain_visit fills everything but the record pointers and
 * ticket_base, which the launcher sets from its am_records and from *ticket_base. */
struct am_emit_args {
    const uint8_t *valid;
    const uint32_t *pos, *e, *tgt;
    const float *inavg;             // reference level of every candidate (goes into the hit records)
    uint32_t emit_max;              // room rule (:212): a valid hit too close to the end of the stream is not
                                    // emitted (and nothing after it can be)
    uint32_t own_lo, own_hi;        // first-stage positions this GPU's time chunk owns (everything on one GPU)
    uint4 *emit_idx;                // out: the candidates to extract, in position order: {candidate index, first-stage position,
                                    // refined position, reference level (bits)} -- everything the extraction kernels need of a hit
                                    // in ONE load (round 5: index -> e / inavg / pos was a dependent memory round trip per hit)
    uint32_t *n_out;                // out: how many
    unsigned long long *slots;      // chained scan of the per-block hit counts (am_chain_prefix)
    uint32_t epoch;
    uint32_t *ticket;               // ... and the counter its places are drawn from (am_chain_place)
    uint32_t ticket_base;
    uint32_t *scalars;              // [AM_SW_RESUME]: raised to the largest resume target of a visited candidate
    int want_resume;
};
enum { AM_WALK_AUTO = 0, AM_WALK_SEPARATE = 1, AM_WALK_FUSED = 2 };   /* walk_mode: test builds force a form (AIRMODES_WALK) */
/* ... and what the walk in front of the marking is asked for */
struct am_walk_req {
    uint32_t cur0;                      /* where the scan starts (array coordinate), unless entry_src composes it                  */
    uint32_t *scratch;                  /* am_chain_scratch_bytes(M), as am_launch_chain_prepare left it                            */
    const am_entry_src *entry_src;      /* or null                                                                                  */
    hipEvent_t after_walk;              /* or null: recorded behind the walk's launch                                               */
    unsigned long long *entry_slots;    /* one 64-bit word per block, zero at allocation, tagged with ea.epoch like ea.slots -- given,
                                           and with neither an entry source nor a walk event, walk and marking are ONE launch whenever
                                           its workgroups are resident at once; null: two launches                                  */
    int walk_mode;
};
/* *ticket_base: the value ea.ticket has when this launch starts (advanced by the grid size); *fused_out (or null): which form ran */
hipError_t am_launch_chain_visit(const am_records &r, const am_emit_args &ea, const am_walk_req &w, uint32_t *ticket_base,
                                 int *fused_out, hipStream_t s);
/* exit table of a time chunk.  header (or null): the message header in front of the table, header[1] = {*carry, 0}: where the scan
 * left this chunk a step ago */
struct am_exit_dst {
    am_shard_exit *table;
    am_shard_exit *header;
    const uint64_t *carry;
};
/* lead_end (array coordinate): the table is only needed up to the first candidate at or past it */
hipError_t am_launch_chain_exit_table(const am_records &r, uint32_t n, uint32_t lead_end, uint32_t *scratch, uint64_t base_abs,
                                      const am_exit_dst &dst, hipStream_t s);
/* device-side am_shard_entry2: es.world messages of AM_SHARD_MSG_HEADER + es.cap entries; writes the array coordinate at which the
 * scan enters chunk es.rank (cur0_out), the absolute position at which it leaves it, and sets es.flags[0] if some table did not fit */
hipError_t am_launch_shard_entry(const am_entry_src &es, uint32_t *cur0_out, hipStream_t s);
/* the header of a message without a table: {0, 0}, {*carry, 0} */
hipError_t am_launch_shard_header(am_shard_exit *header, const uint64_t *carry, hipStream_t s);

/* ---- burst extraction + slicer + CRC --------------------------------------------------- */
/* "rx_time" stream tag (lib/preamble_impl.cc:165-170): from item `offset` on, time = (secs, frac) +
 * (item - offset) / rate */
struct am_time_tag {
    uint64_t offset;
    uint64_t secs;
    double frac;
};
#define AM_MAX_TIME_TAGS 4096
/* What the three slicing launches write, and which instantiation runs.  packets[i].reserved[0] = 1 when the reference would post
 * the message, else 0.
 * fix_bits: which instantiation am_k_*<FIX> runs -- 0 = the kernels as they are without the repair; 1, 2 = DF11 / DF17 replies with
 * up to that many wrong bits are repaired (am_set_fix_errors) and the number flipped is left in reserved[1].
 * gate: 1 = am_k_*<FIX, 1>, which also leaves an am_gate_rec per hit at the address in scalars[AM_SW_GATE_REC] (scalars must not be
 * null then); 2 = am_k_*<FIX, 2>: the same, and an address/parity record carries its DF (am_k_gate_repair); 0 = the kernels as they
 * are without the gate.
 * long_mask: am_set_long_formats' mask; non-zero = am_k_*<FIX, GATE, 1>, which reads the enabled formats from
 * scalars[AM_SW_LONG_FMT] (the host has written them there on the same stream); 0 = the kernels as they are without the option.
 * NO MEMBER HAS AN INITIALISER, and no site value-initialises one of these ("am_slice_out o = {};"): a silent 0 in fix_bits,
 * gate or long_mask would run a scan without the option and nobody would notice.  Each of the two sites that build one
 * (chain_finish, am_slicer_work) assigns the first nine members by name, in this order, so that a missing one shows when the
 * site is read; the last three -- fix_bits, gate, long_mask -- are assigned by slice_options (am_capi.hip), from the context's
 * am_decode_opts, at both sites. */
struct am_slice_out {
    const uint32_t *n_ptr;     /* device-side number of hits                                                     */
    uint32_t n_max;            /* upper bound used for the grid                                                  */
    float *bursts_out;         /* the extraction launches: [n_max][AM_BURST], or null (am_launch_slice: unused)   */
    am_tag *tags_out;          /* likewise                                                                       */
    const uint32_t *crc_pow;
    am_packet *packets;
    const uint32_t *scalars;   /* the context's device block (AM_SW_*)                                           */
    uint32_t *host_out;        /* the context's pinned block (AM_PW_*), or null                                  */
    const uint32_t *Mp;        /* or null: the scan's device-side candidate count, for host_out[AM_PW_CANDIDATES] */
    int fix_bits;
    int gate;
    int long_mask;
};
/* the time tags of the extraction launches: tt[0..ntt) device array in ascending offset order */
struct am_stamp {
    uint64_t base_abs;         /* absolute index of array coordinate 0                                           */
    uint64_t rate;
    const am_time_tag *tt;
    uint32_t ntt;
};
/* extraction + slicing of the emitted preambles in one launch, from dense bb.  chip_idx: device table of the 240 soft chips' sample
 * offsets int(j * samples per chip) (null: j * spc); hist0: history items of the preamble block (the tag's item count = stream
 * index + hist0) */
struct am_dense_src {
    const float *bb;
    const int *chip_idx;
    int hist0;
    long long e_off;
};
/* (emit_idx: one 16-byte record per hit, as am_emit_args describes) */
hipError_t am_launch_extract_slice(const am_records &r, const am_dense_src &src, int spc, const uint4 *emit_idx, const am_stamp &st,
                                   const am_slice_out &o, hipStream_t s);
/* the same when bb exists only around the candidates: the burst is recomputed from IQ (iq[0] = absolute sample src_abs0) */
struct am_iq_src {
    const void *iq;
    int fmt;                   /* AM_FMT_* of iq; other than AM_FMT_CF32: am_k_extract_slice_iq<SPC, ..., 1> */
    long long src_abs0, src_abs1;
    int use_pmf;
    float s1;
    int spc;
};
hipError_t am_launch_extract_slice_iq(const am_records &r, const am_iq_src &src, const uint4 *emit_idx, const am_stamp &st,
                                      const am_slice_out &o, hipStream_t s);
/* slicing alone, of bursts and tags that exist */
hipError_t am_launch_slice(const float *bursts, const am_tag *tags, const am_slice_out &o, hipStream_t s);

/* ---- address gate (am_set_address_gate; am_gate.inc) ----------------------------------------------------
 * One record per hit index, written by lane 0 of the slicing wave (am_slice_wave<FIX, 1>) into DEVICE memory: the packet
 * array is pinned host memory, which a kernel does not read back. */
struct am_gate_rec {
    unsigned long long sample;   /* am_packet.sample (for K streams: still in the coordinates of the scanned buffer)          */
    uint32_t addr;               /* teach: data[1..3], big-endian; test: the syndrome (<FIX, 2>: and the DF in bits 24..28)   */
    uint32_t cls;                /* AM_GC_*                                                                                   */
};
#define AM_GC_NONE 0u    /* rejected by the slicer, or kept without a part in the gate (a repaired DF11 / DF17 reply)          */
#define AM_GC_TEACH 1u   /* DF11 / DF17, syndrome 0 as sliced: teaches its address, kept                                       */
#define AM_GC_TEST 2u    /* DF0/4/5/16/20/21: kept iff the address was taught at most ttl item counts before                   */
#define AM_GC_OTHER 3u   /* any other format: mode 1 keeps it, mode 2 drops it                                                 */
#define AM_GATE_MAP_SLOTS (1u << 18)   /* the context's map; three quarters may be taken: 196 608 addresses alive               */
struct am_gate_args {
    const am_gate_rec *rec;
    const uint32_t *n_ptr;               /* device-side record count, or null: n                                               */
    uint32_t n;
    uint32_t K;                          /* streams in the scan (am_process_multi), 0: one                                      */
    const unsigned long long *moff;      /* [K] where stream j starts in the scanned buffer                                     */
    const long long *mem;                /* [K] the last position it may emit, -1: none                                         */
    unsigned long long hist0;
    unsigned long long ttl;              /* window in item counts, >= 1                                                         */
    int mode;
    unsigned long long *cnt;             /* the call's table: [0] taught [1] passed [2] dropped, then owner / first / last      */
    unsigned long long *s_owner, *s_first, *s_last;
    uint32_t s_mask;
    unsigned long long *t_hdr;           /* the context's map: [0] slots taken, [1] addresses not learned                       */
    unsigned long long *t_key, *t_last;
    uint32_t t_mask;
    unsigned long long t_limit;
    am_packet *packets;
    uint32_t *rl;                        /* am_set_address_repair: [0] entries [1] repaired [2] ambiguous, from [AM_GATE_RL_HDR]  */
    const uint32_t *crc_pow;             /* the hit indices of the failed address/parity records; null: no repair                 */
};
#define AM_GATE_RL_HDR 4u
size_t am_gate_scratch_bytes(uint32_t slots);                                   /* slots: a power of two                      */
void am_gate_scratch_layout(am_gate_args &a, void *scratch, uint32_t slots);
hipError_t am_launch_gate(const am_gate_args &a, uint32_t n_max, hipStream_t s);   /* zero the call's table, teach, test     */
                                                                                   /* (a.rl: and repair)                      */
hipError_t am_launch_gate_commit(const am_gate_args &a, hipStream_t s);            /* a.n records of an ACCEPTED scan         */
/* a chunk of am_spipe: the records a.n_ptr counts on the device (at most a.n) enter the map a.t_* at once  */
hipError_t am_launch_gate_commit_running(const am_gate_args &a, hipStream_t s);
/* the completion ticket of a gated scan.  pin: the context's pinned block -- pin[AM_PW_TICKET] = seq, pin[AM_PW_GATE_TAUGHT ..
 * AM_PW_GATE_DROPPED] = taught, passed, dropped; rl (a.rl, or null): pin[AM_PW_REPAIRED], pin[AM_PW_AMBIGUOUS];
 * flag_src / word_src (am_spipe; as am_launch_ticket's): these device words come along, to pin[AM_PW_FLAG] and pin[AM_PW_EXIT] */
hipError_t am_launch_gate_ticket(uint32_t *pin, uint32_t seq, const unsigned long long *cnt, const uint32_t *rl, hipStream_t s,
                                 const uint32_t *flag_src = nullptr, const uint64_t *word_src = nullptr);

#endif
