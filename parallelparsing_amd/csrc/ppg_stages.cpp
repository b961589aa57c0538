// ppg_stages.cpp — the record stages of libppgpu.so: work on a batch of a shard while its output is resident
// on the GPU.  Packed reads (ppg_seqpack.hip), sequence query (ppg_seqquery.hip), read filter
// (ppg_readfilter.hip), read trim (ppg_readtrim.hip), read dedup (ppg_readdedup.hip), read profile
// (ppg_readprofile.hip) and record selection (ppg_seqselect.hip): for each its
// pieces on one batch, its C entry points (one-shot on a one-batch shard, the hook of every batch of a
// run, and what the last run left) and the measurement hook of its tools/*_probe.py.  The pair overlap
// (ppg_pairoverlap.hip) is here as well: it has no batch, it reads two packed read sets the pack stage wrote; so is
// the pair merge (ppg_pairmerge.hip), which makes a third packed read set from those two and the overlap's rows, and
// the k-mer counter (ppg_kmercount.hip), which counts one packed read set's k-mers into a table of the caller's.
//
// A batch's hooks run from one place, shard_batch_hooks, called once by batch_collect (ppg_api.cpp).  The
// unit kernels of query, filter, trim, dedup and profile read one layout of the batch (StageLayout, ppg_host.h), which
// their caller makes with shard_layout once per batch before the first of them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <algorithm>

#include "../../include/ppgpu.h"
#include "ppg_device.h"
#include "ppg_host.h"
#include "ppg_launch.h"

// the result structs are the kernels' accumulators in order; the chunk counts follow them in pinned memory
static_assert(sizeof(ppg_seq_query_result) == 8 * 8 && sizeof(ppg_read_filter_result) == 8 * kRfAcc &&
                  sizeof(ppg_read_trim_result) == 8 * kRtAcc && sizeof(ppg_read_profile_result) == 8 * kRpFixed &&
                  sizeof(ppg_read_profile) == sizeof(PpgReadProfile) && PPG_PROFILE_MAX_POS == kRpMaxPos &&
                  sizeof(ppg_read_dedup_result) == 8 * kDdAcc && sizeof(ppg_read_dedup) == sizeof(PpgReadDedup) &&
                  sizeof(ppg_pair_overlap_result) == 8 * kPoAcc && sizeof(ppg_pair_overlap) == sizeof(PpgPairOverlap) &&
                  sizeof(ppg_packed_view) == sizeof(PpgPackedView) && PPG_OVERLAP_MAX_LEN == kPoMaxLen &&
                  PPG_OVERLAP_HIST == kPoHist && sizeof(ppg_pair_merge_result) == 8 * kPmAcc &&
                  sizeof(ppg_pair_merge) == sizeof(PpgPairMerge) && sizeof(ppg_pair_merge) == 64 && sizeof(PpgMergeRec) == 32 &&
                  sizeof(ppg_kmer_count_result) == 8 * kKmAcc && sizeof(ppg_kmer_count) == sizeof(PpgKmerCount) &&
                  sizeof(ppg_kmer_count) == 64 && PPG_KMER_SPECTRUM == kKmSpectrum,
              "a stage's result struct is its accumulators");

static bool seq_linked() {   // (weak references, ppg_launch.h: absent from the host-only sanitizer build)
    return ppg_launch_seq_totals && ppg_launch_seq_scan && ppg_launch_seq_offsets && ppg_launch_seq_pack;
}

static bool seqquery_linked() {
    return seq_linked() && ppg_launch_seq_query && ppg_launch_seq_query_chunks && ppg_launch_seq_query_totals;
}

static bool readfilter_linked() {
    return seq_linked() && ppg_launch_rf_measure && ppg_launch_rf_decide && ppg_launch_rf_totals;
}

static bool readtrim_linked() {
    return seq_linked() && ppg_launch_rt_measure && ppg_launch_rt_decide && ppg_launch_rt_totals && ppg_launch_rt_gather;
}

static bool readprofile_linked() {
    return seq_linked() && ppg_launch_rp_measure && ppg_launch_rp_finish && ppg_launch_rp_totals;
}

static bool readdedup_linked() {
    return seq_linked() && ppg_launch_dd_init && ppg_launch_dd_measure && ppg_launch_dd_insert && ppg_launch_dd_decide &&
           ppg_launch_dd_levels && ppg_launch_dd_totals;
}

static bool select_linked() {
    return ppg_launch_sel_count && ppg_launch_sel_scan && ppg_launch_sel_place && ppg_launch_sel_copy;
}

PpgBatchView batch_view(const ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs) {
    return PpgBatchView{sh->out.p, sh->jobs.p + b0, sh->res.p + b0, sh->offs.p, sh->oref.p + b0, sh->info.p + b0,
                        sh->base.p + b0, recs, b1 - b0};
}

// a one-batch shard after its run, as the one-shot entry points and the probes take it: all of it
static PpgBatchView whole_view(const ppg_shard *sh) { return batch_view(sh, 0, sh->n, sh->recs.p); }

// Zero the mask words whose first bit belongs to records [bit0, bit0 + tot): a batch's words, and the
// words of every batch after it; the word a batch shares with the one before it was cleared by that batch.
static hipError_t clear_batch_words(hipStream_t s, uint32_t *words, uint64_t bit0, uint64_t tot) {
    const uint64_t w0 = (bit0 + 31) / 32, w1 = (bit0 + tot + 31) / 32;
    return w1 > w0 ? hipMemsetAsync(words + w0, 0, 4 * (size_t)(w1 - w0), s) : hipSuccess;
}

// the accumulators (acc_n values, zeroed by a run's first batch) and the pinned block of a stage
static int stage_out_begin(ppg_shard *sh, StageOut &o, int acc_n, bool first) {
    HIPCHK(o.acc.alloc((size_t)acc_n));
    HIPCHK(o.host.alloc(8 * ((size_t)acc_n + (size_t)sh->n)));
    if (first) HIPCHK(hipMemsetAsync(o.acc.p, 0, 8 * (size_t)acc_n, shard_stream(sh)));
    return PPG_OK;
}

// ---- the layout (ppg_seqpack.hip) ----
int shard_seq_reserve(ppg_shard *sh, int64_t nchunks) {
    HIPCHK(sh->lay.ctot.alloc((size_t)nchunks + 1));
    HIPCHK(sh->lay.cbase.alloc((size_t)nchunks + 1));
    HIPCHK(sh->lay.htot.alloc(8));
    return PPG_OK;
}

int shard_seq_layout(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t *total) {
    hipStream_t s = shard_stream(sh);
    if (!seq_linked()) return PPG_UNSUPPORTED;
    if (int rc = shard_seq_reserve(sh, std::max<int64_t>(b1 - b0, sh->n))) return rc;   // once: every batch fits
    HIPCHK(ppg_launch_seq_totals(s, batch_view(sh, b0, b1, recs), sh->lay.ctot.p));
    HIPCHK(ppg_launch_seq_scan(s, sh->lay.ctot.p, sh->lay.cbase.p, (uint64_t *)sh->lay.htot.p, b1 - b0));
    HIPCHK(hipStreamSynchronize(s));
    *total = sh->lay.total = (int64_t)*(volatile uint64_t *)sh->lay.htot.p;
    return PPG_OK;
}

int shard_layout(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t tot) {
    int64_t total = 0;
    if (int rc = shard_seq_layout(sh, b0, b1, recs, &total)) return rc;
    HIPCHK(grow_buf(sh->lay.off, (size_t)tot + 1));
    HIPCHK(grow_buf(sh->lay.len, (size_t)tot + 1));
    HIPCHK(ppg_launch_seq_offsets(shard_stream(sh), batch_view(sh, b0, b1, recs), sh->lay.cbase.p, 0, sh->lay.off.p,
                                  sh->lay.len.p));
    return PPG_OK;
}

// ---- packed reads (ppg_seqpack.hip) ----
int shard_seq_pack(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t carry, int64_t total,
                   int64_t *seq_off, uint32_t *seq_len, uint32_t *bases, uint32_t *mask, uint8_t *qual) {
    hipStream_t s = shard_stream(sh);
    const PpgBatchView v = batch_view(sh, b0, b1, recs);
    if (!seq_linked()) return PPG_UNSUPPORTED;
    HIPCHK(ppg_launch_seq_offsets(s, v, sh->lay.cbase.p, carry, seq_off, seq_len));
    HIPCHK(ppg_launch_seq_pack(s, v, sh->lay.cbase.p, seq_off, seq_len, carry, (uint64_t)total, bases, mask, qual));
    return PPG_OK;
}

// the pack hook: the batch's tot records go to shard record numbers [total_records, + tot), their bases
// continue from the batches before.  Nothing is written when a cap would be exceeded.
static int pack_hook(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t tot) {
    PackStage &p = sh->pack;
    int64_t total = 0;
    if (int rc = shard_seq_layout(sh, b0, b1, recs, &total)) return rc;
    if (sh->total_records + tot > p.rec_cap || p.total + total > p.base_cap) return PPG_BUF_ERROR;
    if (int rc = shard_seq_pack(sh, b0, b1, recs, p.total, total, p.off + sh->total_records, p.len + sh->total_records,
                                p.bases, p.mask, p.qual))
        return rc;
    p.total += total;
    return PPG_OK;
}

// ---- sequence queries (ppg_seqquery.hip) ----
int shard_seq_query(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                    const PpgSeqPattern &pat, int32_t m, uint32_t *mask, bool first) {
    hipStream_t s = shard_stream(sh);
    const PpgBatchView v = batch_view(sh, b0, b1, recs);
    QueryStage &q = sh->query;
    if (!seqquery_linked()) return PPG_UNSUPPORTED;
    if (int rc = stage_out_begin(sh, q, 8, first)) return rc;
    // the hit bits: the caller's mask at the shard record number, else (a pattern, no mask) scratch
    // at the batch's record number; a census alone with no mask needs none
    uint32_t *words = mask;
    uint64_t bit0 = (uint64_t)rec0;
    if (!mask && m > 0) {
        HIPCHK(grow_buf(q.bits, (size_t)tot / 32 + 1));
        words = q.bits.p;
        bit0 = 0;
    }
    if (words) HIPCHK(clear_batch_words(s, words, bit0, (uint64_t)tot));
    HIPCHK(ppg_launch_seq_query(s, v, sh->lay.cbase.p, sh->lay.off.p, sh->lay.len.p, (uint64_t)sh->lay.total, &pat, m, words,
                                bit0, q.acc.p));
    HIPCHK(ppg_launch_seq_query_chunks(s, v, m, words, bit0, q.acc.p, q.result() + 8 + b0));
    HIPCHK(ppg_launch_seq_query_totals(s, q.acc.p, q.result()));
    return PPG_OK;
}

// m bytes of pattern (NULL: m = 0) as the kernel's argument; false for a length outside [0, 64] or a '\n'
bool seqquery_pattern(const uint8_t *pattern, int32_t m, PpgSeqPattern *pat) {
    if (m < 0 || m > 64 || (m > 0 && !pattern)) return false;
    memset(pat, 0, sizeof *pat);
    for (int32_t i = 0; i < m; i++) {
        if (pattern[i] == '\n') return false;
        pat->w[i >> 3] |= (uint64_t)pattern[i] << (8 * (i & 7));
    }
    return true;
}

static bool seqquery_mask_ok(const uint32_t *mask, int64_t rec_cap) {
    return rec_cap >= 0 && rec_cap % 32 == 0 && ((uintptr_t)mask & 3) == 0 && (mask != nullptr || rec_cap == 0);
}

// ---- read filters (ppg_readfilter.hip) ----
// the rules of include/ppgpu.h "read filters"; host only
static bool readfilter_ok(const void *filter, PpgReadFilter *out) {
    if (!filter) return false;
    PpgReadFilter f;
    memcpy(&f, filter, sizeof f);
    if (f.criteria & ~(int64_t)0x10F) return false;
    if (f.min_len < 0 || f.max_len < -1 || (f.max_len >= 0 && f.max_len < f.min_len)) return false;
    if ((f.criteria & 2) && f.max_other < 0) return false;
    if (f.qual_base < 0 || f.qual_base > 255) return false;
    if (f.low_q < 0 || f.low_q > 256 || f.qual_base + f.low_q > 256) return false;
    if (f.max_low_milli < 0 || f.max_low_milli > 1000) return false;
    if (f.min_mean_milli > 255000 || f.min_mean_milli < -255000) return false;
    if (out) *out = f;
    return true;
}

static bool readfilter_bufs_ok(const PpgReadFilter &f, const uint32_t *mask, int64_t rec_cap, const uint8_t *metrics,
                               int64_t metrics_cap) {
    if (!seqquery_mask_ok(mask, rec_cap) || ((f.criteria & 0x100) && !mask)) return false;
    return metrics_cap >= 0 && ((uintptr_t)metrics & 7) == 0 && (metrics != nullptr || metrics_cap == 0);
}

int shard_read_filter(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                      const PpgReadFilter &flt, uint32_t *mask, uint8_t *metrics, bool first) {
    hipStream_t s = shard_stream(sh);
    const PpgBatchView v = batch_view(sh, b0, b1, recs);
    FilterStage &f = sh->filter;
    if (!readfilter_linked()) return PPG_UNSUPPORTED;
    HIPCHK(grow_buf(f.rsc, 2 * ((size_t)tot + 1)));
    if (int rc = stage_out_begin(sh, f, kRfAcc, first)) return rc;
    if (tot) HIPCHK(hipMemsetAsync(f.rsc.p, 0, 16 * (size_t)tot, s));
    // as the query: this batch's words.  (AND_MASK changes this batch's bits alone.)
    if (mask && !(flt.criteria & 0x100)) HIPCHK(clear_batch_words(s, mask, (uint64_t)rec0, (uint64_t)tot));
    HIPCHK(ppg_launch_rf_measure(s, v, sh->lay.cbase.p, sh->lay.off.p, sh->lay.len.p, (uint64_t)sh->lay.total,
                                 (uint32_t)(flt.qual_base + flt.low_q), f.rsc.p, f.acc.p, f.hist));
    HIPCHK(ppg_launch_rf_decide(s, v, f.rsc.p, &flt, mask, (uint64_t)rec0, metrics, f.acc.p, f.result() + kRfAcc + b0));
    HIPCHK(ppg_launch_rf_totals(s, f.acc.p, f.result()));
    return PPG_OK;
}

// ---- read trimming (ppg_readtrim.hip) ----
// the rules of include/ppgpu.h "read trimming"; host only
bool readtrim_ok(const void *trim, PpgReadTrim *out) {
    if (!trim) return false;
    ppg_read_trim t;
    memcpy(&t, trim, sizeof t);
    if (t.ops & ~(int64_t)0x10F) return false;
    if (t.head < 0 || t.tail < 0 || t.min_len < 0) return false;
    if (t.qual_base < 0 || t.qual_base > 255) return false;
    const int64_t q[3] = {t.lead_q, t.trail_q, t.win_q};
    for (int i = 0; i < 3; i++)
        if ((t.ops & (1 << i)) && (q[i] < 0 || q[i] > 256 || t.qual_base + q[i] > 256)) return false;
    if ((t.ops & 4) && (t.win_size < 1 || t.win_size > 32)) return false;
    if (t.ops & 8) {
        if (t.adapter_len < 1 || t.adapter_len > 64) return false;
        for (int64_t i = 0; i < t.adapter_len; i++)
            if (t.adapter[i] == '\n') return false;
        if (t.min_overlap < 1 || t.min_overlap > t.adapter_len) return false;
        if (t.max_err_milli < 0 || t.max_err_milli > 1000) return false;
    }
    if (out) {
        *out = PpgReadTrim{t.ops, t.head, t.tail, t.qual_base, t.lead_q, t.trail_q, t.win_size, t.win_q, t.min_overlap,
                           t.max_err_milli, t.min_len, t.adapter_len, {}};
        for (int i = 0; i < 64; i++) out->adapter[i >> 2] |= (uint32_t)t.adapter[i] << (8 * (i & 3));
    }
    return true;
}

static bool readtrim_bufs_ok(const PpgReadTrim &t, const uint32_t *mask, int64_t rec_cap, const void *rows, int64_t rows_cap) {
    if (!seqquery_mask_ok(mask, rec_cap) || ((t.ops & 0x100) && !mask)) return false;
    return rows_cap >= 0 && ((uintptr_t)rows & 7) == 0 && (rows != nullptr || rows_cap == 0);
}

// the scratch planes' "none found": all ones for the three minima, 0 for the maximum
static hipError_t readtrim_scratch_init(hipStream_t s, uint32_t *rsc, int64_t tot) {
    if (!tot) return hipSuccess;
    const hipError_t e = hipMemsetAsync(rsc, 0xFF, 12 * (size_t)tot, s);
    return e != hipSuccess ? e : hipMemsetAsync(rsc + 3 * (size_t)tot, 0, 4 * (size_t)tot, s);
}

int shard_read_trim(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                    const PpgReadTrim &trm, uint32_t *mask, uint32_t *rows, bool first) {
    hipStream_t s = shard_stream(sh);
    const PpgBatchView v = batch_view(sh, b0, b1, recs);
    TrimStage &t = sh->trim;
    if (!readtrim_linked()) return PPG_UNSUPPORTED;
    HIPCHK(grow_buf(t.rsc, 4 * ((size_t)tot + 1)));
    if (int rc = stage_out_begin(sh, t, kRtAcc, first)) return rc;
    HIPCHK(readtrim_scratch_init(s, t.rsc.p, tot));
    // as the filter: this batch's words; AND_MASK changes its bits alone
    if (mask && !(trm.ops & 0x100)) HIPCHK(clear_batch_words(s, mask, (uint64_t)rec0, (uint64_t)tot));
    HIPCHK(ppg_launch_rt_measure(s, v, sh->lay.cbase.p, sh->lay.off.p, sh->lay.len.p, (uint64_t)sh->lay.total, &trm, t.rsc.p,
                                 (uint64_t)tot));
    HIPCHK(ppg_launch_rt_decide(s, v, t.rsc.p, (uint64_t)tot, &trm, mask, (uint64_t)rec0, rows, t.acc.p,
                                t.result() + kRtAcc + b0));
    HIPCHK(ppg_launch_rt_totals(s, t.acc.p, t.result()));
    return PPG_OK;
}

// ---- read profile (ppg_readprofile.hip) ----
// the rules of include/ppgpu.h "read profile"; host only
static bool readprofile_ok(const void *profile, PpgReadProfile *out) {
    if (!profile) return false;
    PpgReadProfile p;
    memcpy(&p, profile, sizeof p);
    if (p.flags & ~(int64_t)(PPG_PROFILE_USE_MASK | PPG_PROFILE_USE_WINDOWS)) return false;
    if (p.qual_base < 0 || p.qual_base > 255) return false;
    if (p.max_pos < 1 || p.max_pos > kRpMaxPos || p.reserved != 0) return false;
    if (out) *out = p;
    return true;
}

// each flag with its buffer and each buffer with its flag
static bool readprofile_bufs_ok(const PpgReadProfile &p, const uint32_t *mask, int64_t mask_cap, const void *rows,
                                int64_t rows_cap) {
    if (!seqquery_mask_ok(mask, mask_cap) || ((p.flags & PPG_PROFILE_USE_MASK) != 0) != (mask != nullptr)) return false;
    if (((p.flags & PPG_PROFILE_USE_WINDOWS) != 0) != (rows != nullptr)) return false;
    return rows_cap >= 0 && ((uintptr_t)rows & 7) == 0 && (rows != nullptr || rows_cap == 0);
}

int shard_read_profile(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                       const PpgReadProfile &prf, const uint32_t *mask, const uint32_t *rows, bool first) {
    hipStream_t s = shard_stream(sh);
    const PpgBatchView v = batch_view(sh, b0, b1, recs);
    ProfileStage &p = sh->profile;
    if (!readprofile_linked()) return PPG_UNSUPPORTED;
    if (!p.cus) HIPCHK(hipDeviceGetAttribute(&p.cus, hipDeviceAttributeMultiprocessorCount, sh->ctx->device));
    HIPCHK(grow_buf(p.rsc, 2 * ((size_t)tot + 1)));
    p.out_pos = prf.max_pos;
    if (int rc = stage_out_begin(sh, p, (int)p.values(), first)) return rc;
    if (tot) HIPCHK(hipMemsetAsync(p.rsc.p, 0, 16 * (size_t)tot, s));
    HIPCHK(ppg_launch_rp_measure(s, v, sh->lay.cbase.p, sh->lay.off.p, sh->lay.len.p, (uint64_t)sh->lay.total, &prf, mask,
                                 rows, (uint64_t)rec0, p.rsc.p, p.acc.p, p.grid, p.cus));
    HIPCHK(ppg_launch_rp_finish(s, v, p.rsc.p, &prf, mask, rows, (uint64_t)rec0, p.acc.p, p.result() + p.values() + b0));
    HIPCHK(ppg_launch_rp_totals(s, p.acc.p, p.result(), (uint32_t)p.values()));
    return PPG_OK;
}

// what the last completed profile left in pinned memory (n: the shard's chunks; P: its max_pos); the caller
// has checked the table's cap
static void readprofile_outputs(const ProfileStage &p, int32_t n, int64_t P, int64_t *chunk_profiled, void *result,
                                int64_t *table) {
    const size_t fixed = 8 * (size_t)kRpFixed, rows = 8 * (size_t)kRpRow * (size_t)P;
    if (!p.host.p) {   // a shard without chunks: no batch ran
        if (result) memset(result, 0, fixed);
        if (table) memset(table, 0, rows);
        return;
    }
    if (result) memcpy(result, p.host.p, fixed);
    if (table) memcpy(table, p.host.p + fixed, rows);
    if (chunk_profiled && n) memcpy(chunk_profiled, p.host.p + fixed + rows, 8 * (size_t)n);
}

// ---- read dedup (ppg_readdedup.hip) ----
// the rules of include/ppgpu.h "read dedup"; host only
static bool readdedup_ok(const void *dedup, PpgReadDedup *out) {
    if (!dedup) return false;
    PpgReadDedup d;
    memcpy(&d, dedup, sizeof d);
    if (d.flags & ~(int64_t)(PPG_DEDUP_USE_WINDOWS | PPG_DEDUP_AND_MASK)) return false;
    if (d.max_bases < 0 || d.reserved[0] != 0 || d.reserved[1] != 0) return false;
    if (out) *out = d;
    return true;
}

// AND_MASK with its mask, the windows with their flag and the flag with its windows, the table
static bool readdedup_bufs_ok(const PpgReadDedup &d, const uint32_t *mask, int64_t mask_cap, const void *rows,
                              int64_t rows_cap, const int64_t *first, int64_t first_cap, const uint64_t *table,
                              int64_t slots) {
    if (!seqquery_mask_ok(mask, mask_cap) || ((d.flags & PPG_DEDUP_AND_MASK) && !mask)) return false;
    if (((d.flags & PPG_DEDUP_USE_WINDOWS) != 0) != (rows != nullptr)) return false;
    if (rows_cap < 0 || ((uintptr_t)rows & 7) != 0 || (!rows && rows_cap != 0)) return false;
    if (first_cap < 0 || ((uintptr_t)first & 7) != 0 || (!first && first_cap != 0)) return false;
    return table && ((uintptr_t)table & 7) == 0 && slots >= 64 && (slots & (slots - 1)) == 0;
}

// a cap or the table's load of 1/2 that `after` records of the run would exceed
static bool readdedup_full(const uint32_t *mask, int64_t mask_cap, const void *rows, int64_t rows_cap, const int64_t *first,
                           int64_t first_cap, int64_t slots, int64_t after) {
    return (mask && after > mask_cap) || (rows && after > rows_cap) || (first && after > first_cap) || after > slots / 2;
}

int shard_read_dedup(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                     const PpgReadDedup &dd, uint32_t *mask, const uint32_t *rows, int64_t *first_out, uint64_t *table,
                     int64_t slots, bool first, bool last) {
    hipStream_t s = shard_stream(sh);
    const PpgBatchView v = batch_view(sh, b0, b1, recs);
    DedupStage &d = sh->dedup;
    if (!readdedup_linked()) return PPG_UNSUPPORTED;
    const bool and_mask = (dd.flags & PPG_DEDUP_AND_MASK) != 0;
    HIPCHK(grow_buf(d.rsc, 2 * ((size_t)tot + 1)));
    if (int rc = stage_out_begin(sh, d, kDdAcc, first)) return rc;
    if (first) HIPCHK(ppg_launch_dd_init(s, table, (uint64_t)slots));
    if (tot) HIPCHK(hipMemsetAsync(d.rsc.p, 0, 16 * (size_t)tot, s));
    // as the filter: this batch's words; AND_MASK changes its bits alone
    if (mask && !and_mask) HIPCHK(clear_batch_words(s, mask, (uint64_t)rec0, (uint64_t)tot));
    const uint32_t *part = and_mask ? mask : nullptr;   // the bits that decide participation
    HIPCHK(ppg_launch_dd_measure(s, v, sh->lay.cbase.p, sh->lay.off.p, sh->lay.len.p, (uint64_t)sh->lay.total, &dd, part, rows,
                                 (uint64_t)rec0, d.rsc.p));
    HIPCHK(ppg_launch_dd_insert(s, v, &dd, part, rows, (uint64_t)rec0, d.rsc.p, table, (uint64_t)slots, d.acc.p));
    HIPCHK(ppg_launch_dd_decide(s, v, &dd, rows, (uint64_t)rec0, d.rsc.p, table, mask, first_out, d.acc.p,
                                d.result() + kDdAcc + b0));
    if (last) {   // the levels and the greatest row, once: max_first starts from "none"
        HIPCHK(hipMemsetAsync(d.acc.p + 7, 0xFF, 8, s));
        HIPCHK(ppg_launch_dd_levels(s, table, (uint64_t)slots, d.acc.p));
    }
    HIPCHK(ppg_launch_dd_totals(s, d.acc.p, d.result()));
    return PPG_OK;
}

// what the last completed dedup left in pinned memory (n: the shard's chunks)
static void readdedup_outputs(const DedupStage &d, int32_t n, int64_t *chunk_unique, void *result) {
    d.outputs(n, chunk_unique, result, sizeof(ppg_read_dedup_result));
    if (!d.host.p && result) ((ppg_read_dedup_result *)result)->max_first = -1;   // no batch ran: an empty table
}

// ---- pair overlap (ppg_pairoverlap.hip) ----
// Not a batch's stage: it works on two packed read sets in caller memory, on the ctx stream.
static bool pairoverlap_linked() { return ppg_launch_pair_overlap != nullptr; }

// the rules of include/ppgpu.h "pair overlap"; host only
static bool pairoverlap_ok(const void *overlap, PpgPairOverlap *out) {
    if (!overlap) return false;
    PpgPairOverlap o;
    memcpy(&o, overlap, sizeof o);
    if (o.flags != 0 || o.min_overlap < 1 || o.max_diff < 0 || o.max_err_milli < 0 || o.max_err_milli > 1000) return false;
    for (int64_t r : o.reserved)
        if (r != 0) return false;
    if (out) *out = o;
    return true;
}

// a ppg_packed_view with every plane but qual, aligned as the packed reads are written
static bool packed_view_ok(const void *set, PpgPackedView *out) {
    if (!set) return false;
    memcpy(out, set, sizeof *out);
    return out->seq_off && out->seq_len && out->bases && out->mask && out->records >= 0 &&
           ((uintptr_t)out->seq_off & 7) == 0 && ((uintptr_t)out->seq_len & 3) == 0 && ((uintptr_t)out->bases & 7) == 0 &&
           ((uintptr_t)out->mask & 3) == 0;
}

struct PairOverlapArgs {
    PpgPairOverlap po;
    PpgPackedView s1, s2;
};

// PPG_ARG_ERROR / PPG_BUF_ERROR of ppg_pairs_overlap, before anything is written
static int pairoverlap_args(ppg_ctx *ctx, const void *overlap, const void *set1, const void *set2, const int64_t *rec1,
                            const int64_t *rec2, int64_t npairs, const void *rows, int64_t row_cap, const uint32_t *found,
                            int64_t mask_cap, const void *win1, int64_t win_cap1, const void *win2, int64_t win_cap2,
                            const int64_t *hist, int64_t hist_cap, PairOverlapArgs &a) {
    if (!ctx || !pairoverlap_ok(overlap, &a.po) || !packed_view_ok(set1, &a.s1) || !packed_view_ok(set2, &a.s2)) return PPG_ARG_ERROR;
    if (npairs < 0 || row_cap < 0 || mask_cap < 0 || mask_cap % 32 != 0 || win_cap1 < 0 || win_cap2 < 0 || hist_cap < 0)
        return PPG_ARG_ERROR;
    if (((uintptr_t)rec1 & 7) || ((uintptr_t)rec2 & 7) || ((uintptr_t)rows & 15) || ((uintptr_t)found & 3) ||
        ((uintptr_t)win1 & 7) || ((uintptr_t)win2 & 7))
        return PPG_ARG_ERROR;
    if ((!rec1 && npairs > a.s1.records) || (!rec2 && npairs > a.s2.records)) return PPG_ARG_ERROR;   // the identity map
    if ((rows && npairs > row_cap) || (found && npairs > mask_cap) || (win1 && a.s1.records > win_cap1) ||
        (win2 && a.s2.records > win_cap2) || (hist && hist_cap < kPoHist))
        return PPG_BUF_ERROR;
    return PPG_OK;
}

// ---- pair merge (ppg_pairmerge.hip) ----
// As the overlap: two packed read sets in caller memory, on the ctx stream; the output is a third.
static bool pairmerge_linked() {
    return ppg_launch_pm_count && ppg_launch_pm_scan && ppg_launch_pm_place && ppg_launch_pm_emit;
}

// the rules of include/ppgpu.h "pair merge"; host only
static bool pairmerge_ok(const void *merge, PpgPairMerge *out) {
    if (!merge) return false;
    PpgPairMerge m;
    memcpy(&m, merge, sizeof m);
    if (m.flags != 0 || m.qual_lo < 0 || m.qual_hi > 255 || m.qual_lo >= m.qual_hi) return false;
    for (int64_t r : m.reserved)
        if (r != 0) return false;
    if (out) *out = m;
    return true;
}

struct PairMergeArgs {
    PpgPairMerge pm;
    PpgPackedView s1, s2;
    int ntiles;
};

// PPG_ARG_ERROR of both merge entry points for the inputs (and PPG_BUF_ERROR for the rows), before anything runs
static int pairmerge_inputs(ppg_ctx *ctx, const void *set1, const void *set2, const int64_t *rec1, const int64_t *rec2,
                            int64_t npairs, const void *rows, int64_t row_cap, bool quals, PairMergeArgs &a) {
    if (!ctx || !packed_view_ok(set1, &a.s1) || !packed_view_ok(set2, &a.s2)) return PPG_ARG_ERROR;
    if (quals && (!a.s1.qual || !a.s2.qual || ((uintptr_t)a.s1.qual & 15) || ((uintptr_t)a.s2.qual & 15))) return PPG_ARG_ERROR;
    if (npairs < 0 || row_cap < 0 || (!rows && npairs > 0) || npairs > (int64_t)kPmTile * INT32_MAX) return PPG_ARG_ERROR;
    if (((uintptr_t)rec1 & 7) || ((uintptr_t)rec2 & 7) || ((uintptr_t)rows & 15)) return PPG_ARG_ERROR;
    if ((!rec1 && npairs > a.s1.records) || (!rec2 && npairs > a.s2.records)) return PPG_ARG_ERROR;   // the identity map
    if (npairs > row_cap) return PPG_BUF_ERROR;
    a.ntiles = (int)((npairs + kPmTile - 1) / kPmTile);
    return PPG_OK;
}

// the merge's scratch: per tile of pairs the merged records and padded bases and their scans, the totals in
// pinned memory, a PpgMergeRec per merged record, the accumulators
struct PairMergeScratch {
    DevBuf<uint64_t> tiles, acc;
    DevBuf<PpgMergeRec> recs;
    PinnedBuf host;
    uint64_t *trec(int) { return tiles.p; }
    uint64_t *tbase(int n) { return tiles.p + (size_t)n + 1; }
    uint64_t *rbase(int n) { return tiles.p + 2 * ((size_t)n + 1); }
    uint64_t *bbase(int n) { return tiles.p + 3 * ((size_t)n + 1); }
};

// ---- k-mer counts (ppg_kmercount.hip) ----
// As the overlap: one packed read set in caller memory, on the ctx stream; the table is the caller's too.
static bool kmercount_linked() {
    return ppg_launch_km_init && ppg_launch_km_records && ppg_launch_km_insert && ppg_launch_km_stats &&
           ppg_launch_km_select && ppg_launch_km_lookup;
}

// the rules of include/ppgpu.h "k-mer counts"; host only
static bool kmercount_ok(const void *kmers, PpgKmerCount *out) {
    if (!kmers) return false;
    PpgKmerCount c;
    memcpy(&c, kmers, sizeof c);
    if ((c.flags & ~(int64_t)(PPG_KMER_CANONICAL | PPG_KMER_USE_WINDOWS | PPG_KMER_USE_MASK | PPG_KMER_ACCUMULATE)) != 0 ||
        c.k < 1 || c.k > 31)
        return false;
    for (int64_t r : c.reserved)
        if (r != 0) return false;
    if (out) *out = c;
    return true;
}

static bool kmer_table_ok(const void *table, int64_t slots) {
    return table && ((uintptr_t)table & 15) == 0 && slots >= 64 && (slots & (slots - 1)) == 0;
}

struct KmerCountArgs {
    PpgKmerCount kc;
    PpgPackedView set;
};

// PPG_ARG_ERROR / PPG_BUF_ERROR of ppg_kmers_count, before anything is written
static int kmercount_args(ppg_ctx *ctx, const void *kmers, const void *set, const uint32_t *mask, int64_t mask_cap,
                          const void *windows, int64_t windows_cap, const void *table, int64_t slots, const int64_t *spectrum,
                          int64_t spectrum_cap, KmerCountArgs &a) {
    if (!ctx || !kmercount_ok(kmers, &a.kc) || !packed_view_ok(set, &a.set)) return PPG_ARG_ERROR;
    if (mask_cap < 0 || mask_cap % 32 != 0 || windows_cap < 0 || spectrum_cap < 0 || !kmer_table_ok(table, slots)) return PPG_ARG_ERROR;
    if (((uintptr_t)mask & 3) || ((uintptr_t)windows & 7) || a.set.records >= (int64_t)0xFFFFFFFFu) return PPG_ARG_ERROR;
    // a flag without its buffer, a buffer without its flag
    if (((a.kc.flags & PPG_KMER_USE_MASK) != 0) != (mask != nullptr) || ((a.kc.flags & PPG_KMER_USE_WINDOWS) != 0) != (windows != nullptr))
        return PPG_ARG_ERROR;
    if ((mask && a.set.records > mask_cap) || (windows && a.set.records > windows_cap) || (spectrum && spectrum_cap < kKmSpectrum))
        return PPG_BUF_ERROR;
    return PPG_OK;
}

// the call's scratch: the accumulators and the record of every 32-base unit
struct KmerCountScratch {
    DevBuf<uint64_t> acc;
    DevBuf<uint32_t> umap;
    uint64_t units = 0;
};

// the set's 32-base units, from seq_off[records] (one 8-byte copy; blocks)
static int kmercount_units(hipStream_t s, const PpgPackedView &set, uint64_t *units) {
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, set.seq_off + set.records, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total < 0 || total % 32 != 0) return PPG_ARG_ERROR;   // not a packed read set
    *units = (uint64_t)total / 32;
    return PPG_OK;
}

// the accumulators as a pass over the table wants them: all zero, max_key all ones
static hipError_t kmercount_clear(hipStream_t s, uint64_t *acc, bool all) {
    hipError_t e = all ? hipMemsetAsync(acc, 0, 8 * (size_t)kKmAccAll, s) : hipSuccess;
    return e != hipSuccess ? e : hipMemsetAsync(acc + 10, 0xFF, 8, s);
}

// count and scan, queued on s; the totals are in w.host once s has been synchronised
static int pairmerge_count(hipStream_t s, const PairMergeArgs &a, const int64_t *rec1, const int64_t *rec2, int64_t npairs,
                           const void *rows, PairMergeScratch &w) {
    const int n = a.ntiles;
    HIPCHK(w.tiles.alloc(4 * ((size_t)n + 1)));
    HIPCHK(w.host.alloc(16));
    HIPCHK(ppg_launch_pm_count(s, a.s1, a.s2, rec1, rec2, npairs, (const int32_t *)rows, w.trec(n), w.tbase(n)));
    HIPCHK(ppg_launch_pm_scan(s, w.trec(n), w.tbase(n), w.rbase(n), w.bbase(n), (int64_t *)w.host.p, n));
    return PPG_OK;
}

// ---- record selection (ppg_seqselect.hip) ----
int shard_select_reserve(ppg_shard *sh, int64_t nchunks) {
    HIPCHK(sh->select.ccnt.alloc(2 * ((size_t)nchunks + 1)));
    HIPCHK(sh->select.cbase.alloc(2 * ((size_t)nchunks + 1)));
    HIPCHK(sh->select.host.alloc(16));
    return PPG_OK;
}

// the scan of the per-chunk counts of n chunks (records in the first half of ccnt / cbase, bytes in the
// second); the totals into pinned memory
static hipError_t select_scan(ppg_shard *sh, int n) {
    SelectStage &e = sh->select;
    const size_t h = e.ccnt.n / 2;
    return ppg_launch_sel_scan(shard_stream(sh), e.ccnt.p, e.ccnt.p + h, e.cbase.p, e.cbase.p + h, (int64_t *)e.host.p, n);
}

int shard_select_sizes(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, const uint32_t *mask, int64_t bit0,
                       int64_t *records, int64_t *bytes) {
    hipStream_t s = shard_stream(sh);
    SelectStage &e = sh->select;
    if (!select_linked()) return PPG_UNSUPPORTED;
    if (int rc = shard_select_reserve(sh, std::max<int64_t>(b1 - b0, sh->n))) return rc;   // once: every batch fits
    HIPCHK(ppg_launch_sel_count(s, batch_view(sh, b0, b1, recs), mask, (uint64_t)bit0, e.ccnt.p, e.ccnt.p + e.ccnt.n / 2));
    HIPCHK(select_scan(sh, b1 - b0));
    HIPCHK(hipStreamSynchronize(s));
    *records = ((volatile int64_t *)e.host.p)[0];
    *bytes = ((volatile int64_t *)e.host.p)[1];
    return PPG_OK;
}

int shard_select_move(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, const uint32_t *mask, int64_t bit0,
                      int64_t rec_lo, int64_t byte_lo, int64_t records, int64_t bytes, int64_t *recno, int64_t *sel_off,
                      uint32_t *desc, uint8_t *dst) {
    hipStream_t s = shard_stream(sh);
    SelectStage &e = sh->select;
    if (!select_linked()) return PPG_UNSUPPORTED;
    HIPCHK(grow_buf(e.src, (size_t)records + 1));
    HIPCHK(grow_buf(e.span, (size_t)((byte_lo + bytes) / kSelSpan - byte_lo / kSelSpan) + 2));
    HIPCHK(ppg_launch_sel_place(s, batch_view(sh, b0, b1, recs), mask, (uint64_t)bit0, e.cbase.p, e.cbase.p + e.ccnt.n / 2,
                                rec_lo, byte_lo, recno, sel_off, desc, e.src.p, e.span.p));
    HIPCHK(ppg_launch_sel_copy(s, sel_off, e.src.p, e.span.p, rec_lo, rec_lo + records, byte_lo, byte_lo + bytes, dst));
    return PPG_OK;
}

// the select hook: the batch's selected records are appended
static int select_hook(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t tot) {
    SelectStage &e = sh->select;
    if (e.mask && sh->total_records + tot > e.mask_cap) return PPG_BUF_ERROR;
    int64_t S = 0, B = 0;
    if (int rc = shard_select_sizes(sh, b0, b1, recs, e.mask, sh->total_records, &S, &B)) return rc;
    if (e.records + S > e.cap || e.nbytes + B > e.byte_cap) return PPG_BUF_ERROR;
    if (int rc = shard_select_move(sh, b0, b1, recs, e.mask, sh->total_records, e.records, e.nbytes, S, B, e.recno, e.off,
                                   e.desc, e.bytes))
        return rc;
    e.records += S;
    e.nbytes += B;
    return PPG_OK;
}

// ---- a batch's hooks ----
// Everything attached to the shard, on the batch [b0, b1) of tot records that batch_collect has just waited
// for, in the order keys, pack, query, filter, trim, dedup, profile, select.  The batch's output is resident: the
// next batch's inflate follows on the same stream, so it is read before it is overwritten.  A filter with
// AND_MASK on the query's mask sees this batch's hit bits, a trim what both have left of them, a dedup with
// AND_MASK clears all but the first occurrences among those (its table persists from batch to batch), the
// profile reads the mask and the rows as they were left, and the selection, last, hands over the product.  A
// cap that the batch would exceed fails with PPG_BUF_ERROR before the stage writes anything.
int shard_batch_hooks(ppg_shard *sh, int32_t b0, int32_t b1, int64_t tot) {
    if (sh->hooks_off) return PPG_OK;   // a batch run again for the pair emission: the run's outputs stand
    const int64_t rec0 = sh->total_records, after = rec0 + tot;
    const uint32_t *recs = sh->recs.p + 4 * (uint64_t)rec0;
    // The run's first batch, where the accumulators and the selection's totals restart.  The pack's base
    // total restarts while the run has no record yet, which b0 == 0 implies and which adds nothing before.
    const bool first = b0 == 0;
    if (first) sh->select.records = sh->select.nbytes = 0;
    if (rec0 == 0) sh->pack.total = 0;
    if (sh->keys_dev) {   // spot keys (ppg_shard_set_keys)
        if (after > sh->keys_cap) return PPG_BUF_ERROR;
        const PpgBatchView v = batch_view(sh, b0, b1, recs);
        HIPCHK(ppg_launch_record_keys(shard_stream(sh), v.out, v.jobs, v.res, v.offs, v.oref, v.info, v.base, v.recs,
                                      sh->keys_dev + rec0, v.n));
    }
    if (sh->pack.off)   // lays the batch out for itself: its seq_off continues from the batches before
        if (int rc = pack_hook(sh, b0, b1, recs, tot)) return rc;
    const QueryStage &q = sh->query;
    const FilterStage &f = sh->filter;
    const TrimStage &t = sh->trim;
    const DedupStage &d = sh->dedup;
    const ProfileStage &p = sh->profile;
    if (q.on || f.on || t.on || d.on || p.on) {   // the unit kernels' layout, once for the five
        if (q.on && q.mask && after > q.rec_cap) return PPG_BUF_ERROR;
        if (f.on && ((f.mask && after > f.rec_cap) || (f.metrics && after > f.metrics_cap))) return PPG_BUF_ERROR;
        if (t.on && ((t.mask && after > t.rec_cap) || (t.rows && after > t.rows_cap))) return PPG_BUF_ERROR;
        if (d.on && readdedup_full(d.mask, d.mask_cap, d.rows, d.rows_cap, d.first, d.first_cap, d.slots, after))
            return PPG_BUF_ERROR;
        if (p.on && ((p.mask && after > p.mask_cap) || (p.rows && after > p.rows_cap))) return PPG_BUF_ERROR;
        if (int rc = shard_layout(sh, b0, b1, recs, tot)) return rc;
    }
    if (q.on)
        if (int rc = shard_seq_query(sh, b0, b1, recs, rec0, tot, q.pat, q.m, q.mask, first)) return rc;
    if (f.on)
        if (int rc = shard_read_filter(sh, b0, b1, recs, rec0, tot, f.flt, f.mask, f.metrics, first)) return rc;
    if (t.on)
        if (int rc = shard_read_trim(sh, b0, b1, recs, rec0, tot, t.trm, t.mask, t.rows, first)) return rc;
    if (d.on)
        if (int rc = shard_read_dedup(sh, b0, b1, recs, rec0, tot, d.dd, d.mask, d.rows, d.first, d.table, d.slots, first,
                                      b1 == sh->n))
            return rc;
    if (p.on)
        if (int rc = shard_read_profile(sh, b0, b1, recs, rec0, tot, p.prf, p.mask, p.rows, first)) return rc;
    if (sh->select.on)
        if (int rc = select_hook(sh, b0, b1, recs, tot)) return rc;
    return PPG_OK;
}

void stages_run_begin(ppg_shard *sh) {
    sh->keys_written = sh->pack.written = sh->query.written = sh->filter.written = sh->trim.written = sh->profile.written = 0;
    sh->dedup.written = sh->select.written = 0;
}

void stages_run_end(ppg_shard *sh, bool ok) {
    sh->keys_written = ok && sh->keys_dev != nullptr;
    sh->pack.written = ok && sh->pack.off != nullptr;
    sh->query.written = ok && sh->query.on;
    sh->filter.written = ok && sh->filter.on;
    sh->trim.written = ok && sh->trim.on;
    sh->dedup.written = ok && sh->dedup.on;
    sh->profile.written = ok && sh->profile.on;
    sh->select.written = ok && sh->select.on;
}

// ---- the probes' timing loop ----
// Device time of `nsteps` steps by two events on the stream s: ms[step] = the median of `reps` runs of
// launch(step) after one warm-up run.
template <class Launch>
static int time_steps(hipStream_t s, int nsteps, int reps, float *ms, Launch launch) {
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
    std::vector<float> t;
    for (int step = 0; step < nsteps; step++) {
        t.clear();
        for (int r = 0; r <= reps; r++) {
            float v = 0;
            HIPCHK(hipEventRecord(ev.e[0], s));
            HIPCHK(launch(step));
            HIPCHK(hipEventRecord(ev.e[1], s));
            HIPCHK(hipEventSynchronize(ev.e[1]));
            HIPCHK(hipEventElapsedTime(&v, ev.e[0], ev.e[1]));
            if (r) t.push_back(v);   // (r = 0 warms up)
        }
        std::sort(t.begin(), t.end());
        ms[step] = t[t.size() / 2];
    }
    return PPG_OK;
}

// the probes' layout steps, as shard_layout queues them
static hipError_t launch_totals_scan(ppg_shard *sh, hipStream_t s) {
    const hipError_t e = ppg_launch_seq_totals(s, whole_view(sh), sh->lay.ctot.p);
    return e != hipSuccess ? e : ppg_launch_seq_scan(s, sh->lay.ctot.p, sh->lay.cbase.p, (uint64_t *)sh->lay.htot.p, sh->n);
}

static hipError_t launch_offsets(ppg_shard *sh, hipStream_t s, int64_t *off, uint32_t *len) {
    return ppg_launch_seq_offsets(s, whole_view(sh), sh->lay.cbase.p, 0, off, len);
}

// raw_k = offset_k ++ chunk_k of a one-batch shard, as ppg_pack_raw lays the text out: where each starts
static std::vector<int64_t> raw_offsets(const ppg_shard *sh) {
    std::vector<int64_t> raw_off((size_t)sh->n + 1, 0);
    for (int32_t k = 0; k < sh->n; k++)
        raw_off[(size_t)k + 1] = raw_off[(size_t)k] + (int64_t)sh->h_jobs[(size_t)k].raw_shift + (int64_t)sh->h_res[(size_t)k].produced;
    return raw_off;
}

static hipError_t launch_pack_raw(ppg_shard *sh, hipStream_t s, const int64_t *draw, uint8_t *text) {
    return ppg_launch_pack_raw(s, sh->out.p, sh->jobs.p, sh->res.p, sh->offs.p, sh->oref.p, draw, text, sh->n, 0);
}

extern "C" {

// ---- packed reads: the keys entry points' counterparts ----
static bool seq_args_ok(const int64_t *off, const uint32_t *len, int64_t rec_cap, const uint32_t *bases,
                        const uint32_t *mask, const uint8_t *qual, int64_t base_cap) {
    // a unit is stored as one 8-B word of bases and 32 B of qualities: the planes' alignment
    return off && len && bases && mask && rec_cap >= 0 && base_cap >= 0 && base_cap % 32 == 0 &&
           ((uintptr_t)off & 7) == 0 && ((uintptr_t)len & 3) == 0 && ((uintptr_t)bases & 7) == 0 &&
           ((uintptr_t)mask & 3) == 0 && ((uintptr_t)qual & 15) == 0;
}

int ppg_shard_seq_bases(ppg_shard *sh, int64_t *total_bases, int64_t *records) {
    if (!sh || !sh->ran) return PPG_ARG_ERROR;
    if (!seq_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    if (int rc = shard_seq_reserve(sh, sh->n)) return rc;
    // every batch's descriptors are resident, each with record bases relative to its own first record
    for (auto [b0, b1] : sh->batches)
        HIPCHK(ppg_launch_seq_totals(s, batch_view(sh, b0, b1, sh->recs.p + 4 * (uint64_t)sh->h_base[(size_t)b0]),
                                     sh->lay.ctot.p + b0));
    HIPCHK(ppg_launch_seq_scan(s, sh->lay.ctot.p, sh->lay.cbase.p, (uint64_t *)sh->lay.htot.p, sh->n));
    HIPCHK(hipStreamSynchronize(s));
    if (total_bases) *total_bases = (int64_t)*(volatile uint64_t *)sh->lay.htot.p;
    if (records) *records = sh->total_records;
    return PPG_OK;
}

int ppg_shard_pack_seq(ppg_shard *sh, int64_t *dev_seq_off, uint32_t *dev_seq_len, int64_t rec_cap,
                       uint32_t *dev_bases, uint32_t *dev_mask, uint8_t *dev_qual, int64_t base_cap,
                       int64_t *total_bases) {
    if (!sh || !sh->ran || sh->batches.size() != 1 ||
        !seq_args_ok(dev_seq_off, dev_seq_len, rec_cap, dev_bases, dev_mask, dev_qual, base_cap))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    int64_t total = 0;
    if (int rc = shard_seq_layout(sh, 0, sh->n, sh->recs.p, &total)) return rc;
    if (total_bases) *total_bases = total;
    if (sh->total_records > rec_cap || total > base_cap) return PPG_BUF_ERROR;
    if (int rc = shard_seq_pack(sh, 0, sh->n, sh->recs.p, 0, total, dev_seq_off, dev_seq_len, dev_bases, dev_mask,
                                dev_qual))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    return PPG_OK;
}

int ppg_shard_set_seqpack(ppg_shard *sh, int64_t *dev_seq_off, uint32_t *dev_seq_len, int64_t rec_cap,
                          uint32_t *dev_bases, uint32_t *dev_mask, uint8_t *dev_qual, int64_t base_cap) {
    if (!sh) return PPG_ARG_ERROR;
    const bool off = !dev_seq_off && !dev_seq_len && !dev_bases && !dev_mask && !dev_qual && !rec_cap && !base_cap;
    if (!off && !seq_args_ok(dev_seq_off, dev_seq_len, rec_cap, dev_bases, dev_mask, dev_qual, base_cap))
        return PPG_ARG_ERROR;
    PackStage &p = sh->pack;
    p.off = dev_seq_off;
    p.len = dev_seq_len;
    p.bases = dev_bases;
    p.mask = dev_mask;
    p.qual = dev_qual;
    p.rec_cap = rec_cap;
    p.base_cap = base_cap;
    p.written = 0;   // filled by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_seqpack_ready(ppg_shard *sh, int64_t *total_bases) {
    if (!sh) return PPG_ARG_ERROR;
    if (!sh->pack.written) return 0;
    if (total_bases) *total_bases = sh->pack.total;
    return 1;
}

// ---- sequence queries: the packed reads entry points' counterparts ----
int ppg_shard_query_seq(ppg_shard *sh, const uint8_t *pattern, int32_t pattern_len, uint32_t *dev_hit_mask,
                        int64_t rec_cap, int64_t *chunk_hits, void *result) {
    PpgSeqPattern pat;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !seqquery_pattern(pattern, pattern_len, &pat) ||
        !seqquery_mask_ok(dev_hit_mask, rec_cap))
        return PPG_ARG_ERROR;
    if (!seqquery_linked()) return PPG_UNSUPPORTED;
    if (dev_hit_mask && sh->total_records > rec_cap) return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    sh->query.written = 0;   // the pinned outputs are rewritten: an earlier run's hook result is gone
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, sh->total_records)) return rc;
    if (int rc = shard_seq_query(sh, 0, sh->n, sh->recs.p, 0, sh->total_records, pat, pattern_len, dev_hit_mask, true))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    sh->query.outputs(sh->n, chunk_hits, result, sizeof(ppg_seq_query_result));
    return PPG_OK;
}

int ppg_shard_set_seqquery(ppg_shard *sh, const uint8_t *pattern, int32_t pattern_len, uint32_t *dev_hit_mask,
                           int64_t rec_cap) {
    if (!sh) return PPG_ARG_ERROR;
    const bool off = !pattern && pattern_len < 0 && !dev_hit_mask && !rec_cap;
    PpgSeqPattern pat = {};
    if (!off && (!seqquery_pattern(pattern, pattern_len, &pat) || !seqquery_mask_ok(dev_hit_mask, rec_cap)))
        return PPG_ARG_ERROR;
    QueryStage &q = sh->query;
    q.on = off ? 0 : 1;
    q.pat = pat;
    q.m = off ? 0 : pattern_len;
    q.mask = dev_hit_mask;
    q.rec_cap = rec_cap;
    q.written = 0;   // completed by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_seqquery_ready(ppg_shard *sh, int64_t *chunk_hits, void *result) {
    if (!sh) return PPG_ARG_ERROR;
    if (!sh->query.written) return 0;
    sh->query.outputs(sh->n, chunk_hits, result, sizeof(ppg_seq_query_result));
    return 1;
}

// ---- read filters: the sequence queries entry points' counterparts ----
int ppg_read_filter_check(const void *filter) { return readfilter_ok(filter, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

int ppg_shard_filter_reads(ppg_shard *sh, const void *filter, uint32_t *dev_pass_mask, int64_t rec_cap, void *dev_metrics,
                           int64_t metrics_cap, int64_t *chunk_passed, void *result) {
    PpgReadFilter flt;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !readfilter_ok(filter, &flt) ||
        !readfilter_bufs_ok(flt, dev_pass_mask, rec_cap, (const uint8_t *)dev_metrics, metrics_cap))
        return PPG_ARG_ERROR;
    if (!readfilter_linked()) return PPG_UNSUPPORTED;
    if ((dev_pass_mask && sh->total_records > rec_cap) || (dev_metrics && sh->total_records > metrics_cap))
        return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    sh->filter.written = 0;   // the pinned outputs are rewritten: an earlier run's hook result is gone
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, sh->total_records)) return rc;
    if (int rc = shard_read_filter(sh, 0, sh->n, sh->recs.p, 0, sh->total_records, flt, dev_pass_mask,
                                   (uint8_t *)dev_metrics, true))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    sh->filter.outputs(sh->n, chunk_passed, result, sizeof(ppg_read_filter_result));
    return PPG_OK;
}

int ppg_shard_set_readfilter(ppg_shard *sh, const void *filter, uint32_t *dev_pass_mask, int64_t rec_cap, void *dev_metrics,
                             int64_t metrics_cap) {
    if (!sh) return PPG_ARG_ERROR;
    PpgReadFilter flt = {};
    if (filter && (!readfilter_ok(filter, &flt) ||
                   !readfilter_bufs_ok(flt, dev_pass_mask, rec_cap, (const uint8_t *)dev_metrics, metrics_cap)))
        return PPG_ARG_ERROR;
    FilterStage &f = sh->filter;
    f.on = filter ? 1 : 0;
    f.flt = flt;
    f.mask = filter ? dev_pass_mask : nullptr;
    f.rec_cap = filter ? rec_cap : 0;
    f.metrics = filter ? (uint8_t *)dev_metrics : nullptr;
    f.metrics_cap = filter ? metrics_cap : 0;
    f.written = 0;   // completed by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_readfilter_ready(ppg_shard *sh, int64_t *chunk_passed, void *result) {
    if (!sh) return PPG_ARG_ERROR;
    if (!sh->filter.written) return 0;
    sh->filter.outputs(sh->n, chunk_passed, result, sizeof(ppg_read_filter_result));
    return 1;
}

// ---- read trimming: the read filters entry points' counterparts ----
int ppg_read_trim_check(const void *trim) { return readtrim_ok(trim, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

int ppg_shard_trim_reads(ppg_shard *sh, const void *trim, uint32_t *dev_keep_mask, int64_t rec_cap, void *dev_trim,
                         int64_t trim_cap, int64_t *chunk_kept, void *result) {
    PpgReadTrim trm;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !readtrim_ok(trim, &trm) ||
        !readtrim_bufs_ok(trm, dev_keep_mask, rec_cap, dev_trim, trim_cap))
        return PPG_ARG_ERROR;
    if (!readtrim_linked()) return PPG_UNSUPPORTED;
    if ((dev_keep_mask && sh->total_records > rec_cap) || (dev_trim && sh->total_records > trim_cap)) return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    sh->trim.written = 0;   // the pinned outputs are rewritten: an earlier run's hook result is gone
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, sh->total_records)) return rc;
    if (int rc = shard_read_trim(sh, 0, sh->n, sh->recs.p, 0, sh->total_records, trm, dev_keep_mask, (uint32_t *)dev_trim, true))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    sh->trim.outputs(sh->n, chunk_kept, result, sizeof(ppg_read_trim_result));
    return PPG_OK;
}

int ppg_shard_set_readtrim(ppg_shard *sh, const void *trim, uint32_t *dev_keep_mask, int64_t rec_cap, void *dev_trim,
                           int64_t trim_cap) {
    if (!sh) return PPG_ARG_ERROR;
    PpgReadTrim trm = {};
    if (trim && (!readtrim_ok(trim, &trm) || !readtrim_bufs_ok(trm, dev_keep_mask, rec_cap, dev_trim, trim_cap)))
        return PPG_ARG_ERROR;
    TrimStage &t = sh->trim;
    t.on = trim ? 1 : 0;
    t.trm = trm;
    t.mask = trim ? dev_keep_mask : nullptr;
    t.rec_cap = trim ? rec_cap : 0;
    t.rows = trim ? (uint32_t *)dev_trim : nullptr;
    t.rows_cap = trim ? trim_cap : 0;
    t.written = 0;   // completed by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_readtrim_ready(ppg_shard *sh, int64_t *chunk_kept, void *result) {
    if (!sh) return PPG_ARG_ERROR;
    if (!sh->trim.written) return 0;
    sh->trim.outputs(sh->n, chunk_kept, result, sizeof(ppg_read_trim_result));
    return 1;
}

// ---- read profile: the read trimming entry points' counterparts ----
int ppg_read_profile_check(const void *profile) { return readprofile_ok(profile, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

int ppg_shard_profile_reads(ppg_shard *sh, const void *profile, const uint32_t *dev_mask, int64_t mask_cap,
                            const void *dev_windows, int64_t windows_cap, int64_t *chunk_profiled, void *result,
                            int64_t *table, int64_t table_cap) {
    PpgReadProfile prf;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !readprofile_ok(profile, &prf) ||
        !readprofile_bufs_ok(prf, dev_mask, mask_cap, dev_windows, windows_cap))
        return PPG_ARG_ERROR;
    if (!readprofile_linked()) return PPG_UNSUPPORTED;
    if ((dev_mask && sh->total_records > mask_cap) || (dev_windows && sh->total_records > windows_cap) ||
        (table && table_cap < prf.max_pos))
        return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    sh->profile.written = 0;   // the pinned outputs are rewritten: an earlier run's hook result is gone
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, sh->total_records)) return rc;
    if (int rc = shard_read_profile(sh, 0, sh->n, sh->recs.p, 0, sh->total_records, prf, dev_mask,
                                    (const uint32_t *)dev_windows, true))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    readprofile_outputs(sh->profile, sh->n, prf.max_pos, chunk_profiled, result, table);
    return PPG_OK;
}

int ppg_shard_set_readprofile(ppg_shard *sh, const void *profile, const uint32_t *dev_mask, int64_t mask_cap,
                              const void *dev_windows, int64_t windows_cap) {
    if (!sh) return PPG_ARG_ERROR;
    PpgReadProfile prf = {};
    if (profile && (!readprofile_ok(profile, &prf) || !readprofile_bufs_ok(prf, dev_mask, mask_cap, dev_windows, windows_cap)))
        return PPG_ARG_ERROR;
    ProfileStage &p = sh->profile;
    p.on = profile ? 1 : 0;
    p.prf = prf;
    p.mask = profile ? dev_mask : nullptr;
    p.mask_cap = profile ? mask_cap : 0;
    p.rows = profile ? (const uint32_t *)dev_windows : nullptr;
    p.rows_cap = profile ? windows_cap : 0;
    p.written = 0;   // completed by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_readprofile_ready(ppg_shard *sh, int64_t *chunk_profiled, void *result, int64_t *table, int64_t table_cap) {
    if (!sh) return PPG_ARG_ERROR;
    const ProfileStage &p = sh->profile;
    if (!p.written) return 0;
    if (table && table_cap < p.prf.max_pos) return PPG_BUF_ERROR;
    readprofile_outputs(p, sh->n, p.prf.max_pos, chunk_profiled, result, table);
    return 1;
}

// ---- read dedup: the read trimming entry points' counterparts ----
int ppg_read_dedup_check(const void *dedup) { return readdedup_ok(dedup, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

int ppg_shard_dedup_reads(ppg_shard *sh, const void *dedup, uint32_t *dev_unique_mask, int64_t mask_cap,
                          const void *dev_windows, int64_t windows_cap, int64_t *dev_first, int64_t first_cap,
                          void *dev_table, int64_t slots, int64_t *chunk_unique, void *result) {
    PpgReadDedup dd;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !readdedup_ok(dedup, &dd) ||
        !readdedup_bufs_ok(dd, dev_unique_mask, mask_cap, dev_windows, windows_cap, dev_first, first_cap,
                           (const uint64_t *)dev_table, slots))
        return PPG_ARG_ERROR;
    if (!readdedup_linked()) return PPG_UNSUPPORTED;
    if (readdedup_full(dev_unique_mask, mask_cap, dev_windows, windows_cap, dev_first, first_cap, slots, sh->total_records))
        return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    sh->dedup.written = 0;   // the pinned outputs are rewritten: an earlier run's hook result is gone
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, sh->total_records)) return rc;
    if (int rc = shard_read_dedup(sh, 0, sh->n, sh->recs.p, 0, sh->total_records, dd, dev_unique_mask,
                                  (const uint32_t *)dev_windows, dev_first, (uint64_t *)dev_table, slots, true, true))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    readdedup_outputs(sh->dedup, sh->n, chunk_unique, result);
    return PPG_OK;
}

int ppg_shard_set_readdedup(ppg_shard *sh, const void *dedup, uint32_t *dev_unique_mask, int64_t mask_cap,
                            const void *dev_windows, int64_t windows_cap, int64_t *dev_first, int64_t first_cap,
                            void *dev_table, int64_t slots) {
    if (!sh) return PPG_ARG_ERROR;
    PpgReadDedup dd = {};
    if (dedup && (!readdedup_ok(dedup, &dd) ||
                  !readdedup_bufs_ok(dd, dev_unique_mask, mask_cap, dev_windows, windows_cap, dev_first, first_cap,
                                     (const uint64_t *)dev_table, slots)))
        return PPG_ARG_ERROR;
    DedupStage &d = sh->dedup;
    d.on = dedup ? 1 : 0;
    d.dd = dd;
    d.mask = dedup ? dev_unique_mask : nullptr;
    d.mask_cap = dedup ? mask_cap : 0;
    d.rows = dedup ? (const uint32_t *)dev_windows : nullptr;
    d.rows_cap = dedup ? windows_cap : 0;
    d.first = dedup ? dev_first : nullptr;
    d.first_cap = dedup ? first_cap : 0;
    d.table = dedup ? (uint64_t *)dev_table : nullptr;
    d.slots = dedup ? slots : 0;
    d.written = 0;   // completed by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_readdedup_ready(ppg_shard *sh, int64_t *chunk_unique, void *result) {
    if (!sh) return PPG_ARG_ERROR;
    if (!sh->dedup.written) return 0;
    readdedup_outputs(sh->dedup, sh->n, chunk_unique, result);
    return 1;
}

// ---- pair overlap: one blocking call on the ctx stream ----
int ppg_pair_overlap_check(const void *overlap) { return pairoverlap_ok(overlap, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

int ppg_pairs_overlap(ppg_ctx *ctx, const void *overlap, const void *set1, const void *set2, const int64_t *dev_rec1,
                      const int64_t *dev_rec2, int64_t npairs, void *dev_rows, int64_t row_cap, uint32_t *dev_found_mask,
                      int64_t mask_cap, void *dev_windows1, int64_t win_cap1, void *dev_windows2, int64_t win_cap2,
                      void *result, int64_t *hist, int64_t hist_cap) {
    PairOverlapArgs a;
    if (int rc = pairoverlap_args(ctx, overlap, set1, set2, dev_rec1, dev_rec2, npairs, dev_rows, row_cap, dev_found_mask,
                                  mask_cap, dev_windows1, win_cap1, dev_windows2, win_cap2, hist, hist_cap, a))
        return rc;
    if (!pairoverlap_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    DevBuf<uint64_t> acc;
    HIPCHK(acc.alloc(kPoAcc + kPoHist));
    HIPCHK(hipMemsetAsync(acc.p, 0, 8 * (size_t)(kPoAcc + kPoHist), s));
    HIPCHK(ppg_launch_pair_overlap(s, a.s1, a.s2, dev_rec1, dev_rec2, npairs, &a.po, (int32_t *)dev_rows, dev_found_mask,
                                   (uint32_t *)dev_windows1, (uint32_t *)dev_windows2, acc.p, ctx->overlap_grid, cus));
    std::vector<int64_t> h((size_t)(kPoAcc + kPoHist));
    HIPCHK(hipMemcpyAsync(h.data(), acc.p, 8 * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (result) memcpy(result, h.data(), sizeof(ppg_pair_overlap_result));
    if (hist) memcpy(hist, h.data() + kPoAcc, 8 * (size_t)kPoHist);
    return PPG_OK;
}

// ---- pair merge: blocking calls on the ctx stream ----
int ppg_pair_merge_check(const void *merge) { return pairmerge_ok(merge, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

int ppg_pairs_merge_size(ppg_ctx *ctx, const void *set1, const void *set2, const int64_t *dev_rec1, const int64_t *dev_rec2,
                         int64_t npairs, const void *dev_rows, int64_t row_cap, int64_t *merged, int64_t *padded_bases) {
    PairMergeArgs a;
    if (int rc = pairmerge_inputs(ctx, set1, set2, dev_rec1, dev_rec2, npairs, dev_rows, row_cap, false, a)) return rc;
    if (!pairmerge_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    PairMergeScratch w;
    if (int rc = pairmerge_count(ctx->stream, a, dev_rec1, dev_rec2, npairs, dev_rows, w)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (merged) *merged = ((volatile int64_t *)w.host.p)[0];
    if (padded_bases) *padded_bases = ((volatile int64_t *)w.host.p)[1];
    return PPG_OK;
}

int ppg_pairs_merge(ppg_ctx *ctx, const void *merge, const void *set1, const void *set2, const int64_t *dev_rec1,
                    const int64_t *dev_rec2, int64_t npairs, const void *dev_rows, int64_t row_cap, int64_t *dev_seq_off,
                    uint32_t *dev_seq_len, int64_t rec_cap, uint32_t *dev_bases, uint32_t *dev_mask, uint8_t *dev_qual,
                    int64_t base_cap, int64_t *dev_pair_of, void *result) {
    PairMergeArgs a;
    if (!pairmerge_ok(merge, &a.pm)) return PPG_ARG_ERROR;
    // the output planes, as ppg_shard_pack_seq takes them
    // (a plane of capacity 0 holds nothing and may be NULL: an allocator gives no address for no bytes)
    if (rec_cap < 0 || base_cap < 0 || base_cap % 32 != 0 || !dev_seq_off || (!dev_seq_len && rec_cap > 0) ||
        ((!dev_bases || !dev_mask) && base_cap > 0) ||
        ((uintptr_t)dev_seq_off & 7) || ((uintptr_t)dev_seq_len & 3) || ((uintptr_t)dev_bases & 7) || ((uintptr_t)dev_mask & 3) ||
        ((uintptr_t)dev_qual & 15) || ((uintptr_t)dev_pair_of & 7))
        return PPG_ARG_ERROR;
    if (int rc = pairmerge_inputs(ctx, set1, set2, dev_rec1, dev_rec2, npairs, dev_rows, row_cap, true, a)) return rc;
    if (!pairmerge_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    PairMergeScratch w;
    if (int rc = pairmerge_count(s, a, dev_rec1, dev_rec2, npairs, dev_rows, w)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const int64_t merged = ((volatile int64_t *)w.host.p)[0], padded = ((volatile int64_t *)w.host.p)[1];
    if (merged > rec_cap || padded > base_cap) return PPG_BUF_ERROR;   // before the writers: nothing is written
    HIPCHK(w.acc.alloc(kPmAcc));
    HIPCHK(w.recs.alloc((size_t)merged));
    HIPCHK(hipMemsetAsync(w.acc.p, 0, 8 * (size_t)kPmAcc, s));
    if (npairs == 0) HIPCHK(hipMemsetAsync(dev_seq_off, 0, 8, s));   // (else ppg_pm_place writes seq_off[merged])
    HIPCHK(ppg_launch_pm_place(s, a.s1, a.s2, dev_rec1, dev_rec2, npairs, (const int32_t *)dev_rows, w.rbase(a.ntiles),
                               w.bbase(a.ntiles), dev_seq_off, dev_seq_len, dev_pair_of, w.recs.p, w.acc.p));
    HIPCHK(ppg_launch_pm_emit(s, a.s1, a.s2, w.recs.p, dev_seq_off, merged, padded, &a.pm, dev_bases, dev_mask, dev_qual,
                              w.acc.p, ctx->merge_grid, cus));
    int64_t h[kPmAcc];
    HIPCHK(hipMemcpyAsync(h, w.acc.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (result) memcpy(result, h, sizeof(ppg_pair_merge_result));
    return PPG_OK;
}

// ---- k-mer counts: blocking calls on the ctx stream ----
int ppg_kmer_count_check(const void *kmers) { return kmercount_ok(kmers, nullptr) ? PPG_OK : PPG_ARG_ERROR; }

// the empty table (or the count of its rows), the unit table with the call's totals, and the insert, queued on s
static int kmercount_insert(ppg_ctx *ctx, hipStream_t s, const KmerCountArgs &a, const uint32_t *mask, const void *windows,
                            void *table, int64_t slots, KmerCountScratch &w, int cus) {
    HIPCHK(ppg_launch_km_init(s, (uint64_t *)table, (uint64_t)slots, (a.kc.flags & PPG_KMER_ACCUMULATE) != 0, w.acc.p));
    if (w.units) HIPCHK(hipMemsetAsync(w.umap.p, 0xFF, 4 * (size_t)w.units, s));
    HIPCHK(ppg_launch_km_records(s, a.set, mask, (const uint32_t *)windows, &a.kc, w.units, w.umap.p, w.acc.p));
    HIPCHK(ppg_launch_km_insert(s, a.set, mask, (const uint32_t *)windows, w.umap.p, &a.kc, w.units, (uint64_t *)table,
                                (uint64_t)slots, w.acc.p, ctx->kmer_grid, cus));
    return PPG_OK;
}

int ppg_kmers_count(ppg_ctx *ctx, const void *kmers, const void *set, const uint32_t *dev_mask, int64_t mask_cap,
                    const void *dev_windows, int64_t windows_cap, void *dev_table, int64_t slots, void *result,
                    int64_t *spectrum, int64_t spectrum_cap) {
    KmerCountArgs a;
    if (int rc = kmercount_args(ctx, kmers, set, dev_mask, mask_cap, dev_windows, windows_cap, dev_table, slots, spectrum,
                                spectrum_cap, a))
        return rc;
    if (!kmercount_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    KmerCountScratch w;
    if (int rc = kmercount_units(s, a.set, &w.units)) return rc;
    HIPCHK(w.acc.alloc(kKmAccAll));
    HIPCHK(w.umap.alloc((size_t)w.units));
    HIPCHK(kmercount_clear(s, w.acc.p, true));
    if (int rc = kmercount_insert(ctx, s, a, dev_mask, dev_windows, dev_table, slots, w, cus)) return rc;
    HIPCHK(ppg_launch_km_stats(s, (const uint64_t *)dev_table, (uint64_t)slots, w.acc.p));
    std::vector<int64_t> h((size_t)kKmAccAll);
    HIPCHK(hipMemcpyAsync(h.data(), w.acc.p, 8 * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h[12] != 0 || h[7] > slots / 2) return PPG_BUF_ERROR;   // the table's contents are unspecified; nothing else is written
    h[6] = h[4] - h[5];
    if (h[9] == 0) h[10] = -1;   // an empty table
    if (result) memcpy(result, h.data(), sizeof(ppg_kmer_count_result));
    if (spectrum) memcpy(spectrum, h.data() + kKmSpecAt, 8 * (size_t)kKmSpectrum);
    return PPG_OK;
}

int ppg_kmers_select(ppg_ctx *ctx, const void *dev_table, int64_t slots, int64_t min_count, void *dev_out, int64_t out_cap,
                     int64_t *found) {
    if (!ctx || !kmer_table_ok(dev_table, slots) || min_count < 1 || out_cap < 0 || ((uintptr_t)dev_out & 15) ||
        (!dev_out && out_cap > 0))
        return PPG_ARG_ERROR;
    if (!kmercount_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf<uint64_t> cursor;
    HIPCHK(cursor.alloc(1));
    HIPCHK(hipMemsetAsync(cursor.p, 0, 8, s));
    HIPCHK(ppg_launch_km_select(s, (const uint64_t *)dev_table, (uint64_t)slots, min_count, (uint64_t *)dev_out,
                                dev_out ? out_cap : 0, cursor.p));
    int64_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, cursor.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (found) *found = n;
    return dev_out && n > out_cap ? PPG_BUF_ERROR : PPG_OK;   // (without dev_out the call only counts)
}

int ppg_kmers_lookup(ppg_ctx *ctx, const void *dev_table, int64_t slots, const void *dev_keys, int64_t nkeys,
                     int64_t *dev_counts) {
    if (!ctx || !kmer_table_ok(dev_table, slots) || nkeys < 0 || ((uintptr_t)dev_keys & 7) || ((uintptr_t)dev_counts & 7) ||
        ((!dev_keys || !dev_counts) && nkeys > 0))
        return PPG_ARG_ERROR;
    if (!kmercount_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ppg_launch_km_lookup(ctx->stream, (const uint64_t *)dev_table, (uint64_t)slots, (const uint64_t *)dev_keys, nkeys,
                                dev_counts));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PPG_OK;
}

// ---- record selection: the sequence queries entry points' counterparts ----
static bool select_bufs_ok(const int64_t *recno, const int64_t *sel_off, const uint32_t *desc, int64_t sel_cap,
                           const uint8_t *bytes, int64_t byte_cap) {
    // a descriptor is stored as one 16-B word, the text in 16-B words
    return recno && sel_off && desc && bytes && sel_cap >= 0 && byte_cap >= 0 && ((uintptr_t)recno & 7) == 0 &&
           ((uintptr_t)sel_off & 7) == 0 && ((uintptr_t)desc & 15) == 0 && ((uintptr_t)bytes & 15) == 0;
}

int ppg_shard_select_size(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int64_t *records, int64_t *bytes) {
    if (!sh || !sh->ran || !seqquery_mask_ok(dev_mask, mask_cap)) return PPG_ARG_ERROR;
    if (!select_linked()) return PPG_UNSUPPORTED;
    if (dev_mask && sh->total_records > mask_cap) return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    SelectStage &e = sh->select;
    if (int rc = shard_select_reserve(sh, sh->n)) return rc;
    const size_t h = e.ccnt.n / 2;
    // every batch's descriptors are resident, each with record bases relative to its own first record
    for (auto [b0, b1] : sh->batches) {
        const uint64_t r0 = (uint64_t)sh->h_base[(size_t)b0];
        HIPCHK(ppg_launch_sel_count(s, batch_view(sh, b0, b1, sh->recs.p + 4 * r0), dev_mask, r0, e.ccnt.p + b0,
                                    e.ccnt.p + h + b0));
    }
    HIPCHK(select_scan(sh, sh->batches.empty() ? 0 : sh->n));
    HIPCHK(hipStreamSynchronize(s));
    if (records) *records = ((volatile int64_t *)e.host.p)[0];
    if (bytes) *bytes = ((volatile int64_t *)e.host.p)[1];
    return PPG_OK;
}

int ppg_shard_select_records(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int64_t *dev_recno,
                             int64_t *dev_sel_off, uint32_t *dev_desc, int64_t sel_cap, uint8_t *dev_bytes,
                             int64_t byte_cap, int64_t *records, int64_t *bytes) {
    if (!sh || !sh->ran || sh->batches.size() != 1 || !seqquery_mask_ok(dev_mask, mask_cap) ||
        !select_bufs_ok(dev_recno, dev_sel_off, dev_desc, sel_cap, dev_bytes, byte_cap))
        return PPG_ARG_ERROR;
    if (!select_linked()) return PPG_UNSUPPORTED;
    if (dev_mask && sh->total_records > mask_cap) return PPG_BUF_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    int64_t S = 0, B = 0;
    if (int rc = shard_select_sizes(sh, 0, sh->n, sh->recs.p, dev_mask, 0, &S, &B)) return rc;
    if (records) *records = S;
    if (bytes) *bytes = B;
    if (S > sel_cap || B > byte_cap) return PPG_BUF_ERROR;   // before the movers: nothing is written
    if (int rc = shard_select_move(sh, 0, sh->n, sh->recs.p, dev_mask, 0, 0, 0, S, B, dev_recno, dev_sel_off, dev_desc,
                                   dev_bytes))
        return rc;
    HIPCHK(hipStreamSynchronize(shard_stream(sh)));
    return PPG_OK;
}

int ppg_shard_set_select(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int64_t *dev_recno,
                         int64_t *dev_sel_off, uint32_t *dev_desc, int64_t sel_cap, uint8_t *dev_bytes, int64_t byte_cap) {
    if (!sh) return PPG_ARG_ERROR;
    const bool off = !dev_mask && !mask_cap && !dev_recno && !dev_sel_off && !dev_desc && !sel_cap && !dev_bytes && !byte_cap;
    if (!off && (!seqquery_mask_ok(dev_mask, mask_cap) ||
                 !select_bufs_ok(dev_recno, dev_sel_off, dev_desc, sel_cap, dev_bytes, byte_cap)))
        return PPG_ARG_ERROR;
    SelectStage &e = sh->select;
    e.on = off ? 0 : 1;
    e.mask = dev_mask;
    e.mask_cap = mask_cap;
    e.recno = dev_recno;
    e.off = dev_sel_off;
    e.desc = dev_desc;
    e.bytes = dev_bytes;
    e.cap = sel_cap;
    e.byte_cap = byte_cap;
    e.written = 0;   // completed by the next run, not by an earlier one
    return PPG_OK;
}

int ppg_shard_select_ready(ppg_shard *sh, int64_t *records, int64_t *bytes) {
    if (!sh) return PPG_ARG_ERROR;
    if (!sh->select.written) return 0;
    if (records) *records = sh->select.records;
    if (bytes) *bytes = sh->select.nbytes;
    return 1;
}

// ---- measurement hooks of tools/*_probe.py (not part of the ABI: no declaration in ppgpu.h) ----
// Each works on a one-batch shard after its run and fills ms[] with device times on the shard's stream,
// the median of reps launches after one warm-up each (time_steps).  The buffers are the hook's own.  Where a
// whole stage runs first, it sizes the scratch buffers and leaves the layout in place; the stage's
// accumulators then keep adding over the launches (only the times are meaningful), and its pinned outputs
// no longer belong to a run.

// tools/seqselect_probe.py.  ms[0..4]: count, scan, place, copy, and ppg_pack_raw of the same batch (which
// moves every text byte once, as a selection of every record does); sizes[0..2]: the selected records,
// their bytes and the raw text's bytes.
int ppgx_seqselect_times(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int reps, float *ms, int64_t *sizes) {
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || !sizes || reps < 1 || !seqquery_mask_ok(dev_mask, mask_cap) ||
        (dev_mask && sh->total_records > mask_cap))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    int64_t S = 0, B = 0;
    if (int rc = shard_select_sizes(sh, 0, sh->n, sh->recs.p, dev_mask, 0, &S, &B)) return rc;
    const std::vector<int64_t> raw_off = raw_offsets(sh);
    DevBuf<int64_t> recno, off, draw;
    DevBuf<uint32_t> desc;
    DevBuf<uint8_t> dst, text;
    HIPCHK(recno.alloc((size_t)S));
    HIPCHK(off.alloc((size_t)S + 1));
    HIPCHK(desc.alloc(4 * (size_t)S));
    HIPCHK(dst.alloc((size_t)B + 16));
    HIPCHK(text.alloc((size_t)raw_off[(size_t)sh->n]));
    HIPCHK(draw.alloc(raw_off.size()));
    HIPCHK(hipMemcpyAsync(draw.p, raw_off.data(), 8 * raw_off.size(), hipMemcpyHostToDevice, s));
    // one whole move first: it sizes the scratch and leaves sel_off / the scratch in place for the copy
    if (int rc = shard_select_move(sh, 0, sh->n, sh->recs.p, dev_mask, 0, 0, 0, S, B, recno.p, off.p, desc.p, dst.p)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    sizes[0] = S;
    sizes[1] = B;
    sizes[2] = raw_off[(size_t)sh->n];
    SelectStage &e = sh->select;
    const size_t h = e.ccnt.n / 2;
    const PpgBatchView v = whole_view(sh);
    return time_steps(s, 5, reps, ms, [&](int step) {
        switch (step) {
            case 0: return ppg_launch_sel_count(s, v, dev_mask, 0, e.ccnt.p, e.ccnt.p + h);
            case 1: return select_scan(sh, sh->n);
            case 2:
                return ppg_launch_sel_place(s, v, dev_mask, 0, e.cbase.p, e.cbase.p + h, 0, 0, recno.p, off.p, desc.p, e.src.p,
                                            e.span.p);
            case 3: return ppg_launch_sel_copy(s, off.p, e.src.p, e.span.p, 0, S, 0, B, dst.p);
            default: return launch_pack_raw(sh, s, draw.p, text.p);
        }
    });
}

// tools/seqpack_probe.py.  ms[0..3]: layout totals + scan, seq_off / seq_len, the pack (qualities when
// quality != 0), and ppg_pack_raw of the same batch (the text cursor's kernel, which reads the same bytes
// and writes all of them); bytes[0..1]: the planes' and the raw text's sizes.
int ppgx_seqpack_times(ppg_shard *sh, int quality, int reps, float *ms, int64_t *bytes) {
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || !bytes || reps < 1) return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    int64_t total = 0;
    if (int rc = shard_seq_layout(sh, 0, sh->n, sh->recs.p, &total)) return rc;
    const int64_t nrec = sh->total_records;
    const std::vector<int64_t> raw_off = raw_offsets(sh);
    DevBuf<int64_t> off, draw;
    DevBuf<uint32_t> len, bases, mask;
    DevBuf<uint8_t> qual, text;
    HIPCHK(off.alloc((size_t)nrec + 1));
    HIPCHK(len.alloc((size_t)nrec));
    HIPCHK(bases.alloc((size_t)total / 16));
    HIPCHK(mask.alloc((size_t)total / 32));
    if (quality) HIPCHK(qual.alloc((size_t)total));
    HIPCHK(text.alloc((size_t)raw_off[(size_t)sh->n]));
    HIPCHK(draw.alloc(raw_off.size()));
    HIPCHK(hipMemcpyAsync(draw.p, raw_off.data(), 8 * raw_off.size(), hipMemcpyHostToDevice, s));
    bytes[0] = total / 4 + total / 8 + (quality ? total : 0) + 12 * nrec + 8;
    bytes[1] = raw_off[(size_t)sh->n];
    return time_steps(s, 4, reps, ms, [&](int step) {
        switch (step) {
            case 0: return launch_totals_scan(sh, s);
            case 1: return launch_offsets(sh, s, off.p, len.p);
            case 2:
                return ppg_launch_seq_pack(s, whole_view(sh), sh->lay.cbase.p, off.p, len.p, 0, (uint64_t)total, bases.p,
                                           mask.p, quality ? qual.p : nullptr);
            default: return launch_pack_raw(sh, s, draw.p, text.p);
        }
    });
}

// tools/seqquery_probe.py.  ms[0..3]: layout totals + scan, seq_off / seq_len, the query kernel (with the
// clearing of its hit bits when there is a pattern), and the per-chunk reduction + the totals' store.
int ppgx_seqquery_times(ppg_shard *sh, const uint8_t *pattern, int32_t m, int reps, float *ms) {
    PpgSeqPattern pat;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || reps < 1 || !seqquery_pattern(pattern, m, &pat))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    const int64_t tot = sh->total_records;
    QueryStage &q = sh->query;
    q.written = 0;
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, tot)) return rc;
    if (int rc = shard_seq_query(sh, 0, sh->n, sh->recs.p, 0, tot, pat, m, nullptr, true)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const StageLayout &lay = sh->lay;
    uint32_t *words = m > 0 ? q.bits.p : nullptr;
    const PpgBatchView v = whole_view(sh);
    return time_steps(s, 4, reps, ms, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0: return launch_totals_scan(sh, s);
            case 1: return launch_offsets(sh, s, lay.off.p, lay.len.p);
            case 2:
                if (words) e = hipMemsetAsync(words, 0, 4 * (size_t)((tot + 31) / 32), s);
                if (e != hipSuccess) return e;
                return ppg_launch_seq_query(s, v, lay.cbase.p, lay.off.p, lay.len.p, (uint64_t)lay.total, &pat, m, words, 0,
                                            q.acc.p);
            default:
                e = ppg_launch_seq_query_chunks(s, v, m, words, 0, q.acc.p, q.result() + 8);
                return e != hipSuccess ? e : ppg_launch_seq_query_totals(s, q.acc.p, q.result());
        }
    });
}

// tools/readfilter_probe.py.  ms[0..2]: the layout (totals + scan + seq_off / seq_len), the measure kernel
// with the zeroing of its scratch, and the decide kernel (with the clearing of its mask words) + the
// totals' store.  with_mask / with_metrics: the decide kernel writes scratch planes of that size.  hist:
// ppg_rf_measure's histogram variant (kRfHistRuns / kRfHistBytes).
int ppgx_readfilter_times(ppg_shard *sh, const void *filter, int with_mask, int with_metrics, int hist, int reps,
                          float *ms) {
    PpgReadFilter flt;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || reps < 1 || !readfilter_ok(filter, &flt) ||
        (flt.criteria & 0x100) || (hist != kRfHistRuns && hist != kRfHistBytes))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    const int64_t tot = sh->total_records;
    DevBuf<uint32_t> words;
    DevBuf<uint8_t> rows;
    if (with_mask) HIPCHK(words.alloc((size_t)tot / 32 + 1));
    if (with_metrics) HIPCHK(rows.alloc(24 * (size_t)tot + 8));
    FilterStage &f = sh->filter;
    f.written = 0;
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, tot)) return rc;
    const int hist_was = f.hist;
    f.hist = hist;
    const int rc = shard_read_filter(sh, 0, sh->n, sh->recs.p, 0, tot, flt, words.p, rows.p, true);
    f.hist = hist_was;
    if (rc != PPG_OK) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const StageLayout &lay = sh->lay;
    const PpgBatchView v = whole_view(sh);
    return time_steps(s, 3, reps, ms, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0:
                e = launch_totals_scan(sh, s);
                return e != hipSuccess ? e : launch_offsets(sh, s, lay.off.p, lay.len.p);
            case 1:
                if (tot) e = hipMemsetAsync(f.rsc.p, 0, 16 * (size_t)tot, s);
                if (e != hipSuccess) return e;
                return ppg_launch_rf_measure(s, v, lay.cbase.p, lay.off.p, lay.len.p, (uint64_t)lay.total,
                                             (uint32_t)(flt.qual_base + flt.low_q), f.rsc.p, f.acc.p, hist);
            default:
                if (words.p) e = hipMemsetAsync(words.p, 0, 4 * (size_t)((tot + 31) / 32), s);
                if (e == hipSuccess) e = ppg_launch_rf_decide(s, v, f.rsc.p, &flt, words.p, 0, rows.p, f.acc.p, f.result() + kRfAcc);
                return e != hipSuccess ? e : ppg_launch_rf_totals(s, f.acc.p, f.result());
        }
    });
}

// tools/readtrim_probe.py.  ms[0..3]: the layout, the measure kernel without the ADAPTER bit and with the
// trim's ops as they are (both with the initialisation of the scratch; equal ops when the trim has no
// adapter), and the decide kernel (with the clearing of its mask words, writing the rows) + the totals'
// store.  with_mask: the decide kernel writes a scratch mask.
int ppgx_readtrim_times(ppg_shard *sh, const void *trim, int with_mask, int reps, float *ms) {
    PpgReadTrim trm;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || reps < 1 || !readtrim_ok(trim, &trm) || (trm.ops & 0x100))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    const int64_t tot = sh->total_records;
    DevBuf<uint32_t> words, rows;
    if (with_mask) HIPCHK(words.alloc((size_t)tot / 32 + 1));
    HIPCHK(rows.alloc(2 * (size_t)tot + 2));
    TrimStage &t = sh->trim;
    t.written = 0;
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, tot)) return rc;
    if (int rc = shard_read_trim(sh, 0, sh->n, sh->recs.p, 0, tot, trm, words.p, rows.p, true)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const StageLayout &lay = sh->lay;
    const PpgBatchView v = whole_view(sh);
    PpgReadTrim plain = trm;
    plain.ops &= ~(int64_t)8;
    return time_steps(s, 4, reps, ms, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0:
                e = launch_totals_scan(sh, s);
                return e != hipSuccess ? e : launch_offsets(sh, s, lay.off.p, lay.len.p);
            case 1:
            case 2:
                e = readtrim_scratch_init(s, t.rsc.p, tot);
                if (e != hipSuccess) return e;
                return ppg_launch_rt_measure(s, v, lay.cbase.p, lay.off.p, lay.len.p, (uint64_t)lay.total,
                                             step == 1 ? &plain : &trm, t.rsc.p, (uint64_t)tot);
            default:
                if (words.p) e = hipMemsetAsync(words.p, 0, 4 * (size_t)((tot + 31) / 32), s);
                if (e == hipSuccess)
                    e = ppg_launch_rt_decide(s, v, t.rsc.p, (uint64_t)tot, &trm, words.p, 0, rows.p, t.acc.p, t.result() + kRtAcc);
                return e != hipSuccess ? e : ppg_launch_rt_totals(s, t.acc.p, t.result());
        }
    });
}

// tools/readprofile_probe.py.  ms[0..2]: the layout, the measure kernel with the zeroing of its scratch, and
// the finish kernel + the totals' store; mask / windows as ppg_shard_profile_reads takes them.
int ppgx_readprofile_times(ppg_shard *sh, const void *profile, const uint32_t *dev_mask, int64_t mask_cap,
                           const void *dev_windows, int64_t windows_cap, int reps, float *ms) {
    PpgReadProfile prf;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || reps < 1 || !readprofile_ok(profile, &prf) ||
        !readprofile_bufs_ok(prf, dev_mask, mask_cap, dev_windows, windows_cap) ||
        (dev_mask && sh->total_records > mask_cap) || (dev_windows && sh->total_records > windows_cap))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    const int64_t tot = sh->total_records;
    const uint32_t *rows = (const uint32_t *)dev_windows;
    ProfileStage &p = sh->profile;
    p.written = 0;
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, tot)) return rc;
    if (int rc = shard_read_profile(sh, 0, sh->n, sh->recs.p, 0, tot, prf, dev_mask, rows, true)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const StageLayout &lay = sh->lay;
    const PpgBatchView v = whole_view(sh);
    return time_steps(s, 3, reps, ms, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0:
                e = launch_totals_scan(sh, s);
                return e != hipSuccess ? e : launch_offsets(sh, s, lay.off.p, lay.len.p);
            case 1:
                if (tot) e = hipMemsetAsync(p.rsc.p, 0, 16 * (size_t)tot, s);
                if (e != hipSuccess) return e;
                return ppg_launch_rp_measure(s, v, lay.cbase.p, lay.off.p, lay.len.p, (uint64_t)lay.total, &prf, dev_mask, rows,
                                             0, p.rsc.p, p.acc.p, p.grid, p.cus);
            default:
                e = ppg_launch_rp_finish(s, v, p.rsc.p, &prf, dev_mask, rows, 0, p.acc.p, p.result() + p.values());
                return e != hipSuccess ? e : ppg_launch_rp_totals(s, p.acc.p, p.result(), (uint32_t)p.values());
        }
    });
}

// tools/readdedup_probe.py.  ms[0..4]: the layout, the measure kernel with the zeroing of its scratch, the
// insert kernel into a table made empty first, the decide kernel + the totals' store, and the levels; windows as
// ppg_shard_dedup_reads takes them, the table the caller's.  No mask: every record participates.
int ppgx_readdedup_times(ppg_shard *sh, const void *dedup, const void *dev_windows, int64_t windows_cap, void *dev_table,
                         int64_t slots, int reps, float *ms) {
    PpgReadDedup dd;
    if (!sh || !sh->ran || sh->batches.size() != 1 || !ms || reps < 1 || !readdedup_ok(dedup, &dd) ||
        (dd.flags & PPG_DEDUP_AND_MASK) ||
        !readdedup_bufs_ok(dd, nullptr, 0, dev_windows, windows_cap, nullptr, 0, (const uint64_t *)dev_table, slots) ||
        readdedup_full(nullptr, 0, dev_windows, windows_cap, nullptr, 0, slots, sh->total_records))
        return PPG_ARG_ERROR;
    HIPCHK(hipSetDevice(sh->ctx->device));
    hipStream_t s = shard_stream(sh);
    const int64_t tot = sh->total_records;
    const uint32_t *rows = (const uint32_t *)dev_windows;
    uint64_t *table = (uint64_t *)dev_table;
    DedupStage &d = sh->dedup;
    d.written = 0;
    if (int rc = shard_layout(sh, 0, sh->n, sh->recs.p, tot)) return rc;
    if (int rc = shard_read_dedup(sh, 0, sh->n, sh->recs.p, 0, tot, dd, nullptr, rows, nullptr, table, slots, true, true)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const StageLayout &lay = sh->lay;
    const PpgBatchView v = whole_view(sh);
    return time_steps(s, 5, reps, ms, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0:
                e = launch_totals_scan(sh, s);
                return e != hipSuccess ? e : launch_offsets(sh, s, lay.off.p, lay.len.p);
            case 1:
                if (tot) e = hipMemsetAsync(d.rsc.p, 0, 16 * (size_t)tot, s);
                if (e != hipSuccess) return e;
                return ppg_launch_dd_measure(s, v, lay.cbase.p, lay.off.p, lay.len.p, (uint64_t)lay.total, &dd, nullptr, rows, 0,
                                             d.rsc.p);
            case 2:
                e = ppg_launch_dd_init(s, table, (uint64_t)slots);
                return e != hipSuccess ? e : ppg_launch_dd_insert(s, v, &dd, nullptr, rows, 0, d.rsc.p, table, (uint64_t)slots, d.acc.p);
            case 3:
                e = ppg_launch_dd_decide(s, v, &dd, rows, 0, d.rsc.p, table, nullptr, nullptr, d.acc.p, d.result() + kDdAcc);
                return e != hipSuccess ? e : ppg_launch_dd_totals(s, d.acc.p, d.result());
            default: return ppg_launch_dd_levels(s, table, (uint64_t)slots, d.acc.p);
        }
    });
}

// ppg_rp_measure's grid on this shard from now on (0: the default, the blocks resident on the device).  The tests force the
// blocks' tile loop and uneven shares at small sizes with it.
int ppgx_readprofile_grid(ppg_shard *sh, int blocks) {
    if (!sh || blocks < 0) return PPG_ARG_ERROR;
    sh->profile.grid = blocks;
    return PPG_OK;
}

// tools/pairoverlap_probe.py.  ms[0]: the overlap kernel over pairs (i, i) of the two sets, with the zeroing of
// its accumulators, writing rows and found bits to scratch of the hook's own; no windows.  The stream is the
// ctx's.
int ppgx_pairoverlap_times(ppg_ctx *ctx, const void *overlap, const void *set1, const void *set2, int64_t npairs, int reps,
                           float *ms) {
    PairOverlapArgs a;
    if (!ms || reps < 1) return PPG_ARG_ERROR;
    if (int rc = pairoverlap_args(ctx, overlap, set1, set2, nullptr, nullptr, npairs, nullptr, 0, nullptr, 0, nullptr, 0,
                                  nullptr, 0, nullptr, 0, a))
        return rc;
    if (!pairoverlap_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    DevBuf<uint64_t> acc;
    DevBuf<int32_t> rows;
    DevBuf<uint32_t> found;
    HIPCHK(acc.alloc(kPoAcc + kPoHist));
    HIPCHK(rows.alloc(4 * (size_t)npairs));
    HIPCHK(found.alloc((size_t)npairs / 32 + 1));
    return time_steps(s, 1, reps, ms, [&](int) {
        const hipError_t e = hipMemsetAsync(acc.p, 0, 8 * (size_t)(kPoAcc + kPoHist), s);
        return e != hipSuccess ? e
                               : ppg_launch_pair_overlap(s, a.s1, a.s2, nullptr, nullptr, npairs, &a.po, rows.p, found.p, nullptr,
                                                         nullptr, acc.p, ctx->overlap_grid, cus);
    });
}

// ppg_po_overlap's grid on this ctx from now on (0: the default).  The tests force one block and uneven shares
// with it.
int ppgx_pairoverlap_grid(ppg_ctx *ctx, int blocks) {
    if (!ctx || blocks < 0) return PPG_ARG_ERROR;
    ctx->overlap_grid = blocks;
    return PPG_OK;
}

// tools/pairmerge_probe.py.  Pairs (i, i) of the two sets with the rows dev_rows, into planes of the hook's own.
// ms[0]: count and scan; ms[1]: place, with the zeroing of the accumulators; ms[2] / ms[3]: the emit kernel with /
// without the output's qual plane.  sizes[0..1]: the merged records and their padded bases.  The stream is the ctx's.
int ppgx_pairmerge_times(ppg_ctx *ctx, const void *merge, const void *set1, const void *set2, int64_t npairs,
                         const void *dev_rows, int reps, float *ms, int64_t *sizes) {
    PairMergeArgs a;
    if (!ms || !sizes || reps < 1 || !pairmerge_ok(merge, &a.pm)) return PPG_ARG_ERROR;
    if (int rc = pairmerge_inputs(ctx, set1, set2, nullptr, nullptr, npairs, dev_rows, npairs, true, a)) return rc;
    if (!pairmerge_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    PairMergeScratch w;
    if (int rc = pairmerge_count(s, a, nullptr, nullptr, npairs, dev_rows, w)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const int64_t merged = sizes[0] = ((volatile int64_t *)w.host.p)[0], padded = sizes[1] = ((volatile int64_t *)w.host.p)[1];
    DevBuf<int64_t> off;
    DevBuf<uint32_t> len, bases, mask;
    DevBuf<uint8_t> qual;
    HIPCHK(w.acc.alloc(kPmAcc));
    HIPCHK(w.recs.alloc((size_t)merged));
    HIPCHK(off.alloc((size_t)merged + 1));
    HIPCHK(len.alloc((size_t)merged));
    HIPCHK(bases.alloc((size_t)padded / 16));
    HIPCHK(mask.alloc((size_t)padded / 32));
    HIPCHK(qual.alloc((size_t)padded));
    HIPCHK(hipMemsetAsync(off.p, 0, 8, s));
    const int n = a.ntiles;
    return time_steps(s, 4, reps, ms, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0:
                e = ppg_launch_pm_count(s, a.s1, a.s2, nullptr, nullptr, npairs, (const int32_t *)dev_rows, w.trec(n), w.tbase(n));
                return e != hipSuccess ? e : ppg_launch_pm_scan(s, w.trec(n), w.tbase(n), w.rbase(n), w.bbase(n), (int64_t *)w.host.p, n);
            case 1:
                e = hipMemsetAsync(w.acc.p, 0, 8 * (size_t)kPmAcc, s);
                return e != hipSuccess ? e
                                       : ppg_launch_pm_place(s, a.s1, a.s2, nullptr, nullptr, npairs, (const int32_t *)dev_rows,
                                                             w.rbase(n), w.bbase(n), off.p, len.p, nullptr, w.recs.p, w.acc.p);
            default:
                return ppg_launch_pm_emit(s, a.s1, a.s2, w.recs.p, off.p, merged, padded, &a.pm, bases.p, mask.p,
                                          step == 2 ? qual.p : nullptr, w.acc.p, ctx->merge_grid, cus);
        }
    });
}

// ppg_pm_emit's grid on this ctx from now on (0: the default).  The tests force one block and uneven shares with it.
int ppgx_pairmerge_grid(ppg_ctx *ctx, int blocks) {
    if (!ctx || blocks < 0) return PPG_ARG_ERROR;
    ctx->merge_grid = blocks;
    return PPG_OK;
}

// tools/kmercount_probe.py.  The set without mask and windows into the caller's table (emptied every time; the
// ACCUMULATE bit is refused).  ms[0]: the table made empty; ms[1]: the unit table and the call's totals; ms[2]: the
// insert, with the emptying before it taken off (so it is the median of a difference); ms[3]: the spectrum's two
// passes; ms[4]: a select of every row with count >= 2 into scratch of the hook's own; ms[5]: a lookup of those rows'
// keys.  sizes[0..3]: valid k-mers, distinct keys, the selected rows, the overflow count of the last insert (not
// 0: the table is undersized, and the passes after the insert saw an unspecified table).  The stream is the ctx's.
int ppgx_kmercount_times(ppg_ctx *ctx, const void *kmers, const void *set, void *dev_table, int64_t slots, int reps,
                         float *ms, int64_t *sizes) {
    KmerCountArgs a;
    if (!ms || !sizes || reps < 1) return PPG_ARG_ERROR;
    if (int rc = kmercount_args(ctx, kmers, set, nullptr, 0, nullptr, 0, dev_table, slots, nullptr, 0, a)) return rc;
    if (a.kc.flags & PPG_KMER_ACCUMULATE) return PPG_ARG_ERROR;
    if (!kmercount_linked()) return PPG_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    KmerCountScratch w;
    if (int rc = kmercount_units(s, a.set, &w.units)) return rc;
    DevBuf<uint64_t> out, keys;
    DevBuf<int64_t> counts;
    const int64_t cap = slots / 2;
    HIPCHK(w.acc.alloc(kKmAccAll));
    HIPCHK(w.umap.alloc((size_t)w.units));
    HIPCHK(out.alloc(2 * (size_t)cap));
    HIPCHK(keys.alloc((size_t)cap));
    HIPCHK(counts.alloc((size_t)cap));
    uint64_t *table = (uint64_t *)dev_table;
    int64_t nsel = 0;
    float t[7];
    const int rc = time_steps(s, 7, reps, t, [&](int step) {
        hipError_t e = hipSuccess;
        switch (step) {
            case 0: return ppg_launch_km_init(s, table, (uint64_t)slots, 0, w.acc.p);
            case 1:
                e = kmercount_clear(s, w.acc.p, true);
                if (e == hipSuccess && w.units) e = hipMemsetAsync(w.umap.p, 0xFF, 4 * (size_t)w.units, s);
                return e != hipSuccess ? e : ppg_launch_km_records(s, a.set, nullptr, nullptr, &a.kc, w.units, w.umap.p, w.acc.p);
            case 2:
                e = kmercount_clear(s, w.acc.p, true);
                if (e == hipSuccess) e = ppg_launch_km_init(s, table, (uint64_t)slots, 0, w.acc.p);
                return e != hipSuccess ? e
                                       : ppg_launch_km_insert(s, a.set, nullptr, nullptr, w.umap.p, &a.kc, w.units, table,
                                                              (uint64_t)slots, w.acc.p, ctx->kmer_grid, cus);
            case 3: {
                // (the insert's totals stay: only the passes' own accumulators are cleared)
                e = hipMemsetAsync(w.acc.p + 7, 0, 8 * 5, s);
                if (e == hipSuccess) e = hipMemsetAsync(w.acc.p + kKmSpecAt, 0, 8 * (size_t)kKmSpectrum, s);
                if (e == hipSuccess) e = kmercount_clear(s, w.acc.p, false);
                return e != hipSuccess ? e : ppg_launch_km_stats(s, table, (uint64_t)slots, w.acc.p);
            }
            case 4:
                e = hipMemsetAsync(w.acc.p + kKmCursor, 0, 8, s);
                return e != hipSuccess ? e : ppg_launch_km_select(s, table, (uint64_t)slots, 2, out.p, cap, w.acc.p + kKmCursor);
            case 5: {
                // the selected rows' keys, once
                e = hipMemcpyAsync(&nsel, w.acc.p + kKmCursor, 8, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                nsel = std::min(nsel, cap);
                if (e == hipSuccess && nsel)
                    e = hipMemcpy2DAsync(keys.p, 8, out.p, 16, 8, (size_t)nsel, hipMemcpyDeviceToDevice, s);
                return e;
            }
            default: return ppg_launch_km_lookup(s, table, (uint64_t)slots, keys.p, nsel, counts.p);
        }
    });
    if (rc) return rc;
    ms[0] = t[0];
    ms[1] = t[1];
    ms[2] = t[2] - t[0];
    ms[3] = t[3];
    ms[4] = t[4];
    ms[5] = t[6];
    int64_t h[kKmAcc];
    HIPCHK(hipMemcpy(h, w.acc.p, sizeof h, hipMemcpyDeviceToHost));
    sizes[0] = h[5];
    sizes[1] = h[7];
    sizes[2] = nsel;
    sizes[3] = h[12];
    return PPG_OK;
}

// ppg_km_insert's grid on this ctx from now on (0: the default).  The tests force one block and uneven shares with it.
int ppgx_kmercount_grid(ppg_ctx *ctx, int blocks) {
    if (!ctx || blocks < 0) return PPG_ARG_ERROR;
    ctx->kmer_grid = blocks;
    return PPG_OK;
}

}  // extern "C"
