// ppg_launch.h — the host launchers of every kernel, declared once, grouped by the defining .hip file:
// that file and every translation unit that calls one include this, so a signature has one place to change.
#pragma once
#include <hip/hip_runtime.h>
#include "ppg_device.h"

// ---- ppg_inflate.hip ----
size_t ppg_inflate_lds_bytes(int ring_bits, int lit_bits);
hipError_t ppg_launch_inflate(hipStream_t s, int ring_bits, int lit_bits, const uint32_t *comp, uint64_t nwords,
                              const PpgInflateJob *jobs, const uint8_t *dicts, uint8_t *out, PpgInflateResult *res,
                              int njobs, uint32_t *nls);
hipError_t ppg_launch_inflate_ix(hipStream_t s, const uint32_t *comp, uint64_t nwords, const PpgInflateJob *jobs,
                                 const uint8_t *dicts, uint8_t *out, PpgInflateResult *res, PpgBlockEnd *blk,
                                 int njobs);
hipError_t ppg_launch_inflate_ixf(hipStream_t s, const uint32_t *comp, uint64_t nwords, const PpgInflateJob *jobs,
                                  const uint8_t *dicts, uint8_t *out, PpgInflateResult *res, PpgBlockEnd *blk,
                                  int njobs);
hipError_t ppg_launch_materialize(hipStream_t s, const uint16_t *sym, const uint8_t *wins, const PpgMatInfo *mi,
                                  const PpgInflateJob *jobs, uint8_t *out, PpgInflateResult *res, int njobs,
                                  uint32_t *nls);

// ---- ppg_parse.hip ----
hipError_t ppg_launch_parse_count(hipStream_t s, const uint8_t *out, const PpgInflateJob *jobs,
                                  const PpgInflateResult *ires, const uint8_t *offs, const PpgOffsetRef *oref,
                                  PpgParseInfo *info, uint64_t *base, uint64_t *total, int n, const uint32_t *nls);
hipError_t ppg_launch_total_to_host(hipStream_t s, const uint64_t *total, uint64_t *host);
hipError_t ppg_launch_parse_emit(hipStream_t s, const uint8_t *out, const PpgInflateJob *jobs,
                                 const PpgInflateResult *ires, const uint8_t *offs, const PpgOffsetRef *oref,
                                 PpgParseInfo *info, const uint64_t *base, const uint32_t *nls, uint32_t *recs,
                                 uint64_t cap, int n);
hipError_t ppg_launch_record_keys(hipStream_t s, const uint8_t *out, const PpgInflateJob *jobs,
                                  const PpgInflateResult *ires, const uint8_t *offs, const PpgOffsetRef *oref,
                                  const PpgParseInfo *info, const uint64_t *base, const uint32_t *recs, int64_t *keys,
                                  int n);
hipError_t ppg_launch_pack_raw(hipStream_t s, const uint8_t *out, const PpgInflateJob *jobs, const PpgInflateResult *ires,
                               const uint8_t *offs, const PpgOffsetRef *oref, const int64_t *raw_off, uint8_t *dst,
                               int n, int blocks);
hipError_t ppg_launch_copy16(hipStream_t s, const void *src, void *dst, uint64_t n16, int blocks);
hipError_t ppg_launch_split_merge(hipStream_t s, const PpgInflateJob *sjobs, const PpgInflateResult *sres,
                                  const uint32_t *inv, const uint32_t *sidx, const uint32_t *snls,
                                  const PpgInflateJob *jobs, PpgInflateResult *res, uint32_t *nls, int n);

// ---- ppg_index.hip ----
hipError_t ppg_launch_block_find(hipStream_t s, const uint32_t *comp, uint64_t nwords, const uint64_t *lo,
                                 const uint64_t *hi, uint64_t *cand, int n, int sub);
hipError_t ppg_launch_gather(hipStream_t s, const uint8_t *out, const uint8_t *dicts, const PpgGather *g, uint8_t *dst,
                             const uint8_t *ref, uint32_t *diff, int n);
hipError_t ppg_launch_at_stats(hipStream_t s, const uint8_t *out, const PpgSpan *spans, PpgAtStats *st, int n);
hipError_t ppg_launch_pack_blocks(hipStream_t s, const PpgBlockEnd *blk, const PpgInflateJob *jobs,
                                  const PpgInflateResult *res, const uint64_t *pre, PpgBlockEnd *dense, int n);
int ppg_resolve_groups(int np);
hipError_t ppg_launch_resolve(hipStream_t s, const uint8_t *ta, const uint8_t *tb, const uint32_t *slots, int np,
                              uint8_t *W, uint16_t *M);
hipError_t ppg_launch_resolve_chains(hipStream_t s, const uint8_t *ta, const uint32_t *slots, const uint4 *chains,
                                     int nchains, const uint8_t *windows, uint8_t *W);
hipError_t ppg_launch_pick_windows(hipStream_t s, const uint8_t *src, const uint32_t *idx, int n, uint8_t *dst);
hipError_t ppg_launch_crc(hipStream_t s, const uint8_t *out, uint64_t n, uint64_t pad, const uint32_t *tabs,
                          uint32_t *seg_raw, uint64_t nseg);

// ---- ppg_seqpack.hip ----
// From here on the launchers take the batch as a PpgBatchView (ppg_device.h; batch_view, ppg_stages.cpp)
// and unpack it into their kernel's arguments.
// Weak: libppgpu.so always links that object, but the host-only sanitizer build (tests/native) links
// the host translation units with the kernel objects of inflate / parse / index alone; there the
// packed-read entry points fail with PPG_UNSUPPORTED (seq_linked, ppg_stages.cpp) instead of the link
// failing.  There is no other implementation to fall back to.  (ppg_seqpack.hip includes this header
// as well, which makes its definitions weak symbols: they are the only ones, so they link the same.)
#define PPG_WEAK __attribute__((weak))
PPG_WEAK hipError_t ppg_launch_seq_totals(hipStream_t s, const PpgBatchView &v, uint64_t *ctot);
PPG_WEAK hipError_t ppg_launch_seq_scan(hipStream_t s, const uint64_t *ctot, uint64_t *cbase, uint64_t *host_total,
                                        int n);
PPG_WEAK hipError_t ppg_launch_seq_offsets(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, int64_t carry,
                                           int64_t *seq_off, uint32_t *seq_len);
PPG_WEAK hipError_t ppg_launch_seq_pack(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase,
                                        const int64_t *seq_off, const uint32_t *seq_len, int64_t carry, uint64_t total,
                                        uint32_t *bases, uint32_t *mask, uint8_t *qual);

// ---- ppg_seqquery.hip ----
// Weak for the same reason (seqquery_linked, ppg_stages.cpp).
PPG_WEAK hipError_t ppg_launch_seq_query(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase,
                                         const int64_t *seq_off, const uint32_t *seq_len, uint64_t total,
                                         const PpgSeqPattern *pat, int m, uint32_t *hit_words, uint64_t rec0,
                                         uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_seq_query_chunks(hipStream_t s, const PpgBatchView &v, int m, uint32_t *hit_words,
                                                uint64_t rec0, uint64_t *acc, int64_t *host_chunk_hits);
PPG_WEAK hipError_t ppg_launch_seq_query_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result);

// ---- ppg_readfilter.hip ----
// Weak for the same reason (readfilter_linked, ppg_stages.cpp).
PPG_WEAK hipError_t ppg_launch_rf_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase,
                                          const int64_t *seq_off, const uint32_t *seq_len, uint64_t total, uint32_t thr,
                                          uint64_t *rsc, uint64_t *acc, int hist);
PPG_WEAK hipError_t ppg_launch_rf_decide(hipStream_t s, const PpgBatchView &v, const uint64_t *rsc,
                                         const PpgReadFilter *f, uint32_t *words, uint64_t rec0, uint8_t *metrics,
                                         uint64_t *acc, int64_t *host_chunk_passed);
PPG_WEAK hipError_t ppg_launch_rf_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result);

// ---- ppg_readtrim.hip ----
// Weak for the same reason (readtrim_linked, ppg_stages.cpp).
PPG_WEAK hipError_t ppg_launch_rt_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase,
                                          const int64_t *seq_off, const uint32_t *seq_len, uint64_t total,
                                          const PpgReadTrim *tr, uint32_t *rsc, uint64_t tot);
PPG_WEAK hipError_t ppg_launch_rt_decide(hipStream_t s, const PpgBatchView &v, const uint32_t *rsc, uint64_t tot,
                                         const PpgReadTrim *tr, uint32_t *words, uint64_t rec0, uint32_t *trim,
                                         uint64_t *acc, int64_t *host_chunk_kept);
PPG_WEAK hipError_t ppg_launch_rt_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result);
PPG_WEAK hipError_t ppg_launch_rt_gather(hipStream_t s, const uint32_t *trim, const int64_t *recno, int64_t rec0,
                                         uint64_t n, uint32_t *dst);

// ---- ppg_readprofile.hip ----
// Weak for the same reason (readprofile_linked, ppg_stages.cpp).
PPG_WEAK hipError_t ppg_launch_rp_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase,
                                          const int64_t *seq_off, const uint32_t *seq_len, uint64_t total,
                                          const PpgReadProfile *prf, const uint32_t *words, const uint32_t *rows,
                                          uint64_t rec0, uint64_t *rsc, uint64_t *acc, int blocks, int cus);
PPG_WEAK hipError_t ppg_launch_rp_finish(hipStream_t s, const PpgBatchView &v, const uint64_t *rsc,
                                         const PpgReadProfile *prf, const uint32_t *words, const uint32_t *rows,
                                         uint64_t rec0, uint64_t *acc, int64_t *host_chunk_profiled);
PPG_WEAK hipError_t ppg_launch_rp_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result, uint32_t n);

// ---- ppg_readdedup.hip ----
// Weak for the same reason (readdedup_linked, ppg_stages.cpp).  table: slots rows of {key, first, count}.
PPG_WEAK hipError_t ppg_launch_dd_init(hipStream_t s, uint64_t *table, uint64_t slots);
PPG_WEAK hipError_t ppg_launch_dd_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase,
                                          const int64_t *seq_off, const uint32_t *seq_len, uint64_t total,
                                          const PpgReadDedup *dd, const uint32_t *words, const uint32_t *rows,
                                          uint64_t rec0, uint64_t *rsc);
PPG_WEAK hipError_t ppg_launch_dd_insert(hipStream_t s, const PpgBatchView &v, const PpgReadDedup *dd,
                                         const uint32_t *words, const uint32_t *rows, uint64_t rec0, uint64_t *rsc,
                                         uint64_t *table, uint64_t slots, uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_dd_decide(hipStream_t s, const PpgBatchView &v, const PpgReadDedup *dd,
                                         const uint32_t *rows, uint64_t rec0, const uint64_t *rsc, const uint64_t *table,
                                         uint32_t *words_out, int64_t *first_out, uint64_t *acc,
                                         int64_t *host_chunk_unique);
PPG_WEAK hipError_t ppg_launch_dd_levels(hipStream_t s, const uint64_t *table, uint64_t slots, uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_dd_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result);

// ---- ppg_pairoverlap.hip ----
// Weak for the same reason (pairoverlap_linked, ppg_stages.cpp).  Two packed read sets, not a batch: rows of
// four int32, found in the hit-mask format, win1 / win2 rows of two uint32, acc kPoAcc + kPoHist values.
PPG_WEAK hipError_t ppg_launch_pair_overlap(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2,
                                            const int64_t *rec1, const int64_t *rec2, int64_t npairs,
                                            const PpgPairOverlap *po, int32_t *rows, uint32_t *found, uint32_t *win1,
                                            uint32_t *win2, uint64_t *acc, int blocks, int cus);

// ---- ppg_pairmerge.hip ----
// Weak for the same reason (pairmerge_linked, ppg_stages.cpp).  Two packed read sets with qualities and the
// overlap's rows; trec / tbase: a value per tile of kPmTile pairs, rbase / bbase: one more; host_totals:
// two values in pinned memory; recs: a row per merged record; acc: kPmAcc values.
PPG_WEAK hipError_t ppg_launch_pm_count(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2,
                                        const int64_t *rec1, const int64_t *rec2, int64_t npairs, const int32_t *rows,
                                        uint64_t *trec, uint64_t *tbase);
PPG_WEAK hipError_t ppg_launch_pm_scan(hipStream_t s, const uint64_t *trec, const uint64_t *tbase, uint64_t *rbase,
                                       uint64_t *bbase, int64_t *host_totals, int ntiles);
PPG_WEAK hipError_t ppg_launch_pm_place(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2,
                                        const int64_t *rec1, const int64_t *rec2, int64_t npairs, const int32_t *rows,
                                        const uint64_t *rbase, const uint64_t *bbase, int64_t *seq_off,
                                        uint32_t *seq_len, int64_t *pair_of, PpgMergeRec *recs, uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_pm_emit(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2,
                                       const PpgMergeRec *recs, const int64_t *seq_off, int64_t merged,
                                       int64_t padded_bases, const PpgPairMerge *pm, uint32_t *bases, uint32_t *mask,
                                       uint8_t *qual, uint64_t *acc, int blocks, int cus);

// ---- ppg_kmercount.hip ----
// Weak for the same reason (kmercount_linked, ppg_stages.cpp).  One packed read set; words / rows: the record
// mask and the windows or null; umap: a record number per 32-base unit; table: slots rows of {key, count};
// acc: kKmAccAll values.
PPG_WEAK hipError_t ppg_launch_km_init(hipStream_t s, uint64_t *table, uint64_t slots, int accumulate, uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_km_records(hipStream_t s, const PpgPackedView &set, const uint32_t *words,
                                          const uint32_t *rows, const PpgKmerCount *kc, uint64_t units, uint32_t *umap,
                                          uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_km_insert(hipStream_t s, const PpgPackedView &set, const uint32_t *words,
                                         const uint32_t *rows, const uint32_t *umap, const PpgKmerCount *kc,
                                         uint64_t units, uint64_t *table, uint64_t slots, uint64_t *acc, int blocks,
                                         int cus);
PPG_WEAK hipError_t ppg_launch_km_stats(hipStream_t s, const uint64_t *table, uint64_t slots, uint64_t *acc);
PPG_WEAK hipError_t ppg_launch_km_select(hipStream_t s, const uint64_t *table, uint64_t slots, int64_t min_count,
                                         uint64_t *out, int64_t out_cap, uint64_t *cursor);
PPG_WEAK hipError_t ppg_launch_km_lookup(hipStream_t s, const uint64_t *table, uint64_t slots, const uint64_t *keys,
                                         int64_t nkeys, int64_t *counts);

// ---- ppg_seqselect.hip ----
// Weak for the same reason (select_linked, ppg_stages.cpp).
PPG_WEAK hipError_t ppg_launch_sel_count(hipStream_t s, const PpgBatchView &v, const uint32_t *mask, uint64_t bit0,
                                         uint64_t *crec, uint64_t *cbyte);
PPG_WEAK hipError_t ppg_launch_sel_scan(hipStream_t s, const uint64_t *crec, const uint64_t *cbyte, uint64_t *rbase,
                                        uint64_t *bbase, int64_t *host_totals, int n);
PPG_WEAK hipError_t ppg_launch_sel_place(hipStream_t s, const PpgBatchView &v, const uint32_t *mask, uint64_t bit0,
                                         const uint64_t *rbase, const uint64_t *bbase, int64_t rec_lo, int64_t byte_lo,
                                         int64_t *recno, int64_t *sel_off, uint32_t *desc, PpgSelSrc *src,
                                         int64_t *span_first);
PPG_WEAK hipError_t ppg_launch_sel_copy(hipStream_t s, const int64_t *sel_off, const PpgSelSrc *src,
                                        const int64_t *span_first, int64_t rec_lo, int64_t rec_hi, int64_t d0, int64_t d1,
                                        uint8_t *dst);
