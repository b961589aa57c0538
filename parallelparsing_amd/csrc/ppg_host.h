// ppg_host.h — host-side types shared by the translation units of libppgpu.so
// (ppg_api.cpp: C ABI, index I/O, shards, ingest; ppg_stages.cpp: the record stages on a resident batch;
// ppg_index_gpu.cpp: GPU CreateIndex; ppg_cursor.cpp: record streaming; ppg_chunk.cpp + ppg_find.cpp:
// per-chunk Decompress; ppg_comm.cpp + ppg_pairs.hip: multi-GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <memory>
#include <new>
#include <utility>
#include <algorithm>

#include "../../include/ppgpu.h"
#include "ppg_device.h"

#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "ppgpu: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return PPG_DEVICE_ERROR;                                                       \
        }                                                                                  \
    } while (0)

namespace {
constexpr int kWin = PPG_WINSIZE;
// census capacity: one stored newline per this many output bytes (+64) per chunk; FASTQ lines
// average well above it (150 bp Generator records: ~97 B), chunks that overflow fall back to a scan
constexpr int kNlBytesPerEntry = 64;
constexpr int kChunk = PPG_CHUNK;
}

struct PpgPoint {                       // Common/Index.cs:51-82
    int64_t output = 0;                 // offset in the uncompressed stream
    int64_t input = 0;                  // offset of the first full byte in the .gz
    int32_t bits = 0;                   // unused bits (1-7) of byte input-1, or 0
    std::vector<uint8_t> offset;        // bytes since the last '@' (the partial record)
};

// allocator whose value-initialisation is default-initialisation: resize() leaves bytes
// uninitialised, so a window array can grow and be filled by one device-to-host copy
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U> &) {}
    template <class U>
    void construct(U *p) noexcept { ::new ((void *)p) U; }
    template <class U, class... A>
    void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};
using ByteVec = std::vector<uint8_t, NoInitAlloc<uint8_t>>;

struct ppg_index {
    int32_t chunk_max_bytes = 0;
    std::vector<PpgPoint> pts;
    // Point.Window (the preceding 32 KiB of output, oldest first) of point i at i * kWin: one
    // contiguous array, so a range of chunks ships its windows to the GPU in one copy
    ByteVec windows;
    const uint8_t *win(size_t i) const { return windows.data() + i * kWin; }
    // side points (ppg_index_build_gpu_side; not part of the .gzi): block starts inside chunks,
    // absolute bit / output and their 32 KiB windows, for ppg_shard_set_split
    std::vector<int64_t> side_bit, side_out;
    ByteVec side_win;

    // Index.AddPoint (Common/Index.cs:24-48)
    void add_point(int bits, int64_t input, int64_t output, uint32_t left, const uint8_t *circ,
                   const uint8_t *off, size_t off_len) {
        // oldest bytes (those after the circular write head) first
        windows.insert(windows.end(), circ + (kWin - left), circ + kWin);
        windows.insert(windows.end(), circ, circ + (kWin - left));
        add_point_fields(bits, input, output, off, off_len);
    }
    // the same without the window (the caller has appended it to `windows` already)
    void add_point_fields(int bits, int64_t input, int64_t output, const uint8_t *off, size_t off_len) {
        if (pts.empty()) {
            chunk_max_bytes = (int32_t)output;
        } else {
            int32_t sz = (int32_t)((uint32_t)(int32_t)output - (uint32_t)(int32_t)pts.back().output);
            chunk_max_bytes = std::max(chunk_max_bytes, sz);
        }
        PpgPoint p;
        p.output = output;
        p.input = input;
        p.bits = bits;
        p.offset.assign(off, off + off_len);
        pts.push_back(std::move(p));
    }
};

struct IngestState;   // host-ingest buffers kept across ppg_file_decompress_all calls
struct ChunkService;  // ppg_decompress_chunk's launch slots and request queue (ppg_chunk.cpp)
ChunkService *chunk_service_new();
void chunk_service_free(ChunkService *svc);

constexpr int kIxStats = 18;   // ppg_index_build_gpu_stats values (parallelparsing_amd.Core.GPU_INDEX_STATS)

struct ppg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t handoff = nullptr;   // ppg_ctx_wait_stream / ppg_stream_wait_ctx
    IngestState *ingest = nullptr;
    ChunkService *chunks = nullptr;
    int ring_bits = 11;   // inflate history ring: 2^10..2^15 bytes of LDS per wavefront (2 KiB: 32 waves/CU)
    int lit_bits = 8;     // litlen root table: 2^8 entries (codes <= 8 bits: 99.65% of FASTQ tokens)
    double ix_stats[kIxStats] = {0};   // timings / counts of the last GPU CreateIndex (ppg_index_build_gpu_stats)
    uint8_t *stage = nullptr;           // pinned device -> host staging (CreateIndex windows), kept across calls
    size_t stage_n = 0;
    int overlap_grid = 0;               // ppg_po_overlap's grid (0: the default; the tests force small ones)
    int merge_grid = 0;                 // ppg_pm_emit's grid, likewise
    int kmer_grid = 0;                  // ppg_km_insert's grid, likewise
};

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        if (p && n >= count) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; }
        n = count;
        return hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
    }
};

struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t n = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t count) {
        if (p && n >= count) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; }
        n = count;
        return hipHostMalloc((void **)&p, std::max<size_t>(count, 1), hipHostMallocDefault);
    }
};

// grow a buffer to `need` elements, by at least half again its size (no reallocation per call)
template <class B>
hipError_t grow_buf(B &b, size_t need) {
    if (b.p && b.n >= need) return hipSuccess;
    return b.alloc(std::max(need, b.n + b.n / 2));
}

// ---- record stages (ppg_stages.cpp): work on a batch of a shard while its output is resident ----
// The layout the unit kernels share (ppg_seqpack.hip): a batch's records on 32-base units.
struct StageLayout {
    DevBuf<uint64_t> ctot, cbase;   // per-chunk padded bases and their scan (n + 1 entries)
    PinnedBuf htot;                 // the scan's total, stored by the kernel
    DevBuf<int64_t> off;            // seq_off / seq_len of the batch's records from carry 0 (shard_layout)
    DevBuf<uint32_t> len;
    int64_t total = 0;              // padded bases of the batch laid out last
};

// What query, filter, trim and profile each carry: the run's accumulators on the device, and what the kernels
// store to pinned memory, the result struct (the profile's table after it) followed by one count per chunk of
// the shard.
struct StageOut {
    int on = 0;        // attached: every batch of a run goes through the stage
    int written = 0;   // the last successful run completed it (stages_run_end)
    DevBuf<uint64_t> acc;
    PinnedBuf host;
    int64_t *result() const { return (int64_t *)host.p; }
    // what the last completed stage left in pinned memory (n: the shard's chunks)
    void outputs(int32_t n, int64_t *chunk_counts, void *result, size_t result_bytes) const {
        if (!host.p) {   // a shard without chunks: no batch ran
            if (result) memset(result, 0, result_bytes);
            return;
        }
        if (result) memcpy(result, host.p, result_bytes);
        if (chunk_counts && n) memcpy(chunk_counts, host.p + result_bytes, 8 * (size_t)n);
    }
};

// ppg_shard_set_seqpack: every batch also packs its reads into these planes (ppg_seqpack.hip), records at
// their shard record number, bases continuing from the batches before (total)
struct PackStage {
    int64_t *off = nullptr;
    uint32_t *len = nullptr, *bases = nullptr, *mask = nullptr;
    uint8_t *qual = nullptr;
    int64_t rec_cap = 0, base_cap = 0;
    int64_t total = 0;   // padded bases of the run's batches so far
    int written = 0;     // the last successful run filled the planes
};

// ppg_shard_set_seqquery: every batch is also searched for pat and its bases counted (ppg_seqquery.hip);
// hit bits at the shard record number in mask.  acc: records, hits, (unused), count[5].
struct QueryStage : StageOut {
    PpgSeqPattern pat = {};
    int32_t m = 0;
    uint32_t *mask = nullptr;
    int64_t rec_cap = 0;
    DevBuf<uint32_t> bits;   // a batch's hit bits when the caller gives no mask
};

// ppg_shard_set_readfilter: every batch's records are also measured and filtered (ppg_readfilter.hip);
// pass bits and metrics rows at the shard record number.  acc: kRfAcc values.
struct FilterStage : StageOut {
    PpgReadFilter flt = {};
    uint32_t *mask = nullptr;
    int64_t rec_cap = 0;
    uint8_t *metrics = nullptr;
    int64_t metrics_cap = 0;
    int hist = kRfHistRuns;   // ppg_rf_measure's histogram variant (tools/readfilter_probe.py times both)
    DevBuf<uint64_t> rsc;     // scratch: other | low << 32 and qsum of one batch's records
};

// ppg_shard_set_readtrim: every batch's records are also trimmed (ppg_readtrim.hip); keep bits and
// (start, len) rows at the shard record number.  acc: kRtAcc values.
struct TrimStage : StageOut {
    PpgReadTrim trm = {};
    uint32_t *mask = nullptr;
    int64_t rec_cap = 0;
    uint32_t *rows = nullptr;
    int64_t rows_cap = 0;
    DevBuf<uint32_t> rsc;   // scratch: four planes (lead, win, adapt, trail) of one batch's records
};

// ppg_shard_set_readprofile: every batch's records are also profiled (ppg_readprofile.hip); the mask and the
// (start, len) rows are read at the shard record number.  acc and host: kRpFixed + kRpRow * max_pos values,
// the fixed result and then the table; host has the chunk counts after them.
struct ProfileStage : StageOut {
    PpgReadProfile prf = {};
    const uint32_t *mask = nullptr;
    int64_t mask_cap = 0;
    const uint32_t *rows = nullptr;
    int64_t rows_cap = 0;
    int grid = 0;             // ppg_rp_measure's blocks (ppgx_readprofile_grid); 0: the launcher's default
    int cus = 0;              // the device's CUs, asked for once
    int64_t out_pos = 0;      // max_pos of what host holds
    DevBuf<uint64_t> rsc;     // scratch: gc | qn << 32 and qsum of one batch's records
    int64_t values() const { return kRpFixed + (int64_t)kRpRow * out_pos; }
};

// ppg_shard_set_readdedup: every batch's records are also deduplicated (ppg_readdedup.hip) against the table,
// which persists across the batches of a run; the mask, the (start, len) rows and the first-occurrence row at
// the shard record number.  acc: kDdAcc values.
struct DedupStage : StageOut {
    PpgReadDedup dd = {};
    uint32_t *mask = nullptr;
    int64_t mask_cap = 0;
    const uint32_t *rows = nullptr;
    int64_t rows_cap = 0;
    int64_t *first = nullptr;
    int64_t first_cap = 0;
    uint64_t *table = nullptr;
    int64_t slots = 0;
    DevBuf<uint64_t> rsc;   // scratch: the sum of the unit hashes and the table row of one batch's records
};

// ppg_shard_set_select: every batch's selected records are also appended to these buffers
// (ppg_seqselect.hip), output records and bytes continuing from the batches before
struct SelectStage {
    int on = 0;
    int written = 0;   // the last successful run completed the selection
    const uint32_t *mask = nullptr;
    int64_t mask_cap = 0;
    int64_t *recno = nullptr, *off = nullptr;
    uint32_t *desc = nullptr;
    uint8_t *bytes = nullptr;
    int64_t cap = 0, byte_cap = 0;
    int64_t records = 0, nbytes = 0;   // selected by the run's batches so far
    DevBuf<uint64_t> ccnt, cbase;      // per chunk: selected records, then their bytes; the scans of both
    DevBuf<PpgSelSrc> src;             // scratch: where the bytes of a batch's selected records come from
    DevBuf<int64_t> span;              // scratch: ppg_sel_place's span_first
    PinnedBuf host;                    // a batch's totals (records, bytes), stored by the kernel
};

// DecompressAll state over chunks [first, first+n) of an index (ppg_api.cpp); the cursor
// (ppg_cursor.cpp), the per-chunk Decompress (ppg_chunk.cpp) and the pair check (ppg_pairs.hip)
// drive it through the functions below.
struct ppg_shard {
    ppg_ctx *ctx = nullptr;
    int32_t first = 0, n = 0;
    // compressed file range [Index[first].Input-1, Index[first+n].Input-1]
    DevBuf<uint8_t> comp_own;
    const uint8_t *comp = nullptr;
    int64_t comp_len = 0;
    uint64_t nwords = 0;
    DevBuf<PpgInflateJob> jobs;
    DevBuf<uint8_t> dicts;
    DevBuf<uint8_t> offs;
    DevBuf<PpgOffsetRef> oref;
    DevBuf<PpgInflateResult> res;
    DevBuf<PpgParseInfo> info;
    DevBuf<uint64_t> base;     // record base within the batch
    DevBuf<uint64_t> total;
    DevBuf<uint8_t> out;
    DevBuf<uint32_t> recs;     // descriptors of every record of the run, shard-global (all batches)
    DevBuf<uint32_t> nls;      // newline census of the inflate flush (PpgInflateJob::nl_off/nl_cap)
    int64_t out_cap = 0;
    std::vector<std::pair<int32_t, int32_t>> batches;   // chunk ranges [b0, b1) relative to first
    std::vector<PpgInflateJob> h_jobs;
    // results of the last run
    std::vector<PpgInflateResult> h_res;
    std::vector<PpgParseInfo> h_info;
    std::vector<int64_t> h_base;   // shard-global record base per chunk
    int64_t total_records = 0;
    float t_inflate = 0, t_parse = 0, t_total = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t stream = nullptr;   // null: the ctx stream (ppg_file_decompress_all gives each piece shard its own)
    uint64_t *h_tot = nullptr;      // pinned: a batch's record total, read back without a stream sync
    int ran = 0;
    int last_rc = PPG_OK;           // status of the last ppg_shard_run (the count gather forwards it)
    // ppg_shard_set_keys: every batch also writes its records' spot keys here (global record number)
    int64_t *keys_dev = nullptr;
    int64_t keys_cap = 0;
    int keys_written = 0;   // the last successful run filled keys_dev (stages_run_end)
    // a batch run again for the pair emission (ppg_pairs.hip: rerun_launch / rerun_collect): its hooks are
    // suspended, keys and record stages alike, so what the shard's own run left stays as it is
    int hooks_off = 0;
    // the record stages (ppg_stages.cpp), run by shard_batch_hooks on every batch while its output is resident
    StageLayout lay;
    PackStage pack;
    QueryStage query;
    FilterStage filter;
    TrimStage trim;
    DedupStage dedup;
    ProfileStage profile;
    SelectStage select;
    // split chunks (ppg_shard_set_split): the inflate launch runs sub-jobs, ppg_split_merge folds
    // them back into per-chunk results and census regions
    int32_t nsub = 0;                            // side points in use (0: one wave per chunk)
    int64_t base_byte = 0;                       // file byte of comp[0]
    std::vector<int64_t> h_pout;                 // Output of points first .. first + n
    std::vector<PpgInflateJob> h_sjobs;
    DevBuf<PpgInflateJob> sjobs;
    DevBuf<PpgInflateResult> sres;
    DevBuf<uint32_t> sidx;                      // chunk k = sub-jobs [sidx[k], sidx[k+1])
    std::vector<uint32_t> h_sidx;
    bool lpt = false;                           // the launch runs ljobs: sub-jobs longest first per batch,
    DevBuf<PpgInflateJob> ljobs;                // results in that order, sub-job j's at linv[j]
    DevBuf<uint32_t> linv;
    // one-batch launches whose pieces are materialised from pass-1 symbols (ppg_chunk.cpp): ljobs
    // [0, mat_first) are decoded, [mat_first, nsub + n) materialised with mat_info (launch order)
    uint32_t mat_n = 0, mat_first = 0;
    const uint16_t *mat_sym = nullptr;
    const uint8_t *mat_win = nullptr;
    const PpgMatInfo *mat_info = nullptr;
};

// one chunk of a shard: its Points, its window and where file byte from.Input-1 sits in comp
struct ChunkSpec {
    const PpgPoint *from, *to;
    const uint8_t *window;
    int64_t comp_byte;
    bool last;                          // `to` is the index's final Point (R-E5 end not checkable)
};
int shard_prepare_specs(ppg_shard *sh, const ChunkSpec *spec, int32_t n, const uint8_t *comp, int64_t comp_len,
                        int64_t out_capacity, hipStream_t s, const uint8_t *windows_contig);
int shard_prepare(ppg_shard *sh, const ppg_index *ix, int32_t first, int32_t n, const uint8_t *comp, int64_t comp_len,
                  int64_t out_capacity, hipStream_t s);
hipStream_t shard_stream(const ppg_shard *sh);
void shard_reset(ppg_shard *sh);
int batch_launch(ppg_shard *sh, int32_t b0, int32_t b1);
int batch_collect(ppg_shard *sh, int32_t b0, int32_t b1, float &total_ms);
int shard_finish(ppg_shard *sh, float total_ms);
int shard_split_from_index(ppg_shard *sh, const ppg_index *ix, int32_t first, int32_t n);
int shard_set_split_impl(ppg_shard *sh, int32_t nsub, const int64_t *bit, const int64_t *output,
                         const uint8_t *windows, bool lpt);
int shard_reserve(ppg_shard *sh, const ppg_index *ix, int32_t first,
                  const std::vector<std::pair<int32_t, int32_t>> &ranges, bool split);
bool pread_parallel(int fd, uint8_t *dst, int64_t off, int64_t len, int threads);
// ---- record stages (ppg_stages.cpp).  [b0, b1): chunks of one resident batch; recs: the batch's first
// descriptor; rec0: its first record's shard record number; tot: its records.  Everything is queued on the
// shard's stream; the calls said to block synchronise it. ----
PpgBatchView batch_view(const ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs);
// batch_collect's one call: the batch's hooks in the order keys, pack, query, filter, trim, dedup, profile, select
// (none of them while sh->hooks_off)
int shard_batch_hooks(ppg_shard *sh, int32_t b0, int32_t b1, int64_t tot);
// ppg_shard_run's two, and the fused pair emission's (ppg_pairs_emit_run: begin at the call, end after the last
// window): no hook's output counts as written during a run; a run that succeeded wrote them all
void stages_run_begin(ppg_shard *sh);
void stages_run_end(ppg_shard *sh, bool ok);
// packed reads.  layout: per-chunk padded bases, their scan and the batch's total (blocks); pack: seq_off /
// seq_len of the batch's records (pointers at its first record; bases from carry) and the planes, after a
// layout of the same chunks.
int shard_seq_reserve(ppg_shard *sh, int64_t nchunks);
int shard_seq_layout(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t *total);
int shard_seq_pack(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t carry, int64_t total,
                   int64_t *seq_off, uint32_t *seq_len, uint32_t *bases, uint32_t *mask, uint8_t *qual);
// The batch laid out for the unit kernels of query, filter and trim: shard_seq_layout (blocks), then seq_off /
// seq_len from carry 0 into sh->lay.  Made once per batch, before the first of those stages; they read it
// and never make it.
int shard_layout(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t tot);
// sequence query, after shard_layout of the same chunks; first: the run's accumulators start from 0.  The
// totals so far and the chunks' hits are in query.host once the stream has drained.
int shard_seq_query(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                    const PpgSeqPattern &pat, int32_t m, uint32_t *mask, bool first);
bool seqquery_pattern(const uint8_t *pattern, int32_t m, PpgSeqPattern *pat);
// read filter, with the arguments of shard_seq_query; mask and metrics may be null (metrics: row 0 of the
// plane).  The totals so far and the chunks' passes are in filter.host once the stream has drained.
int shard_read_filter(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                      const PpgReadFilter &flt, uint32_t *mask, uint8_t *metrics, bool first);
// read trim, with the arguments of shard_read_filter; mask and rows may be null (rows: row 0 of the plane,
// two words per record).  The totals so far and the chunks' keeps are in trim.host once the stream has
// drained.  readtrim_ok: the rules of ppg_read_trim_check, the struct as the kernels' argument.
int shard_read_trim(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                    const PpgReadTrim &trm, uint32_t *mask, uint32_t *rows, bool first);
bool readtrim_ok(const void *trim, PpgReadTrim *out);
// read profile, after shard_layout of the same chunks; mask and rows (both at the shard's record 0) may be
// null.  The totals so far, the table and the chunks' profiled records are in profile.host once the stream
// has drained.
int shard_read_profile(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                       const PpgReadProfile &prf, const uint32_t *mask, const uint32_t *rows, bool first);
// read dedup, after shard_layout of the same chunks; mask, rows and first_out (all at the shard's record 0) may
// be null; table: slots rows, made empty when `first`; last: the run's last batch, after which the levels
// are made.  The caller has checked 2 * (rec0 + tot) <= slots.  The totals so far and the chunks' uniques are
// in dedup.host once the stream has drained.
int shard_read_dedup(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, int64_t rec0, int64_t tot,
                     const PpgReadDedup &dd, uint32_t *mask, const uint32_t *rows, int64_t *first_out, uint64_t *table,
                     int64_t slots, bool first, bool last);
// record selection (record j of the batch has bit bit0 + j of mask, a null mask selects all).  sizes: the
// selected records and their bytes (blocks).  move: after sizes of the same chunks, queues the selection into
// the buffers from output record rec_lo and byte byte_lo on; recno counts from bit0.
int shard_select_reserve(ppg_shard *sh, int64_t nchunks);
int shard_select_sizes(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, const uint32_t *mask, int64_t bit0,
                       int64_t *records, int64_t *bytes);
int shard_select_move(ppg_shard *sh, int32_t b0, int32_t b1, const uint32_t *recs, const uint32_t *mask, int64_t bit0,
                      int64_t rec_lo, int64_t byte_lo, int64_t records, int64_t bytes, int64_t *recno, int64_t *sel_off,
                      uint32_t *desc, uint8_t *dst);

// collectives of a ppg_comm beyond the count gather (ppg_comm.cpp), used by ppg_pairs.hip
int comm_size(const ppg_comm *c, int32_t *rank, int32_t *nranks);
int comm_device(const ppg_comm *c);   // -1: host transport
int comm_all_gather_i64(ppg_comm *c, const int64_t *send, int64_t *recv, size_t n, bool &sent_ok);
int comm_alltoallv_i64(ppg_comm *c, hipStream_t s, const int64_t *send, int64_t *recv, const int64_t *m,
                       bool on_device);
// the RCCL point-to-point entry points of one grouped exchange (ppg_comm.cpp; host_check passes fakes)
struct CommP2P {
    ncclResult_t (*send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*group_start)();
    ncclResult_t (*group_end)();
    const char *(*err)(ncclResult_t);
};
int comm_grouped_p2p(const CommP2P &f, void *comm, hipStream_t stream, const int64_t *send, int64_t *recv,
                     const int64_t *m, int32_t R, int32_t me, const int64_t *sd, const int64_t *rd);
