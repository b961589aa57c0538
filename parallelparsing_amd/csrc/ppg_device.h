// ppg_device.h — host/device shared records of libppgpu (plain C layout, no HIP types).
#pragma once
#include <stdint.h>

// One inflate job per checkpoint chunk k (Point k -> Point k+1 of Common/Index.cs:51-82).
struct PpgInflateJob {
    uint64_t bit_start;   // 8*from.Input - from.Bits, relative to the device copy of the file range
    uint64_t bit_limit;   // 8*to.Input (relative): the slice LazyFileReader hands zlib ends there
    uint64_t out_off;     // from.Output - base output of the batch (byte offset into the out buffer)
    uint64_t out_len;     // to.Output - from.Output (Core.cs:140)
    uint64_t dict_off;    // byte offset of from.Window (32 KiB) in the dictionary buffer
    uint64_t expect_end;  // 8*to.Input - to.Bits (R-E5), or ~0 when not checkable (last chunk)
    // CreateIndex pass 1 only (ppg_inflate_kernel<.., IX = true>): decode whole blocks until one
    // ends at or past stop_bit (or the final block ends); block ends go to blk[blk_off, +blk_cap)
    uint64_t stop_bit;
    uint32_t blk_off;
    uint32_t blk_cap;
    // DecompressAll: the newline census fused into the output flush (ppg_inflate_kernel, nls != null).
    // Body newline m (chunk position p) is stored as raw_shift + p at nls[nl_off + m] while m < nl_cap.
    uint64_t nl_off;
    uint32_t nl_cap;
    uint32_t raw_shift;   // |offset_k|: raw index of the body's first byte
    uint32_t prev_byte;   // raw byte before the body: offset_k's last byte, or '\n' when offset_k is empty
    uint32_t pad;         // (raw[0] == '\n' is then an empty line, as in Parsing.Parse's view)
};

struct PpgInflateResult {
    uint64_t produced;    // bytes written (Core.cs:191: len - AvailOut)
    uint64_t end_bit;     // bit position after the chunk's trailing end-of-block code
    int32_t status;       // 0 or a ZResult error code (Interop/Conventions.cs:9-20)
    int32_t flags;        // PPG_FLAG_*
    uint32_t nblocks;     // CreateIndex pass 1: block ends recorded
    uint32_t last;        // CreateIndex pass 1: the final block (BFINAL) was decoded
    uint32_t newlines;    // census: '\n' bytes in the produced body
    uint32_t pflags;      // census: PPG_PF_* below
};

#define PPG_PF_SERIAL 1     // an empty line (incl. at the offset junction) or a NUL byte in the body
#define PPG_PF_OVERFLOW 2   // more body newlines than nl_cap: descriptors come from ppg_parse_emit
#define PPG_PF_NUL 4        // a NUL byte in the body (ppg_parse_chain declines the chunk)

// CreateIndex: one deflate block end (Core.cs:98 -- where inflate(Z_BLOCK) reports data_type & 128)
struct PpgBlockEnd {
    uint64_t end_bit;     // absolute bit position after the block (the next block's header)
    uint64_t out_end;     // output bytes of the piece up to the block end
};

// CreateIndex: '@' census of one block's output (Core.cs:79-96), positions relative to the block
struct PpgAtStats {
    uint32_t count;       // '@' bytes
    int32_t first;        // first '@' (-1: none)
    int32_t last;         // last '@' (-1: none)
    uint32_t max_gap;     // largest distance between consecutive '@' inside the block
};

// offset_k bytes (Common/Index.cs:75) live concatenated in one device buffer
// ppg_materialize_kernel: where a piece's pass-1 symbols and its exact starting history are
struct PpgMatInfo {
    uint64_t sym_off;     // first symbol (positions) in the pass-1 output buffer
    uint64_t win_off;     // its 32 KiB starting history in the window buffer (bytes)
    uint64_t end_bit;     // the piece's last block end (its result's end_bit)
    uint32_t nblocks;
    uint32_t last;        // the piece ends with the final block
    uint32_t prev;        // the census's previous byte, or > 255: the history's last byte
    uint32_t pad;
};

struct PpgOffsetRef {
    uint64_t start;
    uint32_t len;
    uint32_t nl;          // '\n' bytes in offset_k | PPG_OFF_SERIAL
};

#define PPG_OFF_SERIAL 0x80000000u   // offset_k alone has an empty line or a NUL (R-P3)
#define PPG_OFF_NUL 0x40000000u      // offset_k has a NUL
#define PPG_OFF_COUNT 0x3FFFFFFFu    // the '\n' count

struct PpgParseInfo {
    uint64_t records;     // FastqRecords emitted by Parsing.Parse for this chunk
    uint32_t newlines;    // '\n' bytes in raw
    uint16_t serial;      // 1: parsed by the exact serial state machine
    uint16_t emit;        // 1: census overflowed; descriptors by the ppg_parse_emit scan
};

// CreateIndex: a 32 KiB history ending at output position `end` of a piece (ppg_gather_kernel)
struct PpgGather {
    uint64_t out_off;     // position p >= 0 of the piece is out[out_off + (p & mask)]
    uint64_t dict_off;    // position p < 0 is dicts[dict_off + 32768 + p]
    uint64_t end;
    uint64_t mask;        // 0xFFFF for pass-1 rings, ~0 for plain output
    uint64_t ref_off;     // with a reference buffer: compare against ref[ref_off, +32768)
};

struct PpgSpan {          // byte range [lo, hi) of an output buffer
    uint64_t lo, hi;
};

// ppg_seq_query's pattern, a kernel argument: byte i is bits [8 (i & 7), + 8) of w[i >> 3] (m <= 64 bytes)
struct PpgSeqPattern {
    uint64_t w[8];
};

// a ppg_read_filter (include/ppgpu.h "read filters") as ppg_rf_decide's kernel argument
struct PpgReadFilter {
    int64_t criteria, min_len, max_len, max_other, qual_base, min_mean_milli, low_q, max_low_milli;
};
// the read filter's accumulators: the int64 fields of a ppg_read_filter_result in order (records, passed,
// failed[4], bases, other, qual_bytes, qual_count[256])
constexpr int kRfAcc = 265;
// ppg_rf_measure's Quality histogram: one LDS add per run of equal bytes of a lane, or one per byte
constexpr int kRfHistRuns = 0, kRfHistBytes = 1;

// a ppg_read_trim (include/ppgpu.h "read trimming") as the trim kernels' argument; the adapter's bytes as
// little-endian dwords
struct PpgReadTrim {
    int64_t ops, head, tail, qual_base, lead_q, trail_q, win_size, win_q, min_overlap, max_err_milli, min_len,
        adapter_len;
    uint32_t adapter[16];
};
// the read trim's accumulators: the int64 fields of a ppg_read_trim_result in order (records, kept, trimmed,
// cut[5], bases, bases_window, bases_kept)
constexpr int kRtAcc = 11;

// a ppg_read_profile (include/ppgpu.h "read profile") as the profile kernels' argument
struct PpgReadProfile {
    int64_t flags, qual_base, max_pos, reserved;
};
// the read profile's accumulators: the int64 fields of a ppg_read_profile_result in order (records, profiled,
// longer, bases, bases_profiled, qual_bytes, no_quality, reserved, gc_hist[101], meanq_hist[64]), then the
// table: max_pos rows of kRpRow values (base[5], qual_n, qual_sum, len_here, qhist[64])
constexpr int kRpFixed = 173, kRpRow = 72, kRpMaxPos = 1024;
// ppg_rp_measure's LDS, in 32-bit counters: 7 planes (base[5], qual_n, qual_sum) of kRpStride(max_pos)
// positions and the quality rows of the first kRpTile(max_pos), both multiples of 32.  80 KiB at most: two
// blocks stay resident per CU (160 KiB).  All of 256 positions fit (72 KiB); of 1,024, 192 quality rows.
constexpr int kRpLdsWords = 20480;
constexpr int kRpStride(int max_pos) { return (max_pos + 31) & ~31; }
constexpr int kRpTile(int max_pos) {
    return ((kRpLdsWords - 7 * kRpStride(max_pos)) / 64 & ~31) < kRpStride(max_pos)
               ? ((kRpLdsWords - 7 * kRpStride(max_pos)) / 64 & ~31)
               : kRpStride(max_pos);
}
static_assert(kRpTile(256) == 256 && kRpTile(kRpMaxPos) == 192 && kRpTile(1) == 32, "ppg_rp_measure's quality rows");

// a ppg_read_dedup (include/ppgpu.h "read dedup") as the dedup kernels' argument
struct PpgReadDedup {
    int64_t flags, max_bases, reserved[2];
};
// the read dedup's accumulators: the int64 fields of a ppg_read_dedup_result in order (records, participating,
// unique, bases, bases_unique, overflow, max_count, max_first, level_distinct[16], level_reads[16])
constexpr int kDdAcc = 40;

// a ppg_packed_view and a ppg_pair_overlap (include/ppgpu.h "pair overlap") as the overlap kernel's arguments
struct PpgPackedView {
    const int64_t *seq_off;
    const uint32_t *seq_len;
    const uint32_t *bases;
    const uint32_t *mask;
    const uint8_t *qual;
    int64_t records;
};
struct PpgPairOverlap {
    int64_t flags, min_overlap, max_diff, max_err_milli, reserved[4];
};
// the pair overlap's accumulators: the int64 fields of a ppg_pair_overlap_result in order (pairs, unmapped,
// too_long, analysed, found, negative, adapter, overlap_bases, mismatches, clipped[2], reserved[5]), then the
// insert-size histogram of kPoHist bins.  kPoMaxLen: the longest read a pair is analysed with.
constexpr int kPoAcc = 16, kPoHist = 2048, kPoMaxLen = 1024;

// a ppg_pair_merge (include/ppgpu.h "pair merge") as the merge's arguments
struct PpgPairMerge {
    int64_t flags, qual_hi, qual_lo, reserved[5];
};
// the pair merge's accumulators: the int64 fields of a ppg_pair_merge_result in order (pairs, unmapped, too_long,
// unmerged, stale, merged, merged_bases, padded_bases: ppg_pm_place; overlap_bases, disagree, from2, ties,
// n_filled, n_both, corrected[2]: ppg_pm_emit)
constexpr int kPmAcc = 16, kPmPlaceAcc = 8;
constexpr int kPmTile = 256;   // pairs per block of ppg_pm_count and ppg_pm_place
// ppg_pm_place -> ppg_pm_emit, per merged record: the first 32-base units of both reads in their sets, their
// lengths and the row's d, all checked (the merged length is L2 + d)
struct alignas(16) PpgMergeRec {
    int64_t u1, u2;
    uint32_t L1, L2;
    int32_t d;
    uint32_t pad;
};

// a ppg_kmer_count (include/ppgpu.h "k-mer counts") as the k-mer kernels' argument
struct PpgKmerCount {
    int64_t flags, k, reserved[6];
};
// the k-mer counter's accumulators: the int64 fields of a ppg_kmer_count_result in order (records, participating,
// short_reads, bases, positions, kmers, invalid, distinct, singletons, max_count, max_key, total_count, overflow,
// reserved[3]), then the claimed-rows counter and the select's cursor, and from kKmSpecAt on the spectrum's kKmSpectrum bins
constexpr int kKmAcc = 16, kKmClaimed = 16, kKmCursor = 17, kKmSpecAt = 32, kKmSpectrum = 1024, kKmAccAll = kKmSpecAt + kKmSpectrum;

// ppg_sel_copy: the destination bytes one workgroup writes (256 threads x 4 words of 16 B); ppg_sel_place
// records, per multiple of it inside a batch's destination range, the selected record that holds that byte
constexpr uint32_t kSelSpan = 16384;

// ppg_sel_place -> ppg_sel_copy, per selected record with first destination byte o (absolute in the
// destination buffer) and text raw_k[a, ..): destination byte p comes from address fast + p when
// p >= cend (the body part) and from slow + p below (the offset carry part)
struct PpgSelSrc {
    int64_t fast;   // (address of body_k) - |offset_k| + a - o
    int64_t slow;   // (address of offset_k) + a - o
    int64_t cend;   // o + |offset_k| - a
};

#define PPG_FLAG_NO_EOB 1     // the symbol after the last output byte is not end-of-block
#define PPG_FLAG_OVERRUN 2    // decoding consumed bits past the chunk's compressed slice
#define PPG_FLAG_BLK_FULL 16  // CreateIndex pass 1: more block ends than blk_cap

// CRC-32 of the GPU CreateIndex's exact output (ppg_crc_kernel): one lane per kCrcSub bytes, one
// wave (64 lanes) per kCrcSeg bytes
constexpr uint32_t kCrcSub = 16384;
constexpr uint32_t kCrcSeg = 64 * kCrcSub;

// One resident batch as the record-stage launchers take it (ppg_launch.h, from ppg_seqpack.hip on; built
// by batch_view, ppg_stages.cpp): the batch's output and offset carries, the per-chunk tables at its
// first chunk, its first record's descriptor and the number of its chunks.
struct PpgBatchView {
    const uint8_t *out;
    const PpgInflateJob *jobs;
    const PpgInflateResult *res;
    const uint8_t *offs;
    const PpgOffsetRef *oref;
    const PpgParseInfo *info;
    const uint64_t *base;
    const uint32_t *recs;
    int n;
};
