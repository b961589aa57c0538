// ppg_readdedup.hip — read dedup over the resident batches of a run (include/ppgpu.h "read dedup"): a 64-bit
// fingerprint of every participating record's key bytes, a hash table in device memory that persists across
// the batches of a run, from it "first occurrence or not" as one mask bit per record, and after the last
// batch the duplication levels of a QC report.  The reference has no such step: its consumer would pull every
// record to the host and hash there; here only a 40-value result leaves the device.
//
//   layout   as the other unit kernels: made once per batch by shard_layout, read here.
//   init     the run's first batch makes every row of the table empty (ppg_dd_init): key 0, first all ones,
//            count 0.
//   measure  one lane per 32-base unit (ppg_dd_measure), chunk and record by unit_lookup (ppg_seqload.h).
//            Unit i of the key bytes D_j = S_j[s_j, s_j + Ld_j) starts at any alignment (load_raw32 takes
//            one), so it is read by the lane of the record's unit i: Ld_j <= L_j, so there are enough lanes.
//            A lane whose unit lies at or past Ld_j, or whose record has a clear mask bit under AND_MASK,
//            loads nothing.  The per-unit hashes h_i are summed mod 2^64 within the wave segmented by record,
//            as ppg_rf_measure sums its counts, and each segment's last lane adds the sum to the record's
//            zeroed scratch word: one 64-bit atomic per record and wave.
//   insert   a block per chunk, a thread per record (ppg_dd_insert): finishes F_j from the scratch word and
//            Ld_j, then probes from the home slot.  Every access to the table is a device-scope atomic:
//            atomicCAS on the key (0 -> F), and on the row that holds F an atomicMin on `first` and an
//            atomicAdd on `count`.  No lane waits for another lane's write: a lane that loses the CAS to
//            another key steps on, one that loses to its own key uses the row.  The probe is bounded by
//            `slots`; a lane that exhausts it bumps `overflow` and gives up.  The record's slot goes to its
//            second scratch word.  The lanes of a wave with one fingerprint are aggregated first, in registers:
//            the lowest of them inserts for all with the group's size, so a hot key costs three atomics per
//            wave, not per record.
//   decide   a separate launch (ppg_dd_decide): the kernel boundary orders every row's atomicMin before the
//            reads.  A block per chunk, a thread per record, as ppg_rf_decide: unique_j = first == j, the
//            first row, the mask words from the wave's ballot by atomicOr / atomicAnd, the chunk's uniques
//            to pinned memory, the totals into the run's accumulators.  Final when the batch's hooks return:
//            earlier batches hold the lower record numbers.
//   levels   after the run's last batch (ppg_dd_levels): a lane per row of the table, the duplication levels
//            accumulated per block in LDS and flushed with one atomic per non-empty bin; the greatest count
//            by atomicMax.  A second pass (ppg_dd_maxfirst) takes the least `first` among the rows of that
//            count: ties go to the lowest first.
//   totals   ppg_dd_totals stores the accumulators, laid out as a ppg_read_dedup_result, to pinned host
//            memory by kernel stores (as ppg_rf_totals: no DMA engine).
//
// Bytes moved per 150 bp record (five units), derived from the formats, not measured: 150 B of Sequence, 12 B
// of seq_off / seq_len per unit lookup (cached across a record's units), 16 B of descriptor in each of the
// measure, insert and decide passes, 16 B of scratch zeroed, added to, read, written and read (~56 B), one
// 24-B table row touched by three atomics and read once more (a 64-B sector each time at random), 8 B of
// dev_first and 1 bit of mask when given: ~290 B of streamed traffic and ~4 scattered sectors.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_mix.h"
#include "ppg_seqload.h"

namespace {

// (dd_mix: ppg_mix.h)
constexpr unsigned long long kDdGold = 0x9E3779B97F4A7C15ull, kDdLen = 0x632BE59BD9B4E019ull;
// the record's second scratch word when it has no row: it does not participate / its probe found none
constexpr unsigned long long kDdNone = ~0ull, kDdOver = ~0ull - 1;

// the window (s, w) of a record of Sequence length L (row r of `rows` clamped, or (0, L)) and from it the
// key bytes' start and length
__device__ __forceinline__ void dd_key(const uint32_t *__restrict__ rows, uint64_t r, uint32_t L, int64_t max_bases,
                                       uint32_t &s, uint32_t &Ld) {
    s = 0;
    uint32_t w = L;
    if (rows) {
        const uint2 row = *(const uint2 *)(rows + 2 * r);
        s = min(row.x, L);
        w = min(row.y, L - s);
    }
    Ld = max_bases > 0 ? (uint32_t)min((int64_t)w, max_bases) : w;
}

__device__ __forceinline__ bool dd_bit(const uint32_t *__restrict__ words, uint64_t r) {
    return !words || ((words[r >> 5] >> (uint32_t)(r & 31u)) & 1u);
}

// FastQC's bins of a row's count: 1 .. 9, 10-49, 50-99, 100-499, 500-999, 1000-4999, 5000-9999, >= 10000
__device__ __forceinline__ uint32_t dd_level(unsigned long long c) {
    return c < 10 ? (uint32_t)c - 1u : c < 50 ? 9u : c < 100 ? 10u : c < 500 ? 11u : c < 1000 ? 12u : c < 5000 ? 13u
         : c < 10000 ? 14u : 15u;
}

}  // namespace

// Every row of the table empty.
extern "C" __global__ __launch_bounds__(256) void ppg_dd_init(unsigned long long *table, uint64_t slots) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < slots; r += (uint64_t)gridDim.x * 256) {
        table[3 * r] = 0;
        table[3 * r + 1] = ~0ull;
        table[3 * r + 2] = 0;
    }
}

// One thread per 32-base unit of the batch.  seq_off / seq_len / recs / rsc point at the batch's first record;
// words (the mask under AND_MASK, else null) and rows (null: no windows) at the shard's: record j of the batch
// is bit / row rec0 + j.  Record j gets rsc[2 j] += the h_i of its key bytes' units.
extern "C" __global__ __launch_bounds__(256) void ppg_dd_measure(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const uint8_t *__restrict__ offs,
    const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase, const int64_t *__restrict__ seq_off,
    const uint32_t *__restrict__ seq_len, uint64_t units, const uint32_t *__restrict__ words,
    const uint32_t *__restrict__ rows, uint64_t rec0, int64_t max_bases, unsigned long long *rsc, int nchunks) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long jkey = ~0ull;   // the unit's record; lanes past the last unit share one key and add nothing
    unsigned long long h = 0;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u < units) {
        const uint64_t rel = 32 * u;
        int k;
        uint64_t j;
        unit_lookup(cbase, base, info, seq_off, nchunks, rel, 0, k, j);
        jkey = j;
        const uint64_t i0 = (uint64_t)((int64_t)rel - seq_off[j]);   // 32 i: the unit's first index within the key bytes
        uint32_t s, Ld;
        dd_key(rows, rec0 + j, seq_len[j], max_bases, s, Ld);
        if (i0 < Ld && dd_bit(words, rec0 + j)) {
            const uint32_t cnt = min(Ld - (uint32_t)i0, 32u);
            const uint32_t n1 = recs[4 * j];
            uint32_t x[8];
            // s + i0 + cnt <= s + Ld <= L_j: inside S_j
            load_raw32(offs + oref[k].start, oref[k].len, out + jobs[k].out_off, (uint64_t)n1 + 1 + s + i0, cnt, x);
            unsigned long long a = dd_mix(kDdGold * (i0 / 32 + 1));
#pragma unroll
            for (int t = 0; t < 4; t++) a = dd_mix(a ^ ((unsigned long long)x[2 * t] | (unsigned long long)x[2 * t + 1] << 32));
            h = a;
        }
    }
    // sums over the lanes of one record: after the step `o` a lane holds its segment's lanes [lane - 2o + 1, lane]
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long jo = __shfl_up(jkey, o, 64), a = __shfl_up(h, o, 64);
        if (lane >= (uint32_t)o && jo == jkey) h += a;
    }
    const unsigned long long jn = __shfl_down(jkey, 1, 64);
    if (jkey != ~0ull && (lane == 63u || jn != jkey) && h) atomicAdd(rsc + 2 * jkey, h);   // the segment's last lane
}

// A block per chunk k of the batch, a thread per record.  A participating record (the chunk decoded and, with
// `words`, its bit set) finishes its fingerprint from rsc[2 j] and its key length.  The lanes of a wave that
// hold one fingerprint then go to the table as one: the lowest of them, which holds the lowest record number,
// claims or joins the row of that key with the group's size, and hands the row to the others.  (Without this
// a hot key costs three same-address atomics per record: 100 ms for 2.88 M records against 0.45 ms when all
// are distinct, tools/readdedup_probe.py.)  Table rows are {key, first, count}, touched by atomics alone.
// rsc[2 j + 1] = the row, kDdNone for a record that does not participate, kDdOver when the probe found no row
// (acc[5] counts those).
extern "C" __global__ __launch_bounds__(256) void ppg_dd_insert(
    const PpgInflateResult *__restrict__ ires, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint32_t *__restrict__ words, const uint32_t *__restrict__ rows,
    uint64_t rec0, int64_t max_bases, unsigned long long *rsc, unsigned long long *table, uint64_t slots, uint32_t shift,
    unsigned long long *acc, int nchunks) {
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (k >= nchunks) return;
    const bool ok = ires[k].status == 0;   // (a failed chunk's descriptors are not defined: none of its records participates)
    const uint64_t nrec = info[k].records, rb = base[k];
    for (uint64_t j0 = 0; j0 < nrec; j0 += 256) {   // every lane of the block takes every round: the wave stays whole
        const uint64_t j = j0 + t, r = rec0 + rb + j;
        const bool valid = j < nrec;
        const bool part = valid && ok && dd_bit(words, r);
        unsigned long long F = 0;
        if (part) {
            const uint4 d = *(const uint4 *)(recs + 4 * (rb + j));
            const uint32_t L = d.y > d.x ? d.y - d.x - 1 : 0u;
            uint32_t s, Ld;
            dd_key(rows, r, L, max_bases, s, Ld);
            F = dd_mix(rsc[2 * (rb + j)] ^ dd_mix((unsigned long long)Ld + kDdLen));
            if (F == 0) F = 1;
        }
        // the wave's groups of equal fingerprints: as many steps as it holds distinct ones, registers alone
        uint32_t leader = lane, group = 1;
        for (unsigned long long rem = __ballot(part); rem;) {
            const int l = __ffsll((long long)rem) - 1;           // the lowest lane not yet in a group
            const unsigned long long Fl = __shfl(F, l, 64);
            const bool same = part && F == Fl;
            const unsigned long long members = __ballot(same);   // (lane l itself among them)
            if (same) {
                leader = (uint32_t)l;
                group = (uint32_t)__popcll(members);
            }
            rem &= ~members;
        }
        unsigned long long where = kDdNone;
        if (part && leader == lane) {
            uint64_t slot = (F * kDdGold) >> shift;
            where = kDdOver;
            for (uint64_t n = 0; n < slots; n++) {
                unsigned long long *row = table + 3 * slot;
                const unsigned long long old = atomicCAS(row, 0ull, F);
                if (old == 0 || old == F) {
                    atomicMin(row + 1, (unsigned long long)r);
                    atomicAdd(row + 2, (unsigned long long)group);
                    where = slot;
                    break;
                }
                slot = (slot + 1) & (slots - 1);
            }
            if (where == kDdOver) atomicAdd(acc + 5, (unsigned long long)group);
        }
        where = __shfl(where, (int)leader, 64);   // (a lane outside every group is its own leader)
        if (valid) rsc[2 * (rb + j) + 1] = where;
    }
}

// A block per chunk k of the batch, a thread per record, after ppg_dd_insert of the same batch has completed.
// unique = the record participates and its row's first is its own number.  Writes first_out[rec0 + j]
// (first_out != null: the first occurrence's number, -1 for a record without a row), the record's bit
// rec0 + j of words_out (and_mask: the bit is cleared when the record is not unique and left alone otherwise,
// else the words were zeroed and the bit is set when it is), host_chunk_unique[k] (pinned) and the run's
// accumulators acc[0] records, acc[1] participating, acc[2] unique, acc[3] bases, acc[4] bases_unique.
extern "C" __global__ __launch_bounds__(256) void ppg_dd_decide(
    const PpgInflateResult *__restrict__ ires, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint32_t *__restrict__ rows, uint64_t rec0, int64_t max_bases,
    const unsigned long long *__restrict__ rsc, const unsigned long long *__restrict__ table, uint32_t *words_out,
    int and_mask, int64_t *first_out, unsigned long long *acc, int64_t *host_chunk_unique, int nchunks) {
    __shared__ uint32_t cnt[2];                  // participating, unique
    __shared__ unsigned long long sums[2];       // bases, bases_unique
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (k >= nchunks) return;
    if (t < 2) cnt[t] = 0;
    if (t < 2) sums[t] = 0;
    __syncthreads();
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records, rb = base[k];
    unsigned long long sB = 0, sU = 0;
    for (uint64_t j0 = 0; j0 < nrec; j0 += 256) {
        const uint64_t j = j0 + t, r = rec0 + rb + j;
        const bool valid = j < nrec;
        bool part = false, uniq = false;
        if (valid) {
            const unsigned long long where = rsc[2 * (rb + j) + 1];
            part = where != kDdNone;
            long long first = -1;
            if (part && where != kDdOver) first = (long long)table[3 * where + 1];
            uniq = first == (long long)r;
            if (first_out) first_out[r] = first;
            if (part) {
                const uint4 d = *(const uint4 *)(recs + 4 * (rb + j));
                const uint32_t L = d.y > d.x ? d.y - d.x - 1 : 0u;
                uint32_t s, Ld;
                dd_key(rows, r, L, max_bases, s, Ld);
                sB += Ld;
                if (uniq) sU += Ld;
            }
        }
        const unsigned long long bp = __ballot(part), bu = __ballot(uniq);
        if (words_out) {
            // the wave's records are bits [R, R + 64) of the mask: at most three words, one lane each
            const unsigned long long bits = and_mask ? __ballot(valid && !uniq) : bu;
            const uint64_t R = rec0 + rb + j0 + (t - lane);
            const uint32_t sh = (uint32_t)(R & 31u);
            if (lane < 3) {
                const uint32_t piece = lane == 0 ? (uint32_t)(bits << sh)
                                     : lane == 1 ? (uint32_t)(bits >> (32 - sh))
                                     : sh ? (uint32_t)(bits >> (64 - sh)) : 0u;
                if (piece) {   // (a set bit is a record of this wave: its word lies below the mask's cap)
                    if (and_mask) atomicAnd(words_out + (R >> 5) + lane, ~piece);
                    else atomicOr(words_out + (R >> 5) + lane, piece);
                }
            }
        }
        if (lane == 0) {
            if (bp) atomicAdd(&cnt[0], (uint32_t)__popcll(bp));
            if (bu) atomicAdd(&cnt[1], (uint32_t)__popcll(bu));
        }
    }
    sB = wave_sum64(sB);
    sU = wave_sum64(sU);
    if (lane == 0) {
        if (sB) atomicAdd(&sums[0], sB);
        if (sU) atomicAdd(&sums[1], sU);
    }
    __syncthreads();
    if (t == 0) {
        *(volatile int64_t *)(host_chunk_unique + k) = (int64_t)cnt[1];
        if (ok && nrec) atomicAdd(acc + 0, (unsigned long long)nrec);
    }
    if (t < 2 && cnt[t]) atomicAdd(acc + 1 + t, (unsigned long long)cnt[t]);
    if (t < 2 && sums[t]) atomicAdd(acc + 3 + t, sums[t]);
}

// A lane per row of the table, after the run's last insert has completed: acc[8 + b] += the rows in bin b,
// acc[24 + b] += their counts, acc[6] = the greatest count.
extern "C" __global__ __launch_bounds__(256) void ppg_dd_levels(const unsigned long long *__restrict__ table,
                                                                 uint64_t slots, unsigned long long *acc) {
    __shared__ uint32_t dist[16];
    __shared__ unsigned long long reads[16], top;
    const uint32_t t = threadIdx.x;
    if (t < 16) dist[t] = 0;
    if (t < 16) reads[t] = 0;
    if (t == 0) top = 0;
    __syncthreads();
    unsigned long long best = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + t; r < slots; r += (uint64_t)gridDim.x * 256) {
        const unsigned long long c = table[3 * r + 2];
        if (table[3 * r] != 0 && c != 0) {
            const uint32_t b = dd_level(c);
            atomicAdd(&dist[b], 1u);
            atomicAdd(&reads[b], c);
            best = max(best, c);
        }
    }
    if (best) atomicMax(&top, best);
    __syncthreads();
    if (t < 16 && dist[t]) atomicAdd(acc + 8 + t, (unsigned long long)dist[t]);
    if (t < 16 && reads[t]) atomicAdd(acc + 24 + t, reads[t]);
    if (t == 0 && top) atomicMax(acc + 6, top);
}

// ... and after ppg_dd_levels has completed: acc[7] (all ones before) = the least first among the rows whose
// count is acc[6].
extern "C" __global__ __launch_bounds__(256) void ppg_dd_maxfirst(const unsigned long long *__restrict__ table,
                                                                   uint64_t slots, unsigned long long *acc) {
    const unsigned long long top = acc[6];
    if (top == 0) return;
    unsigned long long best = ~0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < slots; r += (uint64_t)gridDim.x * 256)
        if (table[3 * r] != 0 && table[3 * r + 2] == top) best = min(best, table[3 * r + 1]);
    if (best != ~0ull) atomicMin(acc + 7, best);
}

// The run's accumulators (kDdAcc values, the layout of a ppg_read_dedup_result) into pinned host memory by
// kernel stores.
extern "C" __global__ __launch_bounds__(64) void ppg_dd_totals(const unsigned long long *__restrict__ acc,
                                                                int64_t *host_result) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)kDdAcc; i += 64) *(volatile int64_t *)(host_result + i) = (int64_t)acc[i];
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); v: the batch (ppg_device.h); table: slots rows, slots a power of two
// ------------------------------------------------------------------------------------------
static unsigned dd_row_blocks(uint64_t slots) { return (unsigned)std::min<uint64_t>((slots + 255) / 256, 4096); }

hipError_t ppg_launch_dd_init(hipStream_t s, uint64_t *table, uint64_t slots) {
    hipLaunchKernelGGL(ppg_dd_init, dim3(dd_row_blocks(slots)), dim3(256), 0, s, (unsigned long long *)table, slots);
    return hipGetLastError();
}

// total: the batch's padded bases (ppg_seq_scan); words: the mask's word 0 under AND_MASK, else null
hipError_t ppg_launch_dd_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, const int64_t *seq_off,
                                 const uint32_t *seq_len, uint64_t total, const PpgReadDedup *dd, const uint32_t *words,
                                 const uint32_t *rows, uint64_t rec0, uint64_t *rsc) {
    const uint64_t units = total / 32;
    if (v.n <= 0 || units == 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_dd_measure, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, v.out, v.jobs, v.offs, v.oref,
                       v.info, v.base, v.recs, cbase, seq_off, seq_len, units, words, rows, rec0, dd->max_bases,
                       (unsigned long long *)rsc, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_dd_insert(hipStream_t s, const PpgBatchView &v, const PpgReadDedup *dd, const uint32_t *words,
                                const uint32_t *rows, uint64_t rec0, uint64_t *rsc, uint64_t *table, uint64_t slots,
                                uint64_t *acc) {
    if (v.n <= 0) return hipSuccess;
    uint32_t lg = 0;
    while ((1ull << lg) < slots) lg++;
    hipLaunchKernelGGL(ppg_dd_insert, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, words, rows, rec0,
                       dd->max_bases, (unsigned long long *)rsc, (unsigned long long *)table, slots, 64u - lg,
                       (unsigned long long *)acc, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_dd_decide(hipStream_t s, const PpgBatchView &v, const PpgReadDedup *dd, const uint32_t *rows,
                                uint64_t rec0, const uint64_t *rsc, const uint64_t *table, uint32_t *words_out,
                                int64_t *first_out, uint64_t *acc, int64_t *host_chunk_unique) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_dd_decide, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, rows, rec0, dd->max_bases,
                       (const unsigned long long *)rsc, (const unsigned long long *)table, words_out,
                       (dd->flags & 0x100) != 0, first_out, (unsigned long long *)acc, host_chunk_unique, v.n);
    return hipGetLastError();
}

// acc[7] must be all ones, acc[6] and acc[8 .. 39] zero before
hipError_t ppg_launch_dd_levels(hipStream_t s, const uint64_t *table, uint64_t slots, uint64_t *acc) {
    hipLaunchKernelGGL(ppg_dd_levels, dim3(dd_row_blocks(slots)), dim3(256), 0, s, (const unsigned long long *)table, slots,
                       (unsigned long long *)acc);
    hipLaunchKernelGGL(ppg_dd_maxfirst, dim3(dd_row_blocks(slots)), dim3(256), 0, s, (const unsigned long long *)table,
                       slots, (unsigned long long *)acc);
    return hipGetLastError();
}

hipError_t ppg_launch_dd_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result) {
    hipLaunchKernelGGL(ppg_dd_totals, dim3(1), dim3(64), 0, s, (const unsigned long long *)acc, host_result);
    return hipGetLastError();
}
