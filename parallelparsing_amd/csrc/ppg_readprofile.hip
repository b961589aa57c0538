// ppg_readprofile.hip — the read profile of a resident batch (include/ppgpu.h "read profile"): per read
// position the bases by class, the Quality bytes, their sum and their histogram, the read-length
// distribution, and per record the GC content and the mean quality as histograms: the report of a QC tool,
// over every record or over those a mask selects, inside the windows a trim left.  The reference has no
// such report: its consumer would walk FastqRecord.Sequence and FastqRecord.Quality on the host; here the
// tables are made where the text already is and 72 x max_pos + 173 numbers leave the device.
//
//   layout   as the other unit kernels: made once per batch by shard_layout, read here.
//   measure  one lane per 32-base unit (ppg_rp_measure), chunk and record by unit_lookup (ppg_seqload.h).
//            A lane whose record has a clear mask bit, or whose unit lies outside the record's window,
//            loads nothing.  The others read their <= 32 bytes of S_j and the bytes of Q_j at the same
//            indices below min(L_j, Lq_j), map index i to position p = i - s_j and count what has
//            p < max_pos into the block's table in LDS.  The per-lane (gc, qn, qsum) over the whole
//            window are summed within the wave segmented by record and added to the record's scratch by
//            each segment's last lane, as ppg_rf_measure does.
//            The table is a two-dimensional histogram, far larger than one tile's events (256 units give
//            ~15 K events for up to 72 x 1,024 counters), so the blocks are persistent: the grid is
//            bounded (the blocks resident on the device, two or three per CU), each block loops over a
//            contiguous share of the 256-unit tiles, accumulates in LDS and flushes its non-zero counters
//            with 64-bit global atomics once per round.
//   LDS      32-bit counters: seven planes (base[5], qual_n, qual_sum) of max_pos rounded up to 32 and the
//            64-bin quality rows of the first T = kRpTile(max_pos) positions, 80 KiB at most, so that two
//            blocks are resident per CU (T covers 256 positions whole; 192 of 1,024).  A quality byte at
//            p >= T goes to the global table by a 64-bit atomic and to the qual_n plane; below T qual_n
//            is not counted per byte: the flush adds every quality row's bins to it.
//   lanes    lane l walks its unit's 32 bytes from byte l & 31 on, wrapping (the registers are rotated
//            once per load, rp_rotate32).  Walked from byte 0, the lanes of equal-length reads meet at a
//            handful of positions in every step (five units per 150 bp record: 13 lanes per address),
//            and same-address LDS adds serialise; rotated, the 32 lanes of an LDS cycle are at 32
//            different positions mod 32, which with strides that are multiples of 32 are 32 banks.
//   overflow one tile adds at most 256 to a counter (a unit holds a position once), 256 x 255 to a
//            qual_sum.  A round is at most kRpRound = 65,536 tiles: 65,536 x 65,280 < 2^32.  A block whose
//            share is longer flushes, zeroes its LDS and goes on.
//   finish   a block per chunk, a thread per record (ppg_rp_finish): the window's length into len_here /
//            longer, gc_j and qsum_j / qn_j from the scratch into gc_hist and meanq_hist, the counts and
//            sums of the fixed result; histograms in LDS, flushed per block.  No text is read.
//   totals   ppg_rp_totals stores the accumulators (the fixed result, then the table) to pinned host memory
//            by kernel stores (as ppg_rt_totals: no DMA engine).
//
// Bytes moved per 150 bp record (five units), derived from the formats, not measured: 150 B of Sequence
// and 150 B of Quality, 12 B of seq_off / seq_len read per unit lookup (cached across a record's units),
// 16 B of descriptor in the measure and 16 B in the finish pass, 16 B of scratch zeroed, added to and read
// (48 B), 8 B of window row and 1 bit of mask, each read twice, when given: ~390-410 B, as the filter.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_seqload.h"

namespace {

constexpr uint64_t kRpRound = 65536;   // tiles between two flushes of a block (see "overflow" above)

// the window (s, w) of a record of Sequence length L: row r of `rows` clamped, or (0, L) without rows
__device__ __forceinline__ void rp_window(const uint32_t *__restrict__ rows, uint64_t r, uint32_t L, uint32_t &s,
                                          uint32_t &w) {
    s = 0;
    w = L;
    if (rows) {
        const uint2 row = *(const uint2 *)(rows + 2 * r);
        s = min(row.x, L);
        w = min(row.y, L - s);
    }
}

__device__ __forceinline__ bool rp_bit(const uint32_t *__restrict__ words, uint64_t r) {
    return !words || ((words[r >> 5] >> (uint32_t)(r & 31u)) & 1u);
}

// The 32 bytes of x rotated down by rot (0 .. 31): byte i of the result is byte (i + rot) & 31 of x.  The
// byte part is one alignbyte per dword, the dword part three conditional moves of the eight registers (no
// dynamic register index).
__device__ __forceinline__ void rp_rotate32(uint32_t (&x)[8], uint32_t rot) {
    uint32_t y[8];
#pragma unroll
    for (int k = 0; k < 8; k++) y[k] = __builtin_amdgcn_alignbyte(x[(k + 1) & 7], x[k], rot & 3u);
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = (rot & 16u) ? y[(k + 4) & 7] : y[k];
#pragma unroll
    for (int k = 0; k < 8; k++) y[k] = (rot & 8u) ? x[(k + 2) & 7] : x[k];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = (rot & 4u) ? y[(k + 1) & 7] : y[k];
}

}  // namespace

// Persistent blocks over the 256-unit tiles of the batch: block b takes tiles [ntiles b / G, ntiles (b + 1) / G).
// seq_off / seq_len / recs / rsc point at the batch's first record; words / rows at the shard's (record j of
// the batch is bit / row rec0 + j; null: no mask / no windows).  Record j gets rsc[2 j] += gc | qn << 32 and
// rsc[2 j + 1] += qsum over its window; table (kRpRow values per position) gets base[5], qual_n, qual_sum
// and qhist of the positions below P.  Dynamic LDS: 4 (7 Pp + 64 T) bytes, Pp = P rounded up to 32, T a
// multiple of 32.
extern "C" __global__ __launch_bounds__(256) void ppg_rp_measure(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const uint8_t *__restrict__ offs,
    const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase, const int64_t *__restrict__ seq_off,
    const uint32_t *__restrict__ seq_len, uint64_t units, const uint32_t *__restrict__ words,
    const uint32_t *__restrict__ rows, uint64_t rec0, uint32_t P, uint32_t T, uint32_t qual_base,
    unsigned long long *rsc, unsigned long long *table, int nchunks) {
    extern __shared__ uint32_t rp_lds[];
    const uint32_t Pp = (P + 31u) & ~31u;
    uint32_t *const pl = rp_lds;            // plane c (A C G T other, qual_n, qual_sum) at pl + c Pp
    uint32_t *const qh = rp_lds + 7 * Pp;   // bin b of position p < T at qh + b T + p
    const uint32_t nlds = 7 * Pp + 64 * T;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    // The lane's first byte.  In step i the lane is at byte (i + rot) & 31 of its unit, so the 32 lanes that
    // share an LDS cycle are at 32 different positions mod 32: with every stride a multiple of 32 they hit 32
    // different banks, whatever their counters, and never one address.  (Started at byte 0, the lanes of
    // equal-length reads would all be at one of a handful of positions in every step: see DESIGN.md.)
    const uint32_t rot = lane & 31u;
    const uint64_t ntiles = (units + 255) / 256;
    uint64_t tile = ntiles / gridDim.x * blockIdx.x + ntiles % gridDim.x * blockIdx.x / gridDim.x;
    const uint64_t t1 = ntiles / gridDim.x * (blockIdx.x + 1) + ntiles % gridDim.x * (blockIdx.x + 1) / gridDim.x;

    while (tile < t1) {   // a round; every thread of the block takes the same rounds and tiles
        for (uint32_t e = t; e < nlds; e += 256) rp_lds[e] = 0;
        __syncthreads();
        const uint64_t tend = min(t1, tile + kRpRound);
        for (; tile < tend; tile++) {
            unsigned long long jkey = ~0ull;   // the unit's record; lanes past the last unit share one key and add nothing
            unsigned long long gq = 0, qs = 0;
            const uint64_t u = tile * 256 + t;
            if (u < units) {
                const uint64_t rel = 32 * u;
                int k;
                uint64_t j;
                unit_lookup(cbase, base, info, seq_off, nchunks, rel, 0, k, j);
                jkey = j;
                const uint64_t i0 = (uint64_t)((int64_t)rel - seq_off[j]);   // the unit's first index within the record
                uint32_t s, w;
                rp_window(rows, rec0 + j, seq_len[j], s, w);
                // the unit's indices inside the window: [i0 + a, i0 + e)
                const uint64_t lo = max((uint64_t)s, i0), hi = min((uint64_t)s + w, i0 + 32);
                if (hi > lo && rp_bit(words, rec0 + j)) {
                    const uint32_t a = (uint32_t)(lo - i0), e = (uint32_t)(hi - i0);
                    const uint32_t n1 = recs[4 * j], n3 = recs[4 * j + 2], n4 = recs[4 * j + 3];
                    const uint64_t Lq = n4 > n3 ? n4 - n3 - 1 : 0u;
                    const uint32_t qe = min(hi, Lq) > i0 ? (uint32_t)(min(hi, Lq) - i0) : 0u;   // Quality at [a, qe)
                    // positions: p = pb + i, counted in the table while i < ep
                    const uint32_t pb = (uint32_t)i0 - s;             // (wraps when i0 < s; + i >= a undoes it)
                    const uint64_t pend = (uint64_t)s + P;            // the first index at position P
                    const uint32_t ep = pend > i0 ? (uint32_t)min(pend - i0, (uint64_t)32) : 0u;
                    const uint8_t *off = offs + oref[k].start, *body = out + jobs[k].out_off;
                    const uint64_t olen = oref[k].len;
                    uint32_t x[8];
                    load_raw32(off, olen, body, (uint64_t)n1 + 1 + i0, e, x);
                    rp_rotate32(x, rot);
                    uint32_t gc = 0;
#pragma unroll
                    for (int i = 0; i < 32; i++) {
                        const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
                        const uint32_t ii = (i + rot) & 31u;   // the byte's index in the unit
                        if (ii >= a && ii < e) {
                            const uint32_t cls = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
                            gc += cls == 1u || cls == 2u;
                            if (ii < ep) atomicAdd(&pl[cls * Pp + (pb + ii)], 1u);
                        }
                    }
                    load_raw32(off, olen, body, (uint64_t)n3 + 1 + i0, qe, x);
                    rp_rotate32(x, rot);
                    uint32_t qn = 0, sum = 0;
#pragma unroll
                    for (int i = 0; i < 32; i++) {
                        const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
                        const uint32_t ii = (i + rot) & 31u;
                        if (ii >= a && ii < qe) {
                            qn++;
                            sum += c;
                            if (ii < ep) {
                                const uint32_t p = pb + ii;
                                const uint32_t b = c > qual_base ? min(c - qual_base, 63u) : 0u;
                                atomicAdd(&pl[6 * Pp + p], c);
                                if (p < T) {
                                    atomicAdd(&qh[b * T + p], 1u);
                                } else {
                                    atomicAdd(&pl[5 * Pp + p], 1u);
                                    atomicAdd(table + (uint64_t)kRpRow * p + 8 + b, 1ull);
                                }
                            }
                        }
                    }
                    gq = (unsigned long long)gc | (unsigned long long)qn << 32;
                    qs = sum;
                }
            }
            // sums over the lanes of one record: after the step `o` a lane holds its segment's lanes [lane - 2o + 1, lane]
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long jo = __shfl_up(jkey, o, 64), x0 = __shfl_up(gq, o, 64), x1 = __shfl_up(qs, o, 64);
                if (lane >= (uint32_t)o && jo == jkey) {
                    gq += x0;
                    qs += x1;
                }
            }
            const unsigned long long jn = __shfl_down(jkey, 1, 64);
            if (jkey != ~0ull && (lane == 63u || jn != jkey)) {   // the segment's last lane
                if (gq) atomicAdd(rsc + 2 * jkey, gq);
                if (qs) atomicAdd(rsc + 2 * jkey + 1, qs);
            }
        }
        __syncthreads();
        // the flush: the quality rows first, whose bins also make up qual_n of their positions
        for (uint32_t e = t; e < 64 * T; e += 256) {
            const uint32_t v = qh[e];
            if (v) {
                const uint32_t b = e / T, p = e - b * T;
                atomicAdd(table + (uint64_t)kRpRow * p + 8 + b, (unsigned long long)v);
                atomicAdd(&pl[5 * Pp + p], v);
            }
        }
        __syncthreads();
        for (uint32_t e = t; e < 7 * Pp; e += 256) {
            const uint32_t v = pl[e];
            if (v) {   // (a position at or past P has no counts)
                const uint32_t c = e / Pp, p = e - c * Pp;
                atomicAdd(table + (uint64_t)kRpRow * p + c, (unsigned long long)v);
            }
        }
        __syncthreads();
    }
}

// A block per chunk k of the batch, a thread per record.  From the descriptors, the mask, the rows and the
// scratch of ppg_rp_measure: acc[0] records, acc[1] profiled, acc[2] longer, acc[3] bases, acc[4]
// bases_profiled, acc[5] qual_bytes, acc[6] no_quality, acc[8 + g] gc_hist, acc[109 + q] meanq_hist,
// len_here of the table's row w (acc + kRpFixed), and host_chunk_profiled[k] (pinned).
extern "C" __global__ __launch_bounds__(256) void ppg_rp_finish(
    const PpgInflateResult *__restrict__ ires, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const unsigned long long *__restrict__ rsc, const uint32_t *__restrict__ words,
    const uint32_t *__restrict__ rows, uint64_t rec0, uint32_t P, int64_t qual_base, unsigned long long *acc,
    int64_t *host_chunk_profiled, int nchunks) {
    __shared__ uint32_t lenh[kRpMaxPos];
    __shared__ uint32_t gch[101], mqh[64];
    __shared__ uint32_t cnt[3];                  // profiled, longer, no_quality
    __shared__ unsigned long long sums[3];       // bases, bases_profiled, qual_bytes
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (k >= nchunks) return;
    for (uint32_t e = t; e < P; e += 256) lenh[e] = 0;
    if (t < 101) gch[t] = 0;
    if (t < 64) mqh[t] = 0;
    if (t < 3) cnt[t] = 0;
    if (t < 3) sums[t] = 0;
    __syncthreads();
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records, rb = base[k];
    unsigned long long sW = 0, sP = 0, sQ = 0;
    for (uint64_t j0 = 0; j0 < nrec; j0 += 256) {
        const uint64_t j = j0 + t;
        bool on = false, lng = false, noq = false;
        // (a failed chunk's descriptors are not defined: it contributes nothing)
        if (j < nrec && ok && rp_bit(words, rec0 + rb + j)) {
            on = true;
            const uint4 d = *(const uint4 *)(recs + 4 * (rb + j));
            const uint32_t L = d.y > d.x ? d.y - d.x - 1 : 0u;
            uint32_t s, w;
            rp_window(rows, rec0 + rb + j, L, s, w);
            const unsigned long long g = rsc[2 * (rb + j)], qsum = rsc[2 * (rb + j) + 1];
            const uint32_t gc = (uint32_t)g, qn = (uint32_t)(g >> 32);
            lng = w >= P;
            if (!lng) atomicAdd(&lenh[w], 1u);
            if (w) atomicAdd(&gch[(uint32_t)(100ull * min(gc, w) / w)], 1u);   // (gc <= w: counted inside the window)
            noq = w && !qn;
            if (qn) {
                const unsigned long long zero = (unsigned long long)qual_base * qn;
                atomicAdd(&mqh[qsum <= zero ? 0u : (uint32_t)min((qsum - zero) / qn, 63ull)], 1u);
            }
            sW += w;
            sP += min(w, P);
            sQ += qn;
        }
        const unsigned long long b0 = __ballot(on), b1 = __ballot(lng), b2 = __ballot(noq);
        if (lane == 0) {
            if (b0) atomicAdd(&cnt[0], (uint32_t)__popcll(b0));
            if (b1) atomicAdd(&cnt[1], (uint32_t)__popcll(b1));
            if (b2) atomicAdd(&cnt[2], (uint32_t)__popcll(b2));
        }
    }
    sW = wave_sum64(sW);
    sP = wave_sum64(sP);
    sQ = wave_sum64(sQ);
    if (lane == 0) {
        if (sW) atomicAdd(&sums[0], sW);
        if (sP) atomicAdd(&sums[1], sP);
        if (sQ) atomicAdd(&sums[2], sQ);
    }
    __syncthreads();
    if (t == 0) {
        *(volatile int64_t *)(host_chunk_profiled + k) = (int64_t)cnt[0];
        if (ok && nrec) atomicAdd(acc + 0, (unsigned long long)nrec);
        if (cnt[0]) atomicAdd(acc + 1, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(acc + 2, (unsigned long long)cnt[1]);
        if (cnt[2]) atomicAdd(acc + 6, (unsigned long long)cnt[2]);
    }
    if (t < 3 && sums[t]) atomicAdd(acc + 3 + t, sums[t]);
    if (t < 101 && gch[t]) atomicAdd(acc + 8 + t, (unsigned long long)gch[t]);
    if (t < 64 && mqh[t]) atomicAdd(acc + 109 + t, (unsigned long long)mqh[t]);
    for (uint32_t e = t; e < P; e += 256)
        if (lenh[e]) atomicAdd(acc + kRpFixed + (uint64_t)kRpRow * e + 7, (unsigned long long)lenh[e]);
}

// The run's accumulators (n values: the fixed result, then the table's rows) into pinned host memory by
// kernel stores.
extern "C" __global__ __launch_bounds__(256) void ppg_rp_totals(const unsigned long long *__restrict__ acc,
                                                                 int64_t *host_result, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        *(volatile int64_t *)(host_result + i) = (int64_t)acc[i];
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); v: the batch (ppg_device.h)
// ------------------------------------------------------------------------------------------
// total: the batch's padded bases (ppg_seq_scan); blocks: the grid, cut to the batch's tiles; acc: the
// stage's accumulators (the table follows the fixed result)
hipError_t ppg_launch_rp_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, const int64_t *seq_off,
                                 const uint32_t *seq_len, uint64_t total, const PpgReadProfile *prf,
                                 const uint32_t *words, const uint32_t *rows, uint64_t rec0, uint64_t *rsc,
                                 uint64_t *acc, int blocks, int cus) {
    const uint64_t units = total / 32;
    if (v.n <= 0 || units == 0) return hipSuccess;
    const uint32_t P = (uint32_t)prf->max_pos, T = (uint32_t)kRpTile((int)prf->max_pos);
    const size_t lds = 4 * (size_t)(7 * kRpStride((int)P) + 64 * T);
    const uint64_t ntiles = (units + 255) / 256;
    // The default grid is what is resident: per CU the blocks its 160 KiB of LDS hold, three at most (the
    // kernel's registers allow three waves per SIMD).  More blocks only flush more; fewer leave the lookups'
    // latency uncovered (4.3 / 2.4 / 1.8 / 1.9 ms at one, two, three and eight per CU).
    if (blocks <= 0) blocks = std::max(cus, 1) * (int)std::min<size_t>(3, (160u << 10) / lds);
    const dim3 grid((unsigned)std::min<uint64_t>(ntiles, (uint64_t)blocks));
    // (more than 64 KiB of dynamic LDS is asked for per function; the call is cheap and holds per device)
    const hipError_t e = hipFuncSetAttribute((const void *)ppg_rp_measure, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             4 * kRpLdsWords);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ppg_rp_measure, grid, dim3(256), lds, s, v.out, v.jobs, v.offs, v.oref,
                       v.info, v.base, v.recs, cbase, seq_off, seq_len, units, words, rows, rec0, P, T,
                       (uint32_t)prf->qual_base, (unsigned long long *)rsc, (unsigned long long *)acc + kRpFixed, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_rp_finish(hipStream_t s, const PpgBatchView &v, const uint64_t *rsc, const PpgReadProfile *prf,
                                const uint32_t *words, const uint32_t *rows, uint64_t rec0, uint64_t *acc,
                                int64_t *host_chunk_profiled) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_rp_finish, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs,
                       (const unsigned long long *)rsc, words, rows, rec0, (uint32_t)prf->max_pos, prf->qual_base,
                       (unsigned long long *)acc, host_chunk_profiled, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_rp_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result, uint32_t n) {
    hipLaunchKernelGGL(ppg_rp_totals, dim3(std::min<uint32_t>((n + 255) / 256, 64u)), dim3(256), 0, s,
                       (const unsigned long long *)acc, host_result, n);
    return hipGetLastError();
}
