// ppg_seqquery.hip — sequence queries over a resident batch (include/ppgpu.h "sequence queries"): which
// records' Sequence contains a byte pattern, and the census of A / C / G / T / other over every Sequence.
//
// These are the reference's two consumer workloads beside Count(): Benchmark/Naive.cs RunPattern
// (record.Sequence.Contains("GTTATACACTGC")) and Decompressor/Program.cs:20-21 (Sequence.Count(c => c == 'A')).
// Both need only the slice raw_k[n1+1, n2) of every record and return a handful of integers and one bit
// per record, so they run where the text and its descriptors already are; no text crosses the bus.
//
//   layout   as the packed reads (ppg_seqpack.hip): per-chunk sums of P_j = 32 * ceil(L_j / 32), their
//            scan, then seq_off / seq_len per record into shard scratch (ppg_seq_totals, ppg_seq_scan,
//            ppg_seq_offsets, unchanged).
//   query    one thread per 32-base unit (ppg_seq_query): chunk and record by the two binary searches of
//            ppg_seq_pack (unit_lookup, ppg_seqload.h).  The unit counts its own <= 32 bytes and tests the pattern starts it owns,
//            [i0, i0 + 32) n [0, L - m], reading at most 32 + m - 1 bytes of the Sequence and nothing
//            outside it: a match that straddles units is found by exactly the unit that owns its start.
//            The match is shift-and (bitap) with the state in one 64-bit register (m <= 64) and the
//            256 x 64-bit character masks in LDS, built per block from the pattern (a kernel argument).
//            On DNA text nearly all lanes read one of 4-5 entries, and equal addresses broadcast.
//            A hit sets the record's bit with atomicOr (several units of one record may hit).
//            The census is summed per lane, per wave by shuffles, per block in LDS, then one 64-bit
//            atomic add per block and class: integer adds, so exact and independent of the order.
//   reduce   ppg_seq_query_chunks, a block per chunk: popcount of the chunk's records' bits (m = 0:
//            every record of a decoded chunk is a hit, its bits are set here), stored to pinned host
//            memory and added to the run's accumulators; ppg_seq_query_totals stores the accumulators
//            to pinned host memory by a kernel store (as ppg_seq_scan: no DMA engine).
//
// Bytes moved per 150 bp record (P = 160, five units), derived from the formats, not measured: 16 B of
// descriptor x 2 layout passes, 12 B of seq_off / seq_len written and read back, 4 B of descriptor and
// 150 B of Sequence read by the census, and m - 1 more bytes per unit for the pattern (the neighbouring
// unit's, so they come from L2): ~210 B of HBM traffic against the record's 401 B of text + descriptor,
// and one bit written.  Measured (tools/seqquery_probe.py, 2.88 M records of 150 bp, 1.09 GB of text
// resident): query 0.73 ms for the census alone, 0.79 ms with a pattern of 12 or of 64 bytes, layout
// 0.02 + 0.02 ms, reduction 0.03-0.06 ms.  550-600 GB/s of Sequence and a pattern cost that does not
// grow with m: as in ppg_seq_pack the kernel waits for the two searches per unit, not for bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_seqload.h"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // lane 0 holds the sum
}

}  // namespace

// One thread per 32-base unit of the batch.  seq_off / seq_len / recs point at the batch's first
// record; cbase, seq_off are batch-relative (carry 0).  Record j of the batch has bit rec0 + j of
// hit_words (m > 0); acc[3 + c] += bytes of class c (A, C, G, T, other).
extern "C" __global__ __launch_bounds__(256) void ppg_seq_query(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const uint8_t *__restrict__ offs,
    const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase, const int64_t *__restrict__ seq_off,
    const uint32_t *__restrict__ seq_len, uint64_t units, PpgSeqPattern pat, int m, uint32_t *hit_words,
    uint64_t rec0, unsigned long long *acc, int nchunks) {
    __shared__ uint64_t cmask[256];   // bit i of cmask[c]: pat[i] == c
    __shared__ uint32_t bsum[5];
    const uint32_t t = threadIdx.x;
    if (m > 0) {   // (constant indices into the kernel argument: it stays in scalar registers)
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < 64; i++) {
            const uint32_t c = (uint32_t)(pat.w[i >> 3] >> (8 * (i & 7))) & 255u;
            v |= (uint64_t)(i < m && c == t) << i;
        }
        cmask[t] = v;
    }
    if (t < 5) bsum[t] = 0;
    __syncthreads();

    uint32_t nA = 0, nC = 0, nG = 0, nT = 0, nAll = 0;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + t;
    if (u < units) {
        const uint64_t rel = 32 * u;
        int k;
        uint64_t j;
        unit_lookup(cbase, base, info, seq_off, nchunks, rel, 0, k, j);
        const uint32_t i0 = (uint32_t)((int64_t)rel - seq_off[j]);   // the unit's first base within the record
        const uint32_t L = seq_len[j];
        const uint32_t n1 = recs[4 * j];
        const uint8_t *off = offs + oref[k].start, *body = out + jobs[k].out_off;
        const uint64_t olen = oref[k].len;
        // bytes of the Sequence this unit reads: its own 32 and, for the pattern, m - 1 of the next units'
        const uint32_t span = L > i0 ? min(L - i0, 31u + (uint32_t)max(m, 1)) : 0u;
        nAll = min(span, 32u);
        uint64_t state = 0, seen = 0;
        for (uint32_t g = 0; 32 * g < span; g++) {
            const uint32_t gc = min(span - 32 * g, 32u);
            uint32_t x[8];
            load_raw32(off, olen, body, (uint64_t)n1 + 1 + i0 + 32 * g, gc, x);
            if (g == 0) {   // the census of the unit's own bytes (bytes past gc are 0: no class but "other")
#pragma unroll
                for (int i = 0; i < 32; i++) {
                    const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
                    nA += c == 'A';
                    nC += c == 'C';
                    nG += c == 'G';
                    nT += c == 'T';
                }
            }
            if (m > 0) {
#pragma unroll
                for (int i = 0; i < 32; i++) {
                    const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
                    state = ((state << 1) | 1u) & cmask[c];
                    seen |= (uint32_t)i < gc ? state : 0;   // (a pattern may hold NUL bytes: the zero fill is no text)
                }
            }
        }
        if (m > 0 && ((seen >> (m - 1)) & 1u)) {
            const uint64_t r = rec0 + j;
            atomicOr(hit_words + (r >> 5), 1u << (r & 31u));
        }
    }
    const uint32_t nO = nAll - (nA + nC + nG + nT);
    const uint32_t w[5] = {wave_sum(nA), wave_sum(nC), wave_sum(nG), wave_sum(nT), wave_sum(nO)};
    if ((t & 63u) == 0) {
#pragma unroll
        for (int c = 0; c < 5; c++)
            if (w[c]) atomicAdd(&bsum[c], w[c]);
    }
    __syncthreads();
    if (t < 5 && bsum[t]) atomicAdd(acc + 3 + t, (unsigned long long)bsum[t]);
}

// A block per chunk k of the batch: the hits among its records (bits [rec0 + base[k], + records) of
// hit_words) into host_chunk_hits[k] (pinned) and the run's accumulators acc[0] records, acc[1] hits.
// m = 0: every record of a decoded chunk is a hit; with a mask (hit_words != null) its bits are set here.
extern "C" __global__ __launch_bounds__(256) void ppg_seq_query_chunks(const PpgInflateResult *__restrict__ ires,
                                                                        const PpgParseInfo *__restrict__ info,
                                                                        const uint64_t *__restrict__ base, int m,
                                                                        uint32_t *hit_words, uint64_t rec0,
                                                                        unsigned long long *acc,
                                                                        int64_t *host_chunk_hits, int nchunks) {
    __shared__ uint32_t part[4];
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (k >= nchunks) return;
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records, r0 = rec0 + base[k], r1 = r0 + nrec;
    uint32_t n = 0;
    if (nrec && hit_words && (m > 0 || ok)) {
        for (uint64_t wd = (r0 >> 5) + t; wd <= ((r1 - 1) >> 5); wd += 256) {
            // the word's bits that belong to records [r0, r1)
            const uint32_t b0 = wd * 32 < r0 ? (uint32_t)(r0 - wd * 32) : 0u;
            const uint32_t b1 = wd * 32 + 32 > r1 ? (uint32_t)(r1 - wd * 32) : 32u;
            const uint32_t bits = (b1 == 32 ? 0xFFFFFFFFu : (1u << b1) - 1u) & ~((1u << b0) - 1u);
            if (m > 0) n += __popc(hit_words[wd] & bits);
            else atomicOr(hit_words + wd, bits);
        }
    }
    n = wave_sum(n);
    if ((t & 63u) == 0) part[t >> 6] = n;
    __syncthreads();
    if (t == 0) {
        const uint64_t hits = m > 0 ? (uint64_t)part[0] + part[1] + part[2] + part[3] : ok ? nrec : 0;
        *(volatile int64_t *)(host_chunk_hits + k) = (int64_t)hits;
        if (nrec) atomicAdd(acc + 0, (unsigned long long)nrec);
        if (hits) atomicAdd(acc + 1, (unsigned long long)hits);
    }
}

// The run's accumulators as a ppg_seq_query_result (records, hits, bases = the five classes' sum,
// count[5]) into pinned host memory by kernel stores.
extern "C" __global__ __launch_bounds__(64) void ppg_seq_query_totals(const unsigned long long *__restrict__ acc,
                                                                       int64_t *host_result) {
    const uint32_t t = threadIdx.x;
    if (t >= 8) return;
    const unsigned long long v = t == 2 ? acc[3] + acc[4] + acc[5] + acc[6] + acc[7] : acc[t];
    *(volatile int64_t *)(host_result + t) = (int64_t)v;
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); v: the batch (ppg_device.h)
// ------------------------------------------------------------------------------------------
// total: the batch's padded bases (ppg_seq_scan)
hipError_t ppg_launch_seq_query(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, const int64_t *seq_off,
                                const uint32_t *seq_len, uint64_t total, const PpgSeqPattern *pat, int m,
                                uint32_t *hit_words, uint64_t rec0, uint64_t *acc) {
    const uint64_t units = total / 32;
    if (v.n <= 0 || units == 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_seq_query, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, v.out, v.jobs, v.offs, v.oref,
                       v.info, v.base, v.recs, cbase, seq_off, seq_len, units, *pat, m, hit_words, rec0,
                       (unsigned long long *)acc, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_seq_query_chunks(hipStream_t s, const PpgBatchView &v, int m, uint32_t *hit_words, uint64_t rec0,
                                       uint64_t *acc, int64_t *host_chunk_hits) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_seq_query_chunks, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, m, hit_words, rec0,
                       (unsigned long long *)acc, host_chunk_hits, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_seq_query_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result) {
    hipLaunchKernelGGL(ppg_seq_query_totals, dim3(1), dim3(64), 0, s, (const unsigned long long *)acc, host_result);
    return hipGetLastError();
}
