// ppg_seqpack.hip — packed reads: the records of a resident batch as a structure of arrays
// (include/ppgpu.h "packed reads"): 2-bit bases, a 1-bit "not ACGT" mask and, optionally, the
// qualities as a flat byte plane, every record starting on a 32-base unit.
//
// The reference hands a consumer FastqRecord slices of the text (Parsing.cs:41-47); a read
// consumer then packs the Sequence itself.  Here the pack runs where the text already is: the
// batch's output and its descriptors (n1..n4 per record) are resident after the parse kernels.
//
//   layout   L_j = n2 - n1 - 1 and P_j = 32 * ceil(L_j / 32) per record; per-chunk sums of P_j
//            (ppg_seq_totals), their exclusive scan and the batch total into pinned host memory
//            (ppg_seq_scan, the shape of ppg_scan_counts), then seq_off / seq_len per record from
//            a carried base (ppg_seq_offsets: a block per chunk, 256-record tiles scanned in LDS).
//   pack     one thread per 32-base output unit (ppg_seq_pack), not per record: reads of 36 to
//            2,000 bases would leave most lanes of a per-record mapping idle.  The unit's chunk and
//            record come from two binary searches (unit_lookup, ppg_seqload.h: chunk bases, then the
//            chunk's slice of seq_off; both tables are small and stay in L2).  The unit's 32 source bytes are 9 aligned
//            dwords + v_alignbyte, as ppg_pack_raw loads them (the output buffer has a 64-byte
//            tail); a unit that touches offset_k goes bytewise through offs / oref.  Each thread
//            stores one uint2 of bases, one mask word and two uint4 of qualities, so a wave writes
//            contiguous runs of 512 B, 256 B and 2 KiB.
//
// Bytes moved per 150 bp record (P = 160): 16 B descriptor x 3 passes, ~2 x 160 B of text read
// (sequence + quality; the identifier and '+' lines are never touched beyond the sectors the
// unaligned ends share), 40 + 20 + 160 B written + 12 B of seq_off / seq_len: ~600 B against the
// ~790 B ppg_pack_raw moves for the same record.  Measured (tools/seqpack_probe.py, 2.88 M records
// of 150 bp, 1.09 GB of text resident): pack 0.60 ms with qualities and 0.51 ms without, layout
// 0.02 + 0.02 ms, ppg_pack_raw 0.41 ms on the same batch.  That the quality plane -- 70% of the
// bytes written -- adds only 0.09 ms says the pack is not bandwidth bound: what it waits for is the
// chain of ~20 dependent L2 loads of the two searches per unit, against ~6 ms of decode
// for a quarter of that text.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_seqload.h"

namespace {

// L_j of descriptor r (n1, n2, ..), 0 for a chunk that failed (its descriptors are not defined)
__device__ __forceinline__ uint32_t seq_len_of(const uint32_t *r, bool ok) {
    const uint32_t n1 = r[0], n2 = r[1];
    return ok && n2 > n1 ? n2 - n1 - 1 : 0u;
}
__device__ __forceinline__ uint64_t pad32(uint32_t L) { return ((uint64_t)L + 31) & ~(uint64_t)31; }

}  // namespace

// Per-chunk sum of P_j (padded bases).  Grid: one block per chunk.
extern "C" __global__ __launch_bounds__(256) void ppg_seq_totals(const PpgInflateResult *__restrict__ ires,
                                                                 const PpgParseInfo *__restrict__ info,
                                                                 const uint64_t *__restrict__ base,
                                                                 const uint32_t *__restrict__ recs,
                                                                 uint64_t *__restrict__ ctot, int nchunks) {
    __shared__ uint64_t part[256];
    const int k = blockIdx.x;
    if (k >= nchunks) return;
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records;
    const uint32_t *r = recs + 4 * base[k];
    uint64_t s = 0;
    for (uint64_t j = threadIdx.x; j < nrec; j += 256) s += pad32(seq_len_of(r + 4 * j, ok));
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) ctot[k] = part[0];
}

// Exclusive scan of ctot[0, n) -> cbase[0, n], cbase[n] = the total, which also goes to pinned host
// memory by a kernel store (as ppg_total_to_host: no DMA engine).  Single workgroup.
extern "C" __global__ __launch_bounds__(1024) void ppg_seq_scan(const uint64_t *__restrict__ ctot,
                                                                uint64_t *__restrict__ cbase, uint64_t *host_total,
                                                                int nchunks) {
    __shared__ uint64_t part[1024];
    const int t = threadIdx.x;
    const int per = (nchunks + 1023) / 1024;
    const int lo = min(nchunks, t * per), hi = min(nchunks, lo + per);
    uint64_t s = 0;
    for (int k = lo; k < hi; k++) s += ctot[k];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        uint64_t v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = t ? part[t - 1] : 0;
    for (int k = lo; k < hi; k++) { cbase[k] = run; run += ctot[k]; }
    if (t == 1023) {
        cbase[nchunks] = part[1023];
        *(volatile uint64_t *)host_total = part[1023];
    }
}

// seq_off / seq_len of the batch's records (pointers at the batch's first record): record j of
// chunk k gets carry + cbase[k] + the padded bases of the chunk's records before it.  The entry
// after the batch's last record (carry + total) is written by the last chunk's block.
extern "C" __global__ __launch_bounds__(256) void ppg_seq_offsets(
    const PpgInflateResult *__restrict__ ires, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase, int64_t carry, int64_t *__restrict__ seq_off,
    uint32_t *__restrict__ seq_len, int nchunks) {
    __shared__ uint64_t part[256];
    const int k = blockIdx.x, t = threadIdx.x;
    if (k >= nchunks) return;
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records, rb = base[k];
    const uint32_t *r = recs + 4 * rb;
    uint64_t run = (uint64_t)carry + cbase[k];
    for (uint64_t j0 = 0; j0 < nrec; j0 += 256) {
        const uint64_t j = j0 + t;
        const uint32_t L = j < nrec ? seq_len_of(r + 4 * j, ok) : 0u;
        const uint64_t P = j < nrec ? pad32(L) : 0;
        part[t] = P;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            uint64_t v = t >= o ? part[t - o] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        if (j < nrec) {
            seq_off[rb + j] = (int64_t)(run + part[t] - P);
            seq_len[rb + j] = L;
        }
        run += part[255];
        __syncthreads();
    }
    if (k == nchunks - 1 && t == 0) seq_off[rb + nrec] = (int64_t)((uint64_t)carry + cbase[nchunks]);
}

// One thread per 32-base unit u of the batch (base position carry + 32 u).  seq_off / seq_len / recs
// point at the batch's first record; bases / mask / qual are the planes' starts (indexed by the
// absolute position).  qual may be null.
extern "C" __global__ __launch_bounds__(256) void ppg_seq_pack(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const PpgInflateResult *__restrict__ ires,
    const uint8_t *__restrict__ offs, const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info,
    const uint64_t *__restrict__ base, const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase,
    const int64_t *__restrict__ seq_off, const uint32_t *__restrict__ seq_len, int64_t carry, uint64_t units,
    uint32_t *__restrict__ bases, uint32_t *__restrict__ mask, uint8_t *__restrict__ qual, int nchunks) {
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const uint64_t rel = 32 * u;                 // batch-relative base position
    int k;
    uint64_t j;
    unit_lookup(cbase, base, info, seq_off, nchunks, rel, carry, k, j);
    const int64_t b = carry + (int64_t)rel;
    const uint32_t i0 = (uint32_t)(b - seq_off[j]);     // first base of the unit within the record
    const uint32_t L = seq_len[j];
    const uint32_t n1 = recs[4 * j], n3 = recs[4 * j + 2], n4 = recs[4 * j + 3];
    const uint32_t cnt = L > i0 ? min(L - i0, 32u) : 0u;
    const uint8_t *off = offs + oref[k].start, *body = out + jobs[k].out_off;
    const uint64_t olen = oref[k].len;

    uint32_t x[8];
    load_raw32(off, olen, body, (uint64_t)n1 + 1 + i0, cnt, x);
    uint64_t code = 0;
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
        const uint32_t a = is_acgt(c);
        const uint32_t v = a ? ((c >> 1) ^ (c >> 2)) & 3u : 0u;
        code |= (uint64_t)v << (2 * i);
        m |= ((uint32_t)i < cnt ? a ^ 1u : 0u) << i;
    }
    const uint64_t ab = (uint64_t)b;
    *(uint2 *)(bases + (ab >> 4)) = make_uint2((uint32_t)code, (uint32_t)(code >> 32));
    mask[ab >> 5] = m;
    if (qual) {
        // qual[b] = raw[n3 + 1 + i] while n3 + 1 + i < n4, cut or zero-filled to the sequence's length
        const uint32_t qlen = n4 > n3 ? n4 - n3 - 1 : 0u;
        const uint32_t qend = min(L, qlen);
        const uint32_t qcnt = qend > i0 ? min(qend - i0, 32u) : 0u;
        uint32_t q[8];
        load_raw32(off, olen, body, (uint64_t)n3 + 1 + i0, qcnt, q);
        uint4 *dst = (uint4 *)(qual + ab);
        dst[0] = make_uint4(q[0], q[1], q[2], q[3]);
        dst[1] = make_uint4(q[4], q[5], q[6], q[7]);
    }
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); v: the batch (ppg_device.h)
// ------------------------------------------------------------------------------------------
// per-chunk padded totals of the batch's chunks into ctot
hipError_t ppg_launch_seq_totals(hipStream_t s, const PpgBatchView &v, uint64_t *ctot) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_seq_totals, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, ctot, v.n);
    return hipGetLastError();
}

// cbase[0, n] from ctot[0, n); the total also into pinned host memory (n = 0: a total of 0)
hipError_t ppg_launch_seq_scan(hipStream_t s, const uint64_t *ctot, uint64_t *cbase, uint64_t *host_total, int n) {
    hipLaunchKernelGGL(ppg_seq_scan, dim3(1), dim3(1024), 0, s, ctot, cbase, host_total, std::max(n, 0));
    return hipGetLastError();
}

hipError_t ppg_launch_seq_offsets(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, int64_t carry,
                                  int64_t *seq_off, uint32_t *seq_len) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_seq_offsets, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, cbase, carry, seq_off,
                       seq_len, v.n);
    return hipGetLastError();
}

// total: the batch's padded bases (a multiple of 32)
hipError_t ppg_launch_seq_pack(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, const int64_t *seq_off,
                               const uint32_t *seq_len, int64_t carry, uint64_t total, uint32_t *bases, uint32_t *mask,
                               uint8_t *qual) {
    const uint64_t units = total / 32;
    if (v.n <= 0 || units == 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_seq_pack, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, v.out, v.jobs, v.res, v.offs,
                       v.oref, v.info, v.base, v.recs, cbase, seq_off, seq_len, carry, units, bases, mask, qual, v.n);
    return hipGetLastError();
}
