// ppg_pairmerge.hip — one consensus read per overlapping pair (include/ppgpu.h "pair merge"): with the row
// (d, ., ., I) the pair overlap found, the fragment's I bases in read-1 coordinates, every base that both
// mates cover decided by the better of the two observations.  The reference has nothing of the kind.  Both
// files are packed reads with qualities (ppg_seqpack.hip) and the result is a third packed read set, so no
// read text leaves the device and every consumer of packed reads takes the merged reads as they are.
//
//   count    ppg_pm_count, one thread per pair and a tile of 256 pairs per block: map entries, lengths, the
//            row (one 16-byte load into registers; every check in 64-bit before anything is derived from it)
//            and the class of the semantics.  A merged pair has M = I bases and P = 32 ceil(M / 32) padded
//            ones; the block writes its tile's merged records and padded bases.
//   scan     ppg_pm_scan, one block: the exclusive scans of both over the tiles, and the two totals to pinned
//            host memory by kernel stores (the shape of ppg_sel_scan).  The host checks the caps with them.
//   place    ppg_pm_place, the count's mapping again: a merged pair's rank in its tile (ballots and a scan of
//            P in the wave, four partial sums in LDS) on top of the tile's bases gives its record m and
//            seq_off[m]; it writes seq_off, seq_len, pair_of and a 32-byte PpgMergeRec (both reads' first
//            units, their lengths and d), so the emit reads no map, no row and no hostile value.  The class
//            counters are ballots per wave, added in LDS, flushed by 64-bit global atomics once per block.
//   emit     ppg_pm_emit, one thread per 32-base unit of the output, not a wave per pair: a 150 / 150 pair has
//            at most 10 units, a wave per pair would leave 54 lanes idle (ppg_seqpack.hip made the same choice).
//            Unit u finds its record by a binary search of the output seq_off: ceil(log2(merged)) dependent
//            loads (21 for 1.6 M records; the first ~12 levels are the same lines for every thread and stay in
//            L2), then one PpgMergeRec, then the planes: 3 trips to memory after the search.  With k the unit
//            in its record, side 1 is word k of read 1 (8 B of bases, 4 B of mask, 32 B of qual, all aligned).
//            Side R is the 32 read-2 positions from M - 1 - 32 k downwards: two adjacent base words and mask
//            words funnel-shifted to the run's start, then reversed (and the bases complemented); its 32 quality
//            bytes are an unaligned run of read 2's qual plane, loaded as three aligned 16-byte words, shifted
//            by words and bytes in registers and byte-reversed.  Every word index is clipped to the record's
//            own words before the load; what is outside is 0 and never covered.  The choice is lane-local: the
//            "qR > q1" of 32 positions is eight dword compares of four bytes each (pm_gt4), the N bits and the
//            cover bits are 32-bit masks, the bases are picked through masks spread to two bits.  Each thread
//            stores one uint2 of bases, one mask word and two uint4 of qual: a wave writes 512 + 256 + 2,048
//            contiguous bytes.  The thresholds of "corrected" and the ties are only looked at in units with a
//            disagreement.  Counters: popcounts per unit, summed per thread over its units, reduced in the
//            wave, added in LDS, flushed by 64-bit global atomics once per block.  The blocks are persistent:
//            by default four per CU (every wave slot its registers leave), cut to the units' tiles.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), VGPRs / SGPRs / LDS / waves per SIMD, scratch 0
// in all: count 12 / 28 / 32 B / 8, scan 20 / 24 / 16 KiB / 8 (one block), place 54 / 44 / 96 B / 8, emit 110 / 64 / 64 B / 4.
// Memory for a hypothetical merged 150 / 150 pair with I = 200 (7 units) whose every word is touched: 2 x 232 B of
// packed reads with qualities read, 7 x 44 B = 308 B written, 32 B of PpgMergeRec each way.  (DESIGN.md section 6
// quotes other figures, 404 B in and 231 B out: those are the mean over the probe's merged reads, whose mean I is
// 152, with the words of a mate past I left out because they are never touched.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_pairbits.h"

namespace {

enum : uint32_t { kUnmapped = 0, kTooLong = 1, kUnmerged = 2, kStale = 3, kMerged = 4 };

struct PmPair {
    uint32_t cls, L1, L2, M;
    int32_t d;
    int64_t r1, r2;
};

// pair i's class.  The row is read once; d and I are compared as int64 before M is taken from them.
__device__ __forceinline__ PmPair pm_classify(const PpgPackedView &s1, const PpgPackedView &s2, const int64_t *rec1,
                                              const int64_t *rec2, const int4 *rows, int64_t i) {
    PmPair p = {kUnmapped, 0, 0, 0, 0, 0, 0};
    p.r1 = rec1 ? rec1[i] : i;
    p.r2 = rec2 ? rec2[i] : i;
    if (!(p.r1 >= 0 && p.r1 < s1.records && p.r2 >= 0 && p.r2 < s2.records)) return p;
    p.L1 = s1.seq_len[p.r1];
    p.L2 = s2.seq_len[p.r2];
    if (p.L1 > (uint32_t)kPoMaxLen || p.L2 > (uint32_t)kPoMaxLen) {
        p.cls = kTooLong;
        return p;
    }
    const int4 row = rows[i];
    const int64_t d = row.x, I = row.w, l1 = p.L1, l2 = p.L2;
    if (I == 0) {
        p.cls = kUnmerged;
    } else if (!(-l2 < d && d < l1 && I == l2 + d)) {
        p.cls = kStale;
    } else {   // 1 <= I <= 2 kPoMaxLen - 1
        p.cls = kMerged;
        p.d = (int32_t)d;
        p.M = (uint32_t)I;
    }
    return p;
}

__device__ __forceinline__ uint32_t pm_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// the sum of v over the wave's lanes, in every lane
__device__ __forceinline__ uint32_t pm_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t pm_wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o);
    return v;
}

__device__ __forceinline__ uint64_t pm_u64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// the n lowest bits, n = 0 .. 32
__device__ __forceinline__ uint32_t pm_low(uint32_t n) { return n >= 32u ? ~0u : (1u << n) - 1u; }

// the even bits of x (bit 2 b to bit b): po_spread's inverse
__device__ __forceinline__ uint32_t pm_squeeze(uint64_t x) {
    x &= kPoEven;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    return (uint32_t)(x | (x >> 16));
}

// bit b = 1 iff byte b of x exceeds byte b of y (unsigned).  In each half word (y | 0x100) - x keeps bit 8 iff
// y >= x, and is at least 1, so no borrow leaves its half.
__device__ __forceinline__ uint32_t pm_gt4(uint32_t x, uint32_t y) {
    constexpr uint32_t K = 0x00FF00FFu, H = 0x01000100u;
    const uint32_t e = ~(((y & K) | H) - (x & K)) & H;                   // bytes 0 and 2 at bits 8 and 24
    const uint32_t o = ~((((y >> 8) & K) | H) - ((x >> 8) & K)) & H;     // bytes 1 and 3
    const uint32_t v = e | (o << 1);
    return ((v >> 8) & 3u) | ((v >> 22) & 12u);
}

// bits 0 .. 3 of m as the bytes 0x00 / 0xFF of a word
__device__ __forceinline__ uint32_t pm_bytes(uint32_t m) { return (((m & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu; }

// the 32-bit mask of pm_gt4 over eight dwords of four positions each
__device__ __forceinline__ uint32_t pm_gt32(const uint32_t (&x)[8], const uint32_t (&y)[8]) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m |= pm_gt4(x[i], y[i]) << (4 * i);
    return m;
}
__device__ __forceinline__ uint32_t pm_gt32(const uint32_t (&x)[8], uint32_t y) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m |= pm_gt4(x[i], y) << (4 * i);
    return m;
}
__device__ __forceinline__ uint32_t pm_gt32(uint32_t x, const uint32_t (&y)[8]) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m |= pm_gt4(x, y[i]) << (4 * i);
    return m;
}

}  // namespace

// A block per tile of kPmTile pairs: trec[b] its merged pairs, tbase[b] their padded bases.
extern "C" __global__ __launch_bounds__(kPmTile) void ppg_pm_count(const PpgPackedView s1, const PpgPackedView s2,
                                                                   const int64_t *__restrict__ rec1,
                                                                   const int64_t *__restrict__ rec2, int64_t npairs,
                                                                   const int4 *__restrict__ rows, uint64_t *__restrict__ trec,
                                                                   uint64_t *__restrict__ tbase) {
    __shared__ uint32_t wr[kPmTile / 64], wb[kPmTile / 64];
    const uint32_t t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kPmTile + t;
    uint32_t P = 0;
    bool merged = false;
    if (i < npairs) {
        const PmPair p = pm_classify(s1, s2, rec1, rec2, rows, i);
        merged = p.cls == kMerged;
        P = (p.M + 31u) & ~31u;   // (M = 0 unless merged)
    }
    const uint32_t nr = (uint32_t)__popcll(__ballot(merged)), nb = pm_wave_sum(P);
    if ((t & 63u) == 0) {
        wr[t >> 6] = nr;
        wb[t >> 6] = nb;
    }
    __syncthreads();
    if (t == 0) {
        trec[blockIdx.x] = (uint64_t)wr[0] + wr[1] + wr[2] + wr[3];
        tbase[blockIdx.x] = (uint64_t)wb[0] + wb[1] + wb[2] + wb[3];
    }
}

// Exclusive scans of trec / tbase [0, n) -> rbase / bbase [0, n] (entry n: the totals), and the totals (merged
// records, padded bases) into pinned host memory by kernel stores.  Single workgroup.
extern "C" __global__ __launch_bounds__(1024) void ppg_pm_scan(const uint64_t *__restrict__ trec,
                                                               const uint64_t *__restrict__ tbase,
                                                               uint64_t *__restrict__ rbase, uint64_t *__restrict__ bbase,
                                                               int64_t *host_totals, int ntiles) {
    __shared__ uint64_t pr[1024], pb[1024];
    const int t = threadIdx.x;
    const int per = (ntiles + 1023) / 1024;
    const int lo = (int)min((int64_t)ntiles, (int64_t)t * per), hi = (int)min((int64_t)ntiles, (int64_t)lo + per);
    uint64_t sr = 0, sb = 0;
    for (int k = lo; k < hi; k++) {
        sr += trec[k];
        sb += tbase[k];
    }
    pr[t] = sr;
    pb[t] = sb;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint64_t vr = t >= o ? pr[t - o] : 0, vb = t >= o ? pb[t - o] : 0;
        __syncthreads();
        pr[t] += vr;
        pb[t] += vb;
        __syncthreads();
    }
    uint64_t rr = t ? pr[t - 1] : 0, rb = t ? pb[t - 1] : 0;
    for (int k = lo; k < hi; k++) {
        rbase[k] = rr;
        bbase[k] = rb;
        rr += trec[k];
        rb += tbase[k];
    }
    if (t == 1023) {
        rbase[ntiles] = pr[1023];
        bbase[ntiles] = pb[1023];
        *(volatile int64_t *)(host_totals + 0) = (int64_t)pr[1023];
        *(volatile int64_t *)(host_totals + 1) = (int64_t)pb[1023];
    }
}

// A block per tile, as the count: merged record m = rbase[tile] + the pair's rank among the tile's merged pairs,
// seq_off[m] = bbase[tile] + the padded bases of those before it.  Block 0 writes seq_off[merged].  pair_of may be
// null.  acc: the first kPmPlaceAcc accumulators.
extern "C" __global__ __launch_bounds__(kPmTile) void ppg_pm_place(
    const PpgPackedView s1, const PpgPackedView s2, const int64_t *__restrict__ rec1, const int64_t *__restrict__ rec2,
    int64_t npairs, const int4 *__restrict__ rows, const uint64_t *__restrict__ rbase, const uint64_t *__restrict__ bbase,
    int ntiles, int64_t *__restrict__ seq_off, uint32_t *__restrict__ seq_len, int64_t *__restrict__ pair_of,
    PpgMergeRec *__restrict__ recs, unsigned long long *acc) {
    __shared__ uint32_t wr[kPmTile / 64], wb[kPmTile / 64];
    __shared__ unsigned long long tot[kPmPlaceAcc];
    const uint32_t t = threadIdx.x, lane = pm_lane(), w = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * kPmTile + t;
    if (t < (uint32_t)kPmPlaceAcc) tot[t] = 0;
    PmPair p = {kUnmapped, 0, 0, 0, 0, 0, 0};
    const bool in = i < npairs;
    if (in) p = pm_classify(s1, s2, rec1, rec2, rows, i);
    const bool merged = in && p.cls == kMerged;
    const uint32_t P = merged ? (p.M + 31u) & ~31u : 0u;
    // inside the wave: the merged pairs and the padded bases before this lane's pair
    const uint64_t bm = __ballot(merged);
    const uint32_t rank = (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
    uint32_t incl = P;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) {
        wr[w] = (uint32_t)__popcll(bm);
        wb[w] = incl;
    }
    __syncthreads();
    uint64_t m = rbase[blockIdx.x] + rank, off = bbase[blockIdx.x] + (incl - P);
    for (uint32_t v = 0; v < w; v++) {
        m += wr[v];
        off += wb[v];
    }
    if (merged) {
        seq_off[m] = (int64_t)off;
        seq_len[m] = p.M;
        if (pair_of) pair_of[m] = i;
        recs[m] = PpgMergeRec{s1.seq_off[p.r1] >> 5, s2.seq_off[p.r2] >> 5, p.L1, p.L2, p.d, 0u};
    }
    if (blockIdx.x == 0 && t == 0) seq_off[rbase[ntiles]] = (int64_t)bbase[ntiles];
    // the classes and the bases
    const uint64_t b_in = __ballot(in), b_un = __ballot(in && p.cls == kUnmapped), b_long = __ballot(in && p.cls == kTooLong);
    const uint64_t b_none = __ballot(in && p.cls == kUnmerged), b_stale = __ballot(in && p.cls == kStale);
    const uint32_t s_m = pm_wave_sum(p.M);
    if (lane == 0) {
        atomicAdd(&tot[0], (unsigned long long)__popcll(b_in));
        atomicAdd(&tot[1], (unsigned long long)__popcll(b_un));
        atomicAdd(&tot[2], (unsigned long long)__popcll(b_long));
        atomicAdd(&tot[3], (unsigned long long)__popcll(b_none));
        atomicAdd(&tot[4], (unsigned long long)__popcll(b_stale));
        atomicAdd(&tot[5], (unsigned long long)wr[w]);
        atomicAdd(&tot[6], (unsigned long long)s_m);
        atomicAdd(&tot[7], (unsigned long long)wb[w]);
    }
    __syncthreads();
    if (t < (uint32_t)kPmPlaceAcc && tot[t]) atomicAdd(&acc[t], tot[t]);
}

// One thread per 32-base unit of the merged set, the blocks persistent.  recs / seq_off: what ppg_pm_place wrote
// (merged >= 1 records, nunits = seq_off[merged] / 32 units).  hi4 / lo4: qual_hi / qual_lo in every byte.  qual
// may be null.  acc: the kPmAcc accumulators; this kernel adds those from kPmPlaceAcc on.
//   VGPRs 110, SGPRs 64, scratch 0, LDS 64 B: four waves per SIMD (the sixteen quality dwords of both sides, the
//   six words of side R's run and eight 64-bit counters are live together; a bound of 5 or more waves spills), so
//   the default grid of four blocks per CU is resident at once.
extern "C" __global__ __launch_bounds__(256) void ppg_pm_emit(const PpgPackedView s1, const PpgPackedView s2,
                                                              const PpgMergeRec *__restrict__ recs,
                                                              const int64_t *__restrict__ seq_off, int64_t merged,
                                                              int64_t nunits, uint32_t hi4, uint32_t lo4,
                                                              uint2 *__restrict__ bases, uint32_t *__restrict__ mask,
                                                              uint4 *__restrict__ qual, unsigned long long *acc) {
    constexpr int kN = kPmAcc - kPmPlaceAcc;   // overlap_bases, disagree, from2, ties, n_filled, n_both, corrected[2]
    __shared__ unsigned long long tot[kN];
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)kN) tot[t] = 0;
    __syncthreads();
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;   // this thread's share of tot[]

    for (int64_t u = (int64_t)blockIdx.x * 256 + t; u < nunits; u += (int64_t)gridDim.x * 256) {
        // the record that holds base 32 u: the last m with seq_off[m] <= 32 u
        int64_t lo = 0, hi = merged, first = 0;
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1), v = seq_off[mid];
            if (v <= (u << 5)) {
                lo = mid;
                first = v;
            } else {
                hi = mid;
            }
        }
        const PpgMergeRec r = recs[lo];
        const uint32_t L1 = r.L1, L2 = r.L2, M = (uint32_t)((int32_t)L2 + r.d);
        const uint32_t p0 = (uint32_t)(u - (first >> 5)) << 5;   // the unit's first position, < M
        const int32_t d = r.d;
        // the positions of the unit inside the merged read, and those each side covers
        const uint32_t outv = pm_low(M - p0);
        const uint32_t cov1 = p0 < L1 ? pm_low(L1 - p0) & outv : 0u;
        const uint32_t covR = (d <= (int32_t)p0 ? ~0u : ~pm_low((uint32_t)d - p0)) & outv;

        // side 1: word p0 / 32 of read 1
        uint64_t b1 = 0;
        uint32_t n1 = 0, q1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p0 < L1) {
            const int64_t w = r.u1 + (p0 >> 5);
            b1 = ((const uint64_t *)s1.bases)[w];
            n1 = s1.mask[w];
            const uint4 a = ((const uint4 *)s1.qual)[2 * w], b = ((const uint4 *)s1.qual)[2 * w + 1];
            q1[0] = a.x, q1[1] = a.y, q1[2] = a.z, q1[3] = a.w, q1[4] = b.x, q1[5] = b.y, q1[6] = b.z, q1[7] = b.w;
        }

        // side R: position p0 + j faces read-2 position M - 1 - p0 - j; ascending, the run starts at s
        uint64_t bR = 0;
        uint32_t nR = 0, qR[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (covR) {
            const int32_t s = (int32_t)M - 32 - (int32_t)p0, W2 = (int32_t)((L2 + 31u) >> 5);   // s >= -31
            const int32_t w0 = s >> 5;                     // floor: -1 for a negative s
            const uint32_t sh = (uint32_t)s & 31u;
            const bool v0 = w0 >= 0 && w0 < W2, v1 = w0 + 1 >= 0 && w0 + 1 < W2;   // the record's own words
            const uint64_t *const B2 = (const uint64_t *)s2.bases + r.u2;
            const uint32_t *const M2 = s2.mask + r.u2;
            const uint64_t x0 = v0 ? B2[w0] : 0ull, x1 = v1 ? B2[w0 + 1] : 0ull;
            const uint32_t m0 = v0 ? M2[w0] : 0u, m1 = v1 ? M2[w0 + 1] : 0u;
            bR = ~po_reverse(po_funnel(x0, x1, 2u * sh));
            nR = __brev(sh ? (m0 >> sh) | (m1 << (32u - sh)) : m0);
            // the 32 bytes from s on: three 16-byte words from word floor(s / 16) on hold them, as six 64-bit words
            const uint4 *const Q2 = (const uint4 *)s2.qual + 2 * r.u2;
            const int32_t a0 = s >> 4;
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
            const uint4 g0 = a0 >= 0 && a0 < 2 * W2 ? Q2[a0] : z;
            const uint4 g1 = a0 + 1 >= 0 && a0 + 1 < 2 * W2 ? Q2[a0 + 1] : z;
            const uint4 g2 = a0 + 2 >= 0 && a0 + 2 < 2 * W2 ? Q2[a0 + 2] : z;
            const uint64_t e0 = pm_u64(g0.x, g0.y), e1 = pm_u64(g0.z, g0.w), e2 = pm_u64(g1.x, g1.y), e3 = pm_u64(g1.z, g1.w),
                           e4 = pm_u64(g2.x, g2.y), e5 = pm_u64(g2.z, g2.w);
            const bool by8 = (s >> 3) & 1;   // drop a whole word, then s & 7 bytes
            const uint64_t h0 = by8 ? e1 : e0, h1 = by8 ? e2 : e1, h2 = by8 ? e3 : e2, h3 = by8 ? e4 : e3, h4 = by8 ? e5 : e4;
            const uint32_t rb = 8u * ((uint32_t)s & 7u);
            // word e of the run, its bytes reversed, is word 3 - e of the side
            const uint64_t y0 = __builtin_bswap64(po_funnel(h0, h1, rb)), y1 = __builtin_bswap64(po_funnel(h1, h2, rb)),
                           y2 = __builtin_bswap64(po_funnel(h2, h3, rb)), y3 = __builtin_bswap64(po_funnel(h3, h4, rb));
            qR[0] = (uint32_t)y3, qR[1] = (uint32_t)(y3 >> 32), qR[2] = (uint32_t)y2, qR[3] = (uint32_t)(y2 >> 32);
            qR[4] = (uint32_t)y1, qR[5] = (uint32_t)(y1 >> 32), qR[6] = (uint32_t)y0, qR[7] = (uint32_t)(y0 >> 32);
        }

        // the choice: a non-N beats an N, then the higher quality, a tie goes to read 1
        const uint32_t gtR = pm_gt32(qR, q1);
        const uint32_t takeR = covR & (~cov1 | (n1 & ~nR) | (~(n1 ^ nR) & gtR)), take1 = cov1 & ~takeR;
        const uint32_t nout = (takeR & nR) | (take1 & n1);
        const uint64_t bout = (bR & (po_spread(takeR & ~nR) * 3ull)) | (b1 & (po_spread(take1 & ~n1) * 3ull));
        bases[u] = make_uint2((uint32_t)bout, (uint32_t)(bout >> 32));
        mask[u] = nout;
        if (qual) {
            uint32_t qo[8];
#pragma unroll
            for (int e = 0; e < 8; e++) qo[e] = (qR[e] & pm_bytes(takeR >> (4 * e))) | (q1[e] & pm_bytes(take1 >> (4 * e)));
            qual[2 * u] = make_uint4(qo[0], qo[1], qo[2], qo[3]);
            qual[2 * u + 1] = make_uint4(qo[4], qo[5], qo[6], qo[7]);
        }

        const uint32_t both = cov1 & covR;
        if (both) {
            const uint64_t x = b1 ^ bR;
            const uint32_t dis = pm_squeeze(x | (x >> 1)) & both & ~(n1 | nR);   // both non-N, codes differ
            c0 += __popc(both);
            c1 += __popc(dis);
            c2 += __popc(dis & takeR);
            c4 += __popc(both & (n1 ^ nR));
            c5 += __popc(both & n1 & nR);
            if (dis) {
                c3 += __popc(dis & ~gtR & ~pm_gt32(q1, qR));
                // q >= qual_hi: not (qual_hi > q); q <= qual_lo: not (q > qual_lo)
                c6 += __popc(dis & takeR & ~pm_gt32(hi4, qR) & ~pm_gt32(q1, lo4));
                c7 += __popc(dis & ~takeR & ~pm_gt32(hi4, q1) & ~pm_gt32(qR, lo4));
            }
        }
    }

    const uint64_t cs[kN] = {pm_wave_sum64(c0), pm_wave_sum64(c1), pm_wave_sum64(c2), pm_wave_sum64(c3),
                             pm_wave_sum64(c4), pm_wave_sum64(c5), pm_wave_sum64(c6), pm_wave_sum64(c7)};
    if ((t & 63u) < (uint32_t)kN) {   // lane e adds counter e
        uint64_t v = cs[0];
#pragma unroll
        for (int e = 1; e < kN; e++) v = (t & 63u) == (uint32_t)e ? cs[e] : v;
        if (v) atomicAdd(&tot[t & 63u], (unsigned long long)v);
    }
    __syncthreads();
    if (t < (uint32_t)kN && tot[t]) atomicAdd(&acc[kPmPlaceAcc + t], tot[t]);
}

hipError_t ppg_launch_pm_count(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2, const int64_t *rec1,
                               const int64_t *rec2, int64_t npairs, const int32_t *rows, uint64_t *trec, uint64_t *tbase) {
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_pm_count, dim3((unsigned)((npairs + kPmTile - 1) / kPmTile)), dim3(kPmTile), 0, s, s1, s2, rec1, rec2, npairs,
                       (const int4 *)rows, trec, tbase);
    return hipGetLastError();
}

hipError_t ppg_launch_pm_scan(hipStream_t s, const uint64_t *trec, const uint64_t *tbase, uint64_t *rbase, uint64_t *bbase,
                              int64_t *host_totals, int ntiles) {
    hipLaunchKernelGGL(ppg_pm_scan, dim3(1), dim3(1024), 0, s, trec, tbase, rbase, bbase, host_totals, std::max(ntiles, 0));
    return hipGetLastError();
}

hipError_t ppg_launch_pm_place(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2, const int64_t *rec1,
                               const int64_t *rec2, int64_t npairs, const int32_t *rows, const uint64_t *rbase,
                               const uint64_t *bbase, int64_t *seq_off, uint32_t *seq_len, int64_t *pair_of,
                               PpgMergeRec *recs, uint64_t *acc) {
    if (npairs <= 0) return hipSuccess;
    const int ntiles = (int)((npairs + kPmTile - 1) / kPmTile);
    hipLaunchKernelGGL(ppg_pm_place, dim3((unsigned)ntiles), dim3(kPmTile), 0, s, s1, s2, rec1, rec2, npairs,
                       (const int4 *)rows, rbase, bbase, ntiles, seq_off, seq_len, pair_of, recs, (unsigned long long *)acc);
    return hipGetLastError();
}

// blocks: the grid (<= 0: the default, four blocks per CU), cut to the blocks the units fill.
hipError_t ppg_launch_pm_emit(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2, const PpgMergeRec *recs,
                              const int64_t *seq_off, int64_t merged, int64_t padded_bases, const PpgPairMerge *pm,
                              uint32_t *bases, uint32_t *mask, uint8_t *qual, uint64_t *acc, int blocks, int cus) {
    const int64_t nunits = padded_bases / 32;
    if (merged <= 0 || nunits <= 0) return hipSuccess;
    if (blocks <= 0) blocks = 4 * std::max(cus, 1);
    const dim3 grid((unsigned)std::min<int64_t>((nunits + 255) / 256, (int64_t)blocks));
    hipLaunchKernelGGL(ppg_pm_emit, grid, dim3(256), 0, s, s1, s2, recs, seq_off, merged, nunits,
                       (uint32_t)pm->qual_hi * 0x01010101u, (uint32_t)pm->qual_lo * 0x01010101u, (uint2 *)bases, mask,
                       (uint4 *)qual, (unsigned long long *)acc);
    return hipGetLastError();
}
