// ppg_pairoverlap.hip — the overlap of the two mates of a read pair (include/ppgpu.h "pair overlap"): read 1
// against the reverse complement of read 2 without insertions or deletions, which gives the fragment's
// insert size and, when the fragment is shorter than a read, the exact 3' cut of both mates.  The reference
// has nothing of the kind; a consumer would take both files' text to the host.  Here both files are packed
// reads (ppg_seqpack.hip: 2 bits per base and an N bit, 32 bases per 64-bit word), so a candidate offset is
// a shift, an XOR and a popcount per 32 bases, and both files stay resident where their texts cannot.
//
//   wave     one wave64 per pair, and a tile of 64 consecutive pairs per wave; the blocks are persistent: block
//            b takes tiles 4 b + w, then strides by the grid.  Lane l first fetches pair l's map entries, lengths
//            and offsets (two dependent trips to memory per 64 pairs, not per pair); pair i's are then read from
//            lane i into scalar registers, so every branch on them is wave-uniform.  The words of pair i + 1
//            are loaded into registers before pair i is searched, so their latency hides behind the search.
//   stage    lane k < 34 makes word k of four planes in LDS, zero past the reads' words:
//              A, NA   read 1's bases and its N bits spread to the even bits (bit b of a mask word to bit 2 b);
//              R, NR   the reverse complement of read 2: word k of the reversed read is word W2 - 1 - k with
//                      its 64 bits reversed and the two bits of every base swapped back, complemented; the
//                      N bits are the mask word's 32 bits reversed and spread.  Reversing whole words
//                      reverses the padded read, so the planes are shifted down by the pad 32 W2 - L2 (a
//                      funnel shift with the next lane's word, by a shuffle).  The complement of the pad's
//                      zeros is shifted out; past L2 the planes are 0.
//   search   the candidates that can be accepted at all have ov(d) >= min_overlap: d = 0 .. L1 - min_overlap,
//            then d = -1 .. -(L2 - min_overlap), which is the order of the semantics with the others left
//            out.  Lane l of round r takes candidate 64 r + l.  For d >= 0 read 1 moves (32 bases from base
//            d + 32 w: two adjacent words funnel-shifted) and R stands (word w, one address for the wave:
//            a broadcast); for d < 0 the other way round.  x = moving ^ standing, (x | x >> 1) & 0x5555..
//            folds each base's two bits to one, OR both N planes, AND the overlap's valid bits, popcount.  A
//            lane leaves its candidate once mis exceeds lim = min(max_diff, max_err_milli ov / 1000), which is
//            "mis <= max_diff and 1000 mis <= max_err_milli ov" in integers.  After a round the lowest set
//            bit of the ballot is the first accepted candidate; its lane's (d, ov, mis) go to every lane.
//   LDS      neighbouring lanes hold neighbouring d, so a round reads at most three different words of a
//            moving plane per step: broadcasts, no bank conflicts to speak of.  4 waves x 4 planes x 34 words
//            + the block's totals and its 2,048 insert-size bins: 12.4 KiB.
//   outputs  lane i keeps pair i's result; after the tile every lane writes its row (16 bytes, the wave's rows
//            are contiguous), clips its two windows rows (read, clip to the insert size, write; a record is in at
//            most one pair), and the wave's ballot is the tile's two found words, written whole.  Totals are
//            reduced in the wave, added with the histogram in LDS and flushed by 64-bit global atomics once per
//            block.
//
// Work per 150 / 150 pair at min_overlap 30: at most 241 candidates of at most 5 words; an unrelated pair
// leaves nearly every candidate after its first word (32 random bases differ in ~24 places).  Memory per pair:
// 2 x (40 B of bases + 20 B of mask + 12 B of seq_off / seq_len), 16 B of row, 2 x 16 B of windows: the stage is
// bound by the compares, not the bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_pairbits.h"

namespace {

constexpr int kPoWaves = 4;                    // pairs in flight per block
constexpr int kPoRow = kPoMaxLen / 32 + 2;     // words of a plane: the longest read's 32, and zeros a funnel shift reads
// (po_spread, po_reverse, po_funnel: ppg_pairbits.h)

// the 32 bases from base `pos` on of a plane (pos + 32 <= 32 (kPoRow - 1))
__device__ __forceinline__ uint64_t po_fetch(const uint64_t *pl, uint32_t pos) {
    const uint32_t q = pos >> 5;
    return po_funnel(pl[q], pl[q + 1], 2u * (pos & 31u));
}

// LDS operations of one wave complete in order: between a wave's writes and its reads of other lanes' words
// only the compiler has to keep the order
__device__ __forceinline__ void po_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a windows row clipped to the insert size I: (s', e - s') or (0, 0)
__device__ __forceinline__ void po_clip(uint2 *win, int64_t r, uint32_t L, uint32_t I) {
    const uint2 row = win[r];
    const uint32_t s = min(row.x, L), n = min(row.y, L - s), e = min(s + n, I);
    win[r] = e > s ? make_uint2(s, e - s) : make_uint2(0u, 0u);
}

// the words of a pair as they are loaded: lane k holds word k of read 1 and word W2 - 1 - k of read 2
struct PoWords {
    uint64_t a, b;
    uint32_t ma, mb;
};

// (L1, L2, u1, u2: the pair's lengths and first 32-base units, the same in every lane; on: the pair is analysed)
__device__ __forceinline__ PoWords po_load(const PpgPackedView &s1, const PpgPackedView &s2, uint32_t lane, uint32_t L1,
                                           uint32_t L2, int64_t u1, int64_t u2, bool on) {
    PoWords w = {0, 0, 0, 0};
    const uint32_t W1 = on ? (L1 + 31u) >> 5 : 0u, W2 = on ? (L2 + 31u) >> 5 : 0u;
    if (lane < W1) {
        w.a = ((const uint64_t *)s1.bases)[u1 + lane];
        w.ma = s1.mask[u1 + lane];
    }
    if (lane < W2) {
        w.b = ((const uint64_t *)s2.bases)[u2 + (W2 - 1u - lane)];
        w.mb = s2.mask[u2 + (W2 - 1u - lane)];
    }
    return w;
}

// lane i's value in a scalar register (i the same in every lane)
__device__ __forceinline__ uint32_t po_from(uint32_t v, int i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, i); }
__device__ __forceinline__ int64_t po_from64(int64_t v, int i) {
    return (int64_t)(((uint64_t)po_from((uint32_t)((uint64_t)v >> 32), i) << 32) | po_from((uint32_t)v, i));
}

// the sum of v over the wave's lanes, in every lane (v < 2^26)
__device__ __forceinline__ uint32_t po_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

// min_ov in [1, kPoMaxLen + 1], max_diff in [0, kPoMaxLen] (the launcher clamps: a read has kPoMaxLen bases
// at most).  rows / found / win1 / win2 may be null.  acc: kPoAcc totals, then kPoHist bins.  Eight waves per
// SIMD (64 VGPRs): the default grid of eight blocks per CU is resident at once, no block waits for another's end.
extern "C" __global__ __launch_bounds__(256, 8) void ppg_po_overlap(
    const PpgPackedView s1, const PpgPackedView s2, const int64_t *__restrict__ rec1, const int64_t *__restrict__ rec2,
    int64_t npairs, int min_ov, int max_diff, uint32_t err_milli, int4 *__restrict__ rows, uint32_t *found,
    uint2 *win1, uint2 *win2, unsigned long long *acc) {
    __shared__ uint64_t planes[kPoWaves][4][kPoRow];
    __shared__ unsigned long long tot[kPoAcc];
    __shared__ uint32_t hist[kPoHist];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    if (t < kPoAcc) tot[t] = 0;
    for (uint32_t e = t; e < kPoHist; e += 256) hist[e] = 0;
    __syncthreads();
    uint64_t *const A = planes[wave][0], *const NA = planes[wave][1], *const R = planes[wave][2], *const NR = planes[wave][3];
    const int64_t ntiles = (npairs + 63) / 64;

    for (int64_t tile = (int64_t)blockIdx.x * kPoWaves + wave; tile < ntiles; tile += (int64_t)gridDim.x * kPoWaves) {
        const int64_t p0 = tile * 64;
        const int n = (int)min((int64_t)64, npairs - p0);   // the tile's pairs; the same in every lane
        // lane l: pair p0 + l
        int64_t r1 = -1, r2 = -1, u1 = 0, u2 = 0;
        uint32_t L1 = 0, L2 = 0;
        bool mapped = false;
        if ((int)lane < n) {
            r1 = rec1 ? rec1[p0 + lane] : p0 + lane;
            r2 = rec2 ? rec2[p0 + lane] : p0 + lane;
            mapped = r1 >= 0 && r1 < s1.records && r2 >= 0 && r2 < s2.records;
            if (mapped) {
                L1 = s1.seq_len[r1];
                L2 = s2.seq_len[r2];
                u1 = s1.seq_off[r1] >> 5;   // the reads' first 32-base units
                u2 = s2.seq_off[r2] >> 5;
            }
        }
        const bool too_long = L1 > (uint32_t)kPoMaxLen || L2 > (uint32_t)kPoMaxLen;
        const uint64_t on = __ballot(mapped && !too_long);   // the pairs that are analysed
        bool hit = false;                                    // the lane's own pair
        int d = 0, ov = 0, mis = 0;

        PoWords cur = po_load(s1, s2, lane, po_from(L1, 0), po_from(L2, 0), po_from64(u1, 0), po_from64(u2, 0), on & 1u);
        for (int i = 0; i < n; i++) {
            const uint32_t l1 = po_from(L1, i), l2 = po_from(L2, i);
            const int j = min(i + 1, 63);   // the next pair's words, on their way during this pair's search
            const PoWords nxt = po_load(s1, s2, lane, po_from(L1, j), po_from(L2, j), po_from64(u1, j), po_from64(u2, j),
                                        i + 1 < n && ((on >> j) & 1u));
            if ((on >> i) & 1u) {
                const uint32_t W2 = (l2 + 31u) >> 5, pad = 32u * W2 - l2;
                const uint64_t rp = lane < W2 ? ~po_reverse(cur.b) : 0ull, nrp = po_spread(__brev(cur.mb));
                // (W2 <= 32: the lanes from W2 on, lane 63 among them, hold 0)
                const uint64_t r = po_funnel(rp, __shfl_down(rp, 1), 2u * pad);
                const uint64_t nr = po_funnel(nrp, __shfl_down(nrp, 1), 2u * pad);
                po_wave_sync();   // the pair before has been read
                if (lane < (uint32_t)kPoRow) {
                    A[lane] = cur.a;
                    NA[lane] = po_spread(cur.ma);
                    R[lane] = r;
                    NR[lane] = nr;
                }
                po_wave_sync();

                int npos = 0, nneg = 0;   // the candidates with ov >= min_ov: d = 0 .. npos - 1, then -1 .. -nneg
                if ((int)l1 >= min_ov && (int)l2 >= min_ov) {
                    npos = (int)l1 - min_ov + 1;
                    nneg = (int)l2 - min_ov;
                }
                const int ncand = npos + nneg;
                for (int c0 = 0; c0 < ncand; c0 += 64) {
                    const int c = c0 + (int)lane;
                    bool ok = false;
                    int cd = 0, cov = 0, cmis = 0;
                    if (c < ncand) {
                        const bool neg = c >= npos;
                        const int sh = neg ? c - npos + 1 : c;   // |d|
                        cd = neg ? -sh : sh;
                        cov = neg ? min((int)l1, (int)l2 - sh) : min((int)l1 - sh, (int)l2);
                        const int lim = min(max_diff, (int)(err_milli * (uint32_t)cov / 1000u));
                        const uint64_t *const M = neg ? R : A, *const NM = neg ? NR : NA;   // the side that moves
                        const uint64_t *const F = neg ? A : R, *const NF = neg ? NA : NR;
                        for (int w = 0, left = cov; left > 0 && cmis <= lim; w++, left -= 32) {
                            const uint32_t pos = (uint32_t)(sh + 32 * w);
                            uint64_t x = po_fetch(M, pos) ^ F[w];
                            x = ((x | (x >> 1)) & kPoEven) | po_fetch(NM, pos) | NF[w];
                            if (left < 32) x &= (1ull << (2 * left)) - 1ull;
                            cmis += __popcll(x);
                        }
                        ok = cmis <= lim;   // (then the loop has seen the whole overlap)
                    }
                    const uint64_t b = __ballot(ok);
                    if (b) {
                        const int first = __ffsll((unsigned long long)b) - 1;
                        const int wd = __shfl(cd, first), wov = __shfl(cov, first), wmis = __shfl(cmis, first);
                        if ((int)lane == i) {   // pair i's lane keeps the answer
                            d = wd;
                            ov = wov;
                            mis = wmis;
                            hit = true;
                        }
                        break;
                    }
                }
            }
            cur = nxt;
        }

        // lane l: pair p0 + l's outputs
        const uint32_t I = hit ? (uint32_t)((int)L2 + d) : 0u;
        if ((int)lane < n && rows) rows[p0 + lane] = hit ? make_int4(d, ov, mis, (int)I) : make_int4(0, 0, 0, 0);
        if (hit) {
            if (win1) po_clip(win1, r1, L1, I);
            if (win2) po_clip(win2, r2, L2, I);
            atomicAdd(&hist[I], 1u);   // I = L2 + d < L2 + L1 <= kPoHist
        }
        const uint64_t hits = __ballot(hit);
        const uint32_t s_ov = po_wave_sum(hit ? (uint32_t)ov : 0u), s_mis = po_wave_sum(hit ? (uint32_t)mis : 0u);
        const uint32_t s_c1 = po_wave_sum(hit && L1 > I ? L1 - I : 0u), s_c2 = po_wave_sum(hit && L2 > I ? L2 - I : 0u);
        const uint64_t b_map = __ballot(mapped), b_neg = __ballot(hit && d < 0), b_ad = __ballot(hit && (I < L1 || I < L2));
        if (lane == 0) {
            if (found) {   // the tile's words, whole
                found[p0 >> 5] = (uint32_t)hits;
                if (n > 32) found[(p0 >> 5) + 1] = (uint32_t)(hits >> 32);
            }
            atomicAdd(&tot[0], (unsigned long long)n);
            atomicAdd(&tot[1], (unsigned long long)(n - __popcll(b_map)));
            atomicAdd(&tot[2], (unsigned long long)(__popcll(b_map) - __popcll(on)));
            atomicAdd(&tot[3], (unsigned long long)__popcll(on));
            atomicAdd(&tot[4], (unsigned long long)__popcll(hits));
            atomicAdd(&tot[5], (unsigned long long)__popcll(b_neg));
            atomicAdd(&tot[6], (unsigned long long)__popcll(b_ad));
            atomicAdd(&tot[7], (unsigned long long)s_ov);
            atomicAdd(&tot[8], (unsigned long long)s_mis);
            atomicAdd(&tot[9], (unsigned long long)s_c1);
            atomicAdd(&tot[10], (unsigned long long)s_c2);
        }
    }
    __syncthreads();
    if (t < kPoAcc && tot[t]) atomicAdd(&acc[t], tot[t]);
    for (uint32_t e = t; e < kPoHist; e += 256)
        if (hist[e]) atomicAdd(&acc[kPoAcc + e], (unsigned long long)hist[e]);
}

// blocks: the grid (<= 0: the default, eight blocks per CU, which is every wave slot of the device), cut to
// the blocks the pairs' tiles of 64 fill.
hipError_t ppg_launch_pair_overlap(hipStream_t s, const PpgPackedView &s1, const PpgPackedView &s2, const int64_t *rec1,
                                   const int64_t *rec2, int64_t npairs, const PpgPairOverlap *po, int32_t *rows,
                                   uint32_t *found, uint32_t *win1, uint32_t *win2, uint64_t *acc, int blocks, int cus) {
    static_assert(2 * kPoMaxLen <= kPoHist && kPoRow <= 64, "an insert size has a bin, a plane a lane per word");
    if (npairs <= 0) return hipSuccess;
    if (blocks <= 0) blocks = 8 * std::max(cus, 1);
    const int64_t ntiles = (npairs + 63) / 64;
    const dim3 grid((unsigned)std::min<int64_t>((ntiles + kPoWaves - 1) / kPoWaves, (int64_t)blocks));
    hipLaunchKernelGGL(ppg_po_overlap, grid, dim3(256), 0, s, s1, s2, rec1, rec2, npairs,
                       (int)std::min<int64_t>(po->min_overlap, kPoMaxLen + 1), (int)std::min<int64_t>(po->max_diff, kPoMaxLen),
                       (uint32_t)po->max_err_milli, (int4 *)rows, found, (uint2 *)win1, (uint2 *)win2,
                       (unsigned long long *)acc);
    return hipGetLastError();
}
