// ppg_seqselect.hip — record selection over a resident batch (include/ppgpu.h "record selection"): the
// records a mask selects, compacted on the device while the text is resident, so that only they cross
// the bus.  The mask is the hit mask of a sequence query (ppg_seqquery.hip) or anything a consumer
// computed per record; the body of the reference's RunPattern loop (Benchmark/Naive.cs:168-179) acts on
// exactly these records.
//
// For record q of chunk k with descriptor (n1, n2, n3, n4) relative to raw_k = offset_k ++ chunk_k the
// text is T = raw_k[a, e), a = 0 for q = 0 and (n4 of record q - 1) + 1 otherwise, e = n4 + 1.
//
//   count    ppg_sel_count, a block per chunk: the selected records of the chunk and the sum of their
//            lengths (a failed chunk: 0 and 0).
//   scan     ppg_sel_scan, one block: the exclusive scans of both over the chunks, and the two totals
//            into pinned host memory by kernel stores (no DMA engine); the host checks the capacities
//            before anything is moved.
//   place    ppg_sel_place, a block per chunk in tiles of 256 records with a running carry: a wave scan
//            by shuffles and an LDS scan over the four waves give every selected record its output
//            index i and its destination offset; it writes recno[i], sel_off[i], the descriptor rebased
//            to the record's first byte as one 16-B store, where the record's bytes come from (PpgSelSrc)
//            into scratch, and, for every multiple of kSelSpan its destination bytes cover, its index into
//            span_first: the copy's blocks start from there and search nothing in HBM.
//   copy     ppg_sel_copy, destination driven: a block owns kSelSpan destination bytes, a thread four
//            16-B words of them.  The block stages the destination offsets and source addresses of the
//            records that reach into its span in LDS (groups of kSelCap when a span holds more), and
//            every word finds its record by a binary search there.  A word is assembled from pieces,
//            a piece being its bytes of one record: a body piece from the aligned dwords that hold it
//            + v_alignbyte (piece_load / piece_merge), a carry piece byte by byte.  A thread takes its
//            words two at a time, in passes: every unfinished word takes its next piece, the loads of
//            a pass go out together, then the pieces are merged.  A word inside one record is one
//            pass, a word that straddles two records is two; a loop per word would pay a memory round
//            trip per piece and word, and at 370 B per record nearly every wave has such a word.
//            Words with a carry piece, or with an end of the batch's range inside, go one by one.
//            Every destination byte is written by exactly one thread, none at or past the batch's
//            range, and no read leaves raw_k apart from the dword over-read of the aligned loads
//            (inside the output buffer and its 64-byte tail, as ppg_seqload.h).
//
// Bytes moved per selected 150 bp record (text 369 B), derived from the formats, not measured: 369 B
// read + 369 B written by the copy, 16 B descriptor read + 16 B written, 8 + 8 B recno / sel_off, 24 B
// source scratch written and read, 8 B sel_off read back: ~850 B; per unselected record 4 B (its n4)
// in each of count and place and one mask bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_seqload.h"

namespace {

constexpr int kSelCap = 512;   // records staged in LDS at a time by ppg_sel_copy

__device__ __forceinline__ bool sel_bit(const uint32_t *mask, uint64_t r) {
    return !mask || ((mask[r >> 5] >> (r & 31u)) & 1u);
}

// [a, e) of record q's text in raw_k; r: the chunk's first descriptor
__device__ __forceinline__ void rec_text(const uint32_t *r, uint64_t q, uint32_t &a, uint32_t &len) {
    a = q ? r[4 * q - 1] + 1u : 0u;
    const uint32_t e = r[4 * q + 3] + 1u;
    len = e > a ? e - a : 0u;
}

__device__ __forceinline__ int32_t clamp_rel(int64_t v) {
    return (int32_t)(v < -1 ? -1 : v > (int64_t)kSelSpan ? (int64_t)kSelSpan : v);
}

// the bytes [a, b) of a dword as a mask (a, b relative to the dword's first byte, any integers)
__device__ __forceinline__ uint32_t byte_mask(int a, int b) {
    a = max(a, 0);
    b = min(b, 4);
    if (b <= a) return 0u;
    const uint32_t below_b = b >= 4 ? 0xFFFFFFFFu : (1u << (8 * b)) - 1u, below_a = a <= 0 ? 0u : (1u << (8 * a)) - 1u;
    return below_b & ~below_a;
}

// A body piece: bytes [lo_b, hi_b) of a 16-B destination word come from address s + lo_b .. (s: where
// the word's byte 0 would come from; it may lie outside raw_k, only the piece's bytes are read).
// piece_load fetches the aligned dwords that hold bytes of the piece, and no others; piece_merge ORs
// the piece's bytes into the word.
__device__ __forceinline__ void piece_load(uintptr_t s, int lo_b, int hi_b, uint32_t (&y)[5]) {
    const uint32_t *sw = (const uint32_t *)(s & ~(uintptr_t)3);
    const int sh = (int)(s & 3);
#pragma unroll
    for (int j = 0; j < 5; j++) y[j] = (4 * j - sh + 4 > lo_b && 4 * j - sh < hi_b) ? sw[j] : 0u;
}

__device__ __forceinline__ void piece_merge(const uint32_t (&y)[5], uintptr_t s, int lo_b, int hi_b, uint32_t (&acc)[4]) {
    const uint32_t sh = (uint32_t)(s & 3);
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] |= __builtin_amdgcn_alignbyte(y[k + 1], y[k], sh) & byte_mask(lo_b - 4 * k, hi_b - 4 * k);
}

}  // namespace

// A block per chunk k of the batch: crec[k] selected records, cbyte[k] their text bytes.  Record q of
// chunk k has mask bit bit0 + base[k] + q (mask null: every record).
extern "C" __global__ __launch_bounds__(256) void ppg_sel_count(const PpgInflateResult *__restrict__ ires,
                                                                const PpgParseInfo *__restrict__ info,
                                                                const uint64_t *__restrict__ base,
                                                                const uint32_t *__restrict__ recs,
                                                                const uint32_t *__restrict__ mask, uint64_t bit0,
                                                                uint64_t *__restrict__ crec, uint64_t *__restrict__ cbyte,
                                                                int nchunks) {
    __shared__ uint64_t pr[4], pb[4];
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (k >= nchunks) return;
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = ok ? info[k].records : 0, m0 = bit0 + base[k];
    const uint32_t *r = recs + 4 * base[k];
    uint64_t nr = 0, nb = 0;
    for (uint64_t q = t; q < nrec; q += 256) {
        if (!sel_bit(mask, m0 + q)) continue;
        uint32_t a, len;
        rec_text(r, q, a, len);
        nr++;
        nb += len;
    }
    nr = wave_sum64(nr);
    nb = wave_sum64(nb);
    if ((t & 63u) == 0) {
        pr[t >> 6] = nr;
        pb[t >> 6] = nb;
    }
    __syncthreads();
    if (t == 0) {
        crec[k] = pr[0] + pr[1] + pr[2] + pr[3];
        cbyte[k] = pb[0] + pb[1] + pb[2] + pb[3];
    }
}

// Exclusive scans of crec / cbyte [0, n) -> rbase / bbase [0, n] (entry n: the totals), and the totals
// (records, bytes) into pinned host memory by kernel stores.  Single workgroup.
extern "C" __global__ __launch_bounds__(1024) void ppg_sel_scan(const uint64_t *__restrict__ crec,
                                                                const uint64_t *__restrict__ cbyte,
                                                                uint64_t *__restrict__ rbase, uint64_t *__restrict__ bbase,
                                                                int64_t *host_totals, int nchunks) {
    __shared__ uint64_t pr[1024], pb[1024];
    const int t = threadIdx.x;
    const int per = (nchunks + 1023) / 1024;
    const int lo = min(nchunks, t * per), hi = min(nchunks, lo + per);
    uint64_t sr = 0, sb = 0;
    for (int k = lo; k < hi; k++) {
        sr += crec[k];
        sb += cbyte[k];
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
        rr += crec[k];
        rb += cbyte[k];
    }
    if (t == 1023) {
        rbase[nchunks] = pr[1023];
        bbase[nchunks] = pb[1023];
        *(volatile int64_t *)(host_totals + 0) = (int64_t)pr[1023];
        *(volatile int64_t *)(host_totals + 1) = (int64_t)pb[1023];
    }
}

// A block per chunk k: the chunk's selected records get output indices rec_lo + rbase[k] + ... and
// destination offsets byte_lo + bbase[k] + ... (both continue from the batches before).  src is
// indexed from the batch's first selected record, span_first from the span that holds byte_lo.
extern "C" __global__ __launch_bounds__(256) void ppg_sel_place(
    const PpgInflateResult *__restrict__ ires, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint32_t *__restrict__ mask, uint64_t bit0,
    const uint64_t *__restrict__ rbase, const uint64_t *__restrict__ bbase, const uint8_t *__restrict__ out,
    const PpgInflateJob *__restrict__ jobs, const uint8_t *__restrict__ offs, const PpgOffsetRef *__restrict__ oref,
    int64_t rec_lo, int64_t byte_lo, int64_t *__restrict__ recno, int64_t *__restrict__ sel_off, uint4 *__restrict__ desc,
    PpgSelSrc *__restrict__ src, int64_t *__restrict__ span_first, int nchunks) {
    __shared__ uint32_t wr[4];
    __shared__ uint64_t wb[4];
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (k >= nchunks) return;
    // the entry after the batch's last selected record
    if (k == 0 && t == 0) sel_off[rec_lo + (int64_t)rbase[nchunks]] = byte_lo + (int64_t)bbase[nchunks];
    if (ires[k].status != 0) return;
    const uint64_t nrec = info[k].records, rb = base[k];
    const uint32_t *r = recs + 4 * rb;
    const uint64_t span0 = (uint64_t)byte_lo / kSelSpan;
    const int64_t olen = (int64_t)oref[k].len;
    const int64_t body = (int64_t)(uintptr_t)(out + jobs[k].out_off) - olen, carry = (int64_t)(uintptr_t)(offs + oref[k].start);
    uint64_t run_r = rbase[k], run_b = bbase[k];
    for (uint64_t q0 = 0; q0 < nrec; q0 += 256) {
        const uint64_t q = q0 + t;
        bool sel = false;
        uint32_t a = 0, len = 0;
        if (q < nrec && sel_bit(mask, bit0 + rb + q)) {
            sel = true;
            rec_text(r, q, a, len);
        }
        // inclusive scans over the wave, then the waves before this one from LDS
        uint32_t c = sel ? 1u : 0u;
        uint64_t b = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t c2 = __shfl_up(c, o, 64);
            const uint64_t b2 = __shfl_up((unsigned long long)b, o, 64);
            if (lane >= (uint32_t)o) {
                c += c2;
                b += b2;
            }
        }
        if (lane == 63) {
            wr[w] = c;
            wb[w] = b;
        }
        __syncthreads();
        uint32_t cpre = 0, ctot = 0;
        uint64_t bpre = 0, btot = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            if (i < w) {
                cpre += wr[i];
                bpre += wb[i];
            }
            ctot += wr[i];
            btot += wb[i];
        }
        if (sel) {
            const uint64_t ib = run_r + cpre + c - 1;                                  // among the batch's selected records
            const uint64_t o = (uint64_t)byte_lo + run_b + bpre + b - len;             // its first destination byte
            const int64_t i = rec_lo + (int64_t)ib;
            recno[i] = (int64_t)(bit0 + rb + q);
            sel_off[i] = (int64_t)o;
            const uint32_t *d = r + 4 * q;
            desc[i] = make_uint4(d[0] - a, d[1] - a, d[2] - a, d[3] - a);
            src[ib] = PpgSelSrc{body + (int64_t)a - (int64_t)o, carry + (int64_t)a - (int64_t)o, (int64_t)o + olen - (int64_t)a};
            // the multiples of kSelSpan inside [o, o + len)
            for (uint64_t x = (o + kSelSpan - 1) / kSelSpan; x * kSelSpan < o + len; x++) span_first[x - span0] = i;
        }
        run_r += ctot;
        run_b += btot;
        __syncthreads();   // wr / wb are rewritten by the next tile
    }
}

// Block x owns destination bytes [max(d0, S), min(d1, S + kSelSpan)), S = (d0 / kSelSpan + x) * kSelSpan, of
// the batch's range [d0, d1) of dst (16-byte aligned); selected records [rec_lo, rec_hi) lie in it.
extern "C" __global__ __launch_bounds__(256) void ppg_sel_copy(const int64_t *__restrict__ sel_off,
                                                               const PpgSelSrc *__restrict__ src,
                                                               const int64_t *__restrict__ span_first, int64_t rec_lo,
                                                               int64_t rec_hi, int64_t d0, int64_t d1,
                                                               uint8_t *__restrict__ dst) {
    // per staged record: its first destination byte relative to the span (clamped to [-1, kSelSpan]),
    // where its offset-carry part ends (likewise), and source address - destination offset for the
    // body part (fast) and the carry part (slow)
    __shared__ int32_t roff[kSelCap + 1], cend[kSelCap];
    __shared__ int64_t fast[kSelCap], slow[kSelCap];
    const uint32_t t = threadIdx.x;
    const int64_t sb = (int64_t)(((uint64_t)d0 / kSelSpan + blockIdx.x) * kSelSpan);
    const int64_t lo = std::max(sb, d0), hi = std::min(sb + (int64_t)kSelSpan, d1);
    const int64_t i_lo = blockIdx.x == 0 ? rec_lo : span_first[blockIdx.x];
    const int64_t i_hi = sb + (int64_t)kSelSpan >= d1 ? rec_hi : span_first[blockIdx.x + 1] + 1;
    for (int64_t g = i_lo; g < i_hi; g += kSelCap) {
        const int cnt = (int)std::min<int64_t>(kSelCap, i_hi - g);
        __syncthreads();   // the group before is done with
        for (int r = (int)t; r <= cnt; r += 256) {
            const int64_t o = sel_off[g + r];
            roff[r] = clamp_rel(o - sb);
            if (r < cnt) {
                const PpgSelSrc sr = src[g + r - rec_lo];
                fast[r] = sr.fast;
                slow[r] = sr.slow;
                cend[r] = clamp_rel(sr.cend - sb);
            }
        }
        __syncthreads();
        // the group's bytes inside this block's range
        const int32_t vlo = std::max(roff[0], (int32_t)(lo - sb)), vhi = std::min(roff[cnt], (int32_t)(hi - sb));
        uint32_t todo = 0;   // the words for the general path below
        int top = 1;
        while (2 * top < cnt) top *= 2;
#pragma unroll 1
        for (int h = 0; h < 2; h++) {   // (two words at a time: four keep too many registers live)
            int32_t p[2], pos[2];
            int r[2] = {0, 0};   // the last record with roff <= pos holds byte pos (roff[0] <= vlo <= pos)
            uint32_t live = 0;   // whole words still being assembled
#pragma unroll
            for (int i = 0; i < 2; i++) {
                p[i] = 16 * ((2 * h + i) * 256 + (int)t);
                const bool act = p[i] + 16 > vlo && p[i] < vhi;
                if (act && p[i] >= vlo && p[i] + 16 <= vhi) live |= 1u << i;
                else if (act) todo |= 1u << (2 * h + i);   // an end of the range inside the word
                pos[i] = std::max(p[i], vlo);
            }
            for (int step = top; step > 0; step >>= 1) {
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int m = r[i] + step;
                    if (m < cnt && roff[m] <= pos[i]) r[i] = m;
                }
            }
            // Passes over two of the thread's whole words: in a pass every unfinished word takes its next
            // piece (the bytes up to the end of the record that holds pos), the loads of both go out
            // together, then the pieces are merged.  A piece in an offset carry sends its word to the
            // general path.
            uint32_t acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            uint32_t busy = live;
            while (busy) {
                uint32_t y[2][5];
                int lo_b[2], hi_b[2];
                uintptr_t s[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    if (!((busy >> i) & 1u)) continue;
                    while (pos[i] >= roff[r[i] + 1]) r[i]++;   // (pos < vhi <= roff[cnt]: r stays below cnt)
                    if (pos[i] < cend[r[i]]) {
                        busy &= ~(1u << i);
                        live &= ~(1u << i);
                        todo |= 1u << (2 * h + i);
                        continue;
                    }
                    lo_b[i] = pos[i] - p[i];
                    hi_b[i] = std::min(16, roff[r[i] + 1] - p[i]);
                    s[i] = (uintptr_t)(fast[r[i]] + sb + p[i]);
                    piece_load(s[i], lo_b[i], hi_b[i], y[i]);
                }
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    if (!((busy >> i) & 1u)) continue;
                    piece_merge(y[i], s[i], lo_b[i], hi_b[i], acc[i]);
                    pos[i] = p[i] + hi_b[i];
                    if (hi_b[i] == 16) busy &= ~(1u << i);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
                if ((live >> i) & 1u) *(uint4 *)(dst + sb + p[i]) = make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        }
        // The general path, a word at a time: its pieces (a run of bytes of one record, all carry or all
        // body) one after the other.
#pragma unroll 1
        for (int i = 0; i < 4; i++) {
            if (!((todo >> i) & 1u)) continue;
            const int32_t pw = 16 * (i * 256 + (int)t);
            const int32_t b0 = std::max(pw, vlo), b1 = std::min(pw + 16, vhi);   // the word's bytes of this group
            int rr = 0;
            for (int step = top; step > 0; step >>= 1) {
                const int m = rr + step;
                if (m < cnt && roff[m] <= b0) rr = m;
            }
            uint32_t acc[4] = {0, 0, 0, 0};
            int32_t pos = b0;
            while (pos < b1) {
                while (pos >= roff[rr + 1]) rr++;   // (pos < vhi <= roff[cnt]: rr stays below cnt)
                const bool carry = pos < cend[rr];
                const int32_t pe = std::min(b1, carry ? std::min(roff[rr + 1], cend[rr]) : roff[rr + 1]);
                const int lo_b = pos - pw, hi_b = pe - pw;   // the piece: bytes [lo_b, hi_b) of the word
                if (!carry) {
                    const uintptr_t s = (uintptr_t)(fast[rr] + sb + pw);
                    uint32_t y[5];
                    piece_load(s, lo_b, hi_b, y);
                    piece_merge(y, s, lo_b, hi_b, acc);
                } else {
                    const uint8_t *sp = (const uint8_t *)(uintptr_t)(slow[rr] + sb + pw);
#pragma unroll
                    for (int b = 0; b < 16; b++)
                        if (b >= lo_b && b < hi_b) acc[b >> 2] |= (uint32_t)sp[b] << (8 * (b & 3));
                }
                pos = pe;
            }
            if (b0 == pw && b1 == pw + 16) {
                *(uint4 *)(dst + sb + pw) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int b = 0; b < 16; b++)
                    if (pw + b >= b0 && pw + b < b1) dst[sb + pw + b] = (uint8_t)(acc[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); v: the batch (ppg_device.h)
// ------------------------------------------------------------------------------------------
hipError_t ppg_launch_sel_count(hipStream_t s, const PpgBatchView &v, const uint32_t *mask, uint64_t bit0, uint64_t *crec,
                                uint64_t *cbyte) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_sel_count, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, mask, bit0, crec, cbyte,
                       v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_sel_scan(hipStream_t s, const uint64_t *crec, const uint64_t *cbyte, uint64_t *rbase,
                               uint64_t *bbase, int64_t *host_totals, int n) {
    hipLaunchKernelGGL(ppg_sel_scan, dim3(1), dim3(1024), 0, s, crec, cbyte, rbase, bbase, host_totals, std::max(n, 0));
    return hipGetLastError();
}

hipError_t ppg_launch_sel_place(hipStream_t s, const PpgBatchView &v, const uint32_t *mask, uint64_t bit0,
                                const uint64_t *rbase, const uint64_t *bbase, int64_t rec_lo, int64_t byte_lo,
                                int64_t *recno, int64_t *sel_off, uint32_t *desc, PpgSelSrc *src, int64_t *span_first) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_sel_place, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, mask, bit0, rbase, bbase,
                       v.out, v.jobs, v.offs, v.oref, rec_lo, byte_lo, recno, sel_off, (uint4 *)desc, src, span_first, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_sel_copy(hipStream_t s, const int64_t *sel_off, const PpgSelSrc *src, const int64_t *span_first,
                               int64_t rec_lo, int64_t rec_hi, int64_t d0, int64_t d1, uint8_t *dst) {
    if (d1 <= d0 || rec_hi <= rec_lo) return hipSuccess;
    const uint64_t blocks = ((uint64_t)d1 + kSelSpan - 1) / kSelSpan - (uint64_t)d0 / kSelSpan;
    hipLaunchKernelGGL(ppg_sel_copy, dim3((unsigned)blocks), dim3(256), 0, s, sel_off, src, span_first, rec_lo, rec_hi, d0,
                       d1, dst);
    return hipGetLastError();
}
