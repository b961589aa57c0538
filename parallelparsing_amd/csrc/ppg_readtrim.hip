// ppg_readtrim.hip — read trimming over a resident batch (include/ppgpu.h "read trimming"): per record the
// window (start, len) of its Sequence and Quality slices that survives the fixed cuts, the low-quality
// ends, the sliding quality window and the 3' adapter, and the keep bit "still min_len long".  The
// reference has no such step: its consumer would walk FastqRecord.Quality and FastqRecord.Sequence on the
// host; here the window is made where the text already is, and the selection (ppg_seqselect.hip) hands
// out the records with 8 more bytes each.  No text is rebuilt.
//
//   layout   the pack's, unchanged (ppg_seq_totals, ppg_seq_scan, ppg_seq_offsets), made once per batch for
//            the query, the filter and the trim (shard_layout, ppg_stages.cpp).
//   measure  one thread per 32-base unit (ppg_rt_measure), chunk and record by unit_lookup
//            (ppg_seqload.h).  Every cut is decided on [b0, e0) on its own, so a unit gives four
//            candidates among the positions it owns: the least index at or above the leading threshold,
//            1 + the greatest at or above the trailing one, the least start of a failing full window and
//            the least adapter start.  A window or an adapter match belongs to the unit that owns its
//            start, as a query's match does: the unit reads up to W - 1 Quality bytes and up to m - 1
//            Sequence bytes past its own, never past the slices.  The candidates are folded within the
//            wave segmented by record (the Hillis-Steele steps of ppg_rf_measure with min / max for the
//            add) and the last lane of each segment applies them to the record's scratch with atomicMin /
//            atomicMax: records longer than 2,048 bases span waves, longer than 8,192 blocks, and the
//            atomics are what joins them.  The scratch starts at "none found" (all ones for the minima,
//            0 for the maximum: an end found is at least 1).
//            The window sum slides over the unit's 63 Quality bytes in LDS (W is not known at compile
//            time, so a register file of bytes would be indexed dynamically).  The adapter compare reads
//            the unit's <= 95 Sequence bytes from LDS as dwords realigned to the start position, XORs them
//            with the adapter's dwords (LDS, broadcast) and counts the non-zero bytes; a start is left as
//            soon as its mismatch budget floor(max_err_milli * ov / 1000) is spent, which on text that is
//            not the adapter is the first or second dword.  Per-thread LDS rows are 17 and 25 dwords apart:
//            odd strides, no bank conflicts.  The adapter variant is a template argument: a trim without
//            one allocates and reads none of that.
//   decide   a block per chunk, a thread per record (ppg_rt_decide).  Records with L_j = 0 have no unit:
//            their scratch still says "none found", which is their answer.  The thread maps "none" to
//            e0 / b0, combines, writes the row and forms the keep bit by ballot; the mask words are
//            changed by atomicOr / atomicAnd of this wave's bits alone, as in ppg_rf_decide.  The chunk's
//            keeps go to pinned host memory, the totals into the run's accumulators.
//   totals   ppg_rt_totals stores the accumulators, laid out as a ppg_read_trim_result, to pinned host memory.
//   gather   ppg_rt_gather: row i = trim[recno[i] - rec0] for a batch's selected records (the cursor).
//
// Bytes moved per 150 bp record (P = 160, five units), derived from the formats, not measured: 150 B of
// Quality (the windows' look-ahead is the next unit's bytes: L2), 150 B of Sequence with an adapter (the
// look-ahead of m - 1 bytes likewise), 56 B of layout traffic unless a hook before has laid the batch out,
// 16 B of descriptor in the decide pass, 16 B of scratch initialised, updated and read (32-48 B), an 8 B
// row when asked for: ~260-280 B without and ~410-430 B with the adapter, against the filter's ~420-440 B.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_seqload.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;   // a minimum nobody has found

// the number of non-zero bytes of w
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {
    return (uint32_t)__popc((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u);
}

}  // namespace

// One thread per 32-base unit of the batch.  seq_off / seq_len / recs point at the batch's first record;
// cbase, seq_off are batch-relative (carry 0).  rsc holds four planes of `tot` words, record j of the
// batch at word j of each: the minima lead, win, adapt (kNone: none found) and the maximum trail (0: none).
template <bool ADAPT>
__global__ __launch_bounds__(256) void ppg_rt_measure(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const uint8_t *__restrict__ offs,
    const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase, const int64_t *__restrict__ seq_off,
    const uint32_t *__restrict__ seq_len, uint64_t units, PpgReadTrim tr, uint32_t *rsc, uint64_t tot, int nchunks) {
    __shared__ uint32_t qs[256 * 17];                   // per thread: 64 Quality bytes from the unit's first
    __shared__ uint32_t ss[ADAPT ? 256 * 25 : 1];       // per thread: 96 Sequence bytes from the unit's first
    __shared__ uint32_t ad[16];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (ADAPT) {
#pragma unroll
        for (int i = 0; i < 16; i++)   // (constant indices into the kernel argument: it stays in scalar registers)
            if (t == (uint32_t)i) ad[i] = tr.adapter[i];
        __syncthreads();
    }
    const uint32_t ops = (uint32_t)tr.ops;
    unsigned long long jkey = ~0ull;   // the unit's record; lanes past the last unit share one key and find nothing
    uint32_t lead = kNone, win = kNone, adapt = kNone, trail = 0;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + t;
    if (u < units) {
        const uint64_t rel = 32 * u;
        int k;
        uint64_t j;
        unit_lookup(cbase, base, info, seq_off, nchunks, rel, 0, k, j);
        jkey = j;
        const int64_t i0 = (int64_t)rel - seq_off[j];   // the unit's first index within the record
        const int64_t L = seq_len[j];
        const uint32_t n1 = recs[4 * j], n3 = recs[4 * j + 2], n4 = recs[4 * j + 3];
        const int64_t Lq = n4 > n3 ? (int64_t)(n4 - n3 - 1) : 0;
        const int64_t b0 = min(tr.head, L), e0 = max(b0, L - tr.tail);
        // the positions of [b0, e0) this unit owns, as indices [plo, phi) into the unit
        const int64_t p0 = max(b0, i0), p1 = min(e0, i0 + 32);
        if (p0 < p1) {
            const uint32_t plo = (uint32_t)(p0 - i0), phi = (uint32_t)(p1 - i0);
            const uint8_t *off = offs + oref[k].start, *body = out + jobs[k].out_off;
            const uint64_t olen = oref[k].len;
            uint32_t x[8];
            if (ops & 7u) {
                const uint32_t qcnt = Lq > i0 ? (uint32_t)min(Lq - i0, (int64_t)32) : 0u;
                load_raw32(off, olen, body, (uint64_t)n3 + 1 + (uint64_t)i0, qcnt, x);   // (bytes past qcnt are 0: qb)
                if (ops & 3u) {
                    const uint32_t tl = (uint32_t)(tr.qual_base + tr.lead_q), tt = (uint32_t)(tr.qual_base + tr.trail_q);
                    uint32_t gl = 0, gt = 0;
#pragma unroll
                    for (int i = 0; i < 32; i++) {
                        const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
                        gl |= (uint32_t)(c >= tl) << i;
                        gt |= (uint32_t)(c >= tt) << i;
                    }
                    const uint32_t own = (phi == 32u ? ~0u : (1u << phi) - 1u) & ~((1u << plo) - 1u);
                    gl &= own;
                    gt &= own;
                    if ((ops & 1u) && gl) lead = (uint32_t)i0 + (uint32_t)__ffs((int)gl) - 1u;
                    if ((ops & 2u) && gt) trail = (uint32_t)i0 + 32u - (uint32_t)__clz((int)gt);
                }
                const int64_t W = tr.win_size;
                const int64_t w1 = min(p1, e0 - W + 1);   // window starts [p0, w1): the full windows inside [b0, e0)
                if ((ops & 4u) && p0 < w1) {
                    uint32_t *row = qs + 17 * t;
#pragma unroll
                    for (int i = 0; i < 8; i++) row[i] = x[i];
                    // the W - 1 bytes past the unit's own, as far as the Quality slice goes
                    const uint32_t qnext = Lq > i0 + 32 ? (uint32_t)min(Lq - i0 - 32, W - 1) : 0u;
                    load_raw32(off, olen, body, (uint64_t)n3 + 1 + (uint64_t)i0 + 32, qnext, x);
#pragma unroll
                    for (int i = 0; i < 8; i++) row[8 + i] = x[i];
                    const unsigned char *q = (const unsigned char *)row;
                    const int32_t need = (int32_t)(W * (tr.qual_base + tr.win_q)), w = (int32_t)W;
                    const uint32_t whi = (uint32_t)(w1 - i0);   // <= 32
                    int32_t sum = 0;
                    for (int32_t i = 0; i < w; i++) sum += q[plo + (uint32_t)i];
                    for (uint32_t i = plo; i < whi; i++) {   // (q[i + w]: index <= 63)
                        if (sum < need) {
                            win = (uint32_t)i0 + i;
                            break;
                        }
                        sum += (int32_t)q[i + (uint32_t)w] - (int32_t)q[i];
                    }
                }
            }
            if (ADAPT) {
                const int64_t m = tr.adapter_len;
                // the Sequence bytes the unit's starts compare: its own and m - 1 more, none at or past e0
                const int64_t span = min(e0, i0 + 31 + m) - i0;
                uint32_t *row = ss + 25 * t;
#pragma unroll
                for (int g = 0; g < 3; g++) {
                    const uint32_t gc = span > 32 * g ? (uint32_t)min(span - 32 * g, (int64_t)32) : 0u;
                    load_raw32(off, olen, body, (uint64_t)n1 + 1 + (uint64_t)i0 + 32 * g, gc, x);
#pragma unroll
                    for (int i = 0; i < 8; i++) row[8 * g + i] = x[i];
                }
                for (uint32_t s = plo; s < phi; s++) {
                    const int64_t ov = min(m, e0 - (i0 + (int64_t)s));
                    if (ov < tr.min_overlap) break;   // (ov does not grow with s)
                    const uint32_t budget = (uint32_t)(tr.max_err_milli * ov / 1000);   // mis <= budget: 1000 mis <= max_err_milli ov
                    const uint32_t nd = ((uint32_t)ov + 3u) >> 2, sh = s & 3u;
                    const uint32_t *w = row + (s >> 2);   // (w[d + 1]: index <= 7 + 15 + 1)
                    uint32_t mis = 0, a = w[0];
                    for (uint32_t d = 0; d < nd; d++) {
                        const uint32_t b = w[d + 1];
                        uint32_t v = __builtin_amdgcn_alignbyte(b, a, sh) ^ ad[d];
                        a = b;
                        const uint32_t left = (uint32_t)ov - 4u * d;   // bytes of this dword inside the overlap
                        if (left < 4u) v &= (1u << (8u * left)) - 1u;
                        mis += nonzero_bytes(v);
                        if (mis > budget) break;
                    }
                    if (mis <= budget) {
                        adapt = (uint32_t)i0 + s;
                        break;
                    }
                }
            }
        }
    }
    // minima and maximum over the lanes of one record: after the step `o` a lane holds its segment's lanes [lane - 2o + 1, lane]
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long jo = __shfl_up(jkey, o, 64);
        const uint32_t a = __shfl_up(lead, o, 64), b = __shfl_up(win, o, 64), c = __shfl_up(adapt, o, 64),
                       d = __shfl_up(trail, o, 64);
        if (lane >= (uint32_t)o && jo == jkey) {
            lead = min(lead, a);
            win = min(win, b);
            adapt = min(adapt, c);
            trail = max(trail, d);
        }
    }
    const unsigned long long jn = __shfl_down(jkey, 1, 64);
    if (jkey != ~0ull && (lane == 63u || jn != jkey)) {   // the segment's last lane
        if (lead != kNone) atomicMin(rsc + jkey, lead);
        if (win != kNone) atomicMin(rsc + tot + jkey, win);
        if (adapt != kNone) atomicMin(rsc + 2 * tot + jkey, adapt);
        if (trail) atomicMax(rsc + 3 * tot + jkey, trail);
    }
}

// A block per chunk k of the batch, a thread per record.  Combines the candidates and writes: the row
// (start, len) of shard record rec0 + j (trim != null), the record's bit rec0 + j of words (words != null;
// AND_MASK: the bit is cleared when the record is not kept and left alone otherwise, else the words were
// zeroed and the bit is set when it is kept), host_chunk_kept[k] (pinned) and the run's accumulators
// acc[0] records, acc[1] kept, acc[2] trimmed, acc[3..7] cut, acc[8] bases, acc[9] bases_window, acc[10] bases_kept.
extern "C" __global__ __launch_bounds__(256) void ppg_rt_decide(
    const PpgInflateResult *__restrict__ ires, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint32_t *__restrict__ rsc, uint64_t tot, PpgReadTrim tr, uint32_t *words,
    uint64_t rec0, uint32_t *trim, unsigned long long *acc, int64_t *host_chunk_kept, int nchunks) {
    __shared__ uint32_t cnt[7];                  // kept, trimmed, cut[5]
    __shared__ unsigned long long sums[3];       // bases, bases_window, bases_kept
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (k >= nchunks) return;
    if (t < 7) cnt[t] = 0;
    if (t < 3) sums[t] = 0;
    __syncthreads();
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records, rb = base[k];
    const uint32_t ops = (uint32_t)tr.ops;
    const bool and_mask = (ops & 0x100u) != 0;
    unsigned long long sL = 0, sW = 0, sK = 0;
    for (uint64_t j0 = 0; j0 < nrec; j0 += 256) {
        const uint64_t j = j0 + t;
        const bool valid = j < nrec, live = valid && ok;
        int64_t L = 0, start = 0, len = 0;
        bool c0 = false, c1 = false, c2 = false, c3 = false, c4 = false;
        if (live) {   // (a failed chunk's descriptors are not defined: its rows are 0)
            const uint4 d = *(const uint4 *)(recs + 4 * (rb + j));
            L = d.y > d.x ? (int64_t)(d.y - d.x - 1) : 0;
            const int64_t b0 = min(tr.head, L), e0 = max(b0, L - tr.tail);
            const uint32_t vl = rsc[rb + j], vw = rsc[tot + rb + j], va = rsc[2 * tot + rb + j], vt = rsc[3 * tot + rb + j];
            const int64_t lead = (ops & 1u) ? (vl != kNone ? (int64_t)vl : e0) : b0;
            const int64_t trail = (ops & 2u) ? (vt ? (int64_t)vt : b0) : e0;
            const int64_t win = (ops & 4u) && vw != kNone ? (int64_t)vw : e0;
            const int64_t adapt = (ops & 8u) && va != kNone ? (int64_t)va : e0;
            const int64_t b = max(b0, lead), e = min(trail, min(win, adapt));
            len = max(e - b, (int64_t)0);
            start = len > 0 ? b : 0;
            c0 = b0 > 0 || e0 < L;
            c1 = lead > b0;
            c2 = trail < e0;
            c3 = win < e0;
            c4 = adapt < e0;
        }
        const bool keep = live && len >= tr.min_len;
        const bool trimmed = live && !(start == 0 && len == L);
        if (valid && trim) *(uint2 *)(trim + 2 * (rec0 + rb + j)) = make_uint2((uint32_t)start, (uint32_t)len);
        sL += (unsigned long long)L;
        sW += (unsigned long long)len;
        sK += keep ? (unsigned long long)len : 0ull;
        const unsigned long long bk = __ballot(keep), bt = __ballot(trimmed);
        const unsigned long long q0 = __ballot(c0), q1 = __ballot(c1), q2 = __ballot(c2), q3 = __ballot(c3), q4 = __ballot(c4);
        if (words) {
            // the wave's records are bits [R, R + 64) of the mask: at most three words, one lane each
            const unsigned long long bits = and_mask ? __ballot(valid && !keep) : bk;
            const uint64_t R = rec0 + rb + j0 + (t - lane);
            const uint32_t sh = (uint32_t)(R & 31u);
            if (lane < 3) {
                const uint32_t part = lane == 0 ? (uint32_t)(bits << sh)
                                    : lane == 1 ? (uint32_t)(bits >> (32 - sh))
                                    : sh ? (uint32_t)(bits >> (64 - sh)) : 0u;
                if (part) {   // (a set bit is a record of this wave: its word lies below the mask's cap)
                    if (and_mask) atomicAnd(words + (R >> 5) + lane, ~part);
                    else atomicOr(words + (R >> 5) + lane, part);
                }
            }
        }
        if (lane == 0) {
            if (bk) atomicAdd(&cnt[0], (uint32_t)__popcll(bk));
            if (bt) atomicAdd(&cnt[1], (uint32_t)__popcll(bt));
            if (q0) atomicAdd(&cnt[2], (uint32_t)__popcll(q0));
            if (q1) atomicAdd(&cnt[3], (uint32_t)__popcll(q1));
            if (q2) atomicAdd(&cnt[4], (uint32_t)__popcll(q2));
            if (q3) atomicAdd(&cnt[5], (uint32_t)__popcll(q3));
            if (q4) atomicAdd(&cnt[6], (uint32_t)__popcll(q4));
        }
    }
    sL = wave_sum64(sL);
    sW = wave_sum64(sW);
    sK = wave_sum64(sK);
    if (lane == 0) {
        if (sL) atomicAdd(&sums[0], sL);
        if (sW) atomicAdd(&sums[1], sW);
        if (sK) atomicAdd(&sums[2], sK);
    }
    __syncthreads();
    if (t == 0) {
        *(volatile int64_t *)(host_chunk_kept + k) = (int64_t)cnt[0];
        if (nrec) atomicAdd(acc + 0, (unsigned long long)nrec);
    }
    if (t < 7 && cnt[t]) atomicAdd(acc + 1 + t, (unsigned long long)cnt[t]);
    if (t < 3 && sums[t]) atomicAdd(acc + 8 + t, sums[t]);
}

// The run's accumulators (kRtAcc values, the layout of a ppg_read_trim_result) into pinned host memory by
// kernel stores.
extern "C" __global__ __launch_bounds__(64) void ppg_rt_totals(const unsigned long long *__restrict__ acc,
                                                                int64_t *host_result) {
    if (threadIdx.x < (uint32_t)kRtAcc) *(volatile int64_t *)(host_result + threadIdx.x) = (int64_t)acc[threadIdx.x];
}

// dst row i = trim row recno[i] - rec0, i < n: the windows of a batch's selected records, in their order
extern "C" __global__ __launch_bounds__(256) void ppg_rt_gather(const uint2 *__restrict__ trim,
                                                                 const int64_t *__restrict__ recno, int64_t rec0,
                                                                 uint64_t n, uint2 *__restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = trim[recno[i] - rec0];
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp, ppg_cursor.cpp); v: the batch (ppg_device.h)
// ------------------------------------------------------------------------------------------
// total: the batch's padded bases (ppg_seq_scan); rsc: four planes of tot words, initialised by the caller
// (three of all ones, then one of zeros)
hipError_t ppg_launch_rt_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, const int64_t *seq_off,
                                 const uint32_t *seq_len, uint64_t total, const PpgReadTrim *tr, uint32_t *rsc,
                                 uint64_t tot) {
    const uint64_t units = total / 32;
    if (v.n <= 0 || units == 0 || !(tr->ops & 15)) return hipSuccess;   // (no cut looks at a byte)
    const dim3 grid((unsigned)((units + 255) / 256));
    if (tr->ops & 8)
        hipLaunchKernelGGL(ppg_rt_measure<true>, grid, dim3(256), 0, s, v.out, v.jobs, v.offs, v.oref, v.info, v.base, v.recs,
                           cbase, seq_off, seq_len, units, *tr, rsc, tot, v.n);
    else
        hipLaunchKernelGGL(ppg_rt_measure<false>, grid, dim3(256), 0, s, v.out, v.jobs, v.offs, v.oref, v.info, v.base, v.recs,
                           cbase, seq_off, seq_len, units, *tr, rsc, tot, v.n);
    return hipGetLastError();
}

// trim: row 0 of the plane (the batch's rows start at rec0); words: the mask's word 0
hipError_t ppg_launch_rt_decide(hipStream_t s, const PpgBatchView &v, const uint32_t *rsc, uint64_t tot,
                                const PpgReadTrim *tr, uint32_t *words, uint64_t rec0, uint32_t *trim, uint64_t *acc,
                                int64_t *host_chunk_kept) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_rt_decide, dim3(v.n), dim3(256), 0, s, v.res, v.info, v.base, v.recs, rsc, tot, *tr, words, rec0,
                       trim, (unsigned long long *)acc, host_chunk_kept, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_rt_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result) {
    hipLaunchKernelGGL(ppg_rt_totals, dim3(1), dim3(64), 0, s, (const unsigned long long *)acc, host_result);
    return hipGetLastError();
}

hipError_t ppg_launch_rt_gather(hipStream_t s, const uint32_t *trim, const int64_t *recno, int64_t rec0, uint64_t n,
                                uint32_t *dst) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_rt_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint2 *)trim, recno, rec0, n,
                       (uint2 *)dst);
    return hipGetLastError();
}
