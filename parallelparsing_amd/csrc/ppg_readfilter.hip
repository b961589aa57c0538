// ppg_readfilter.hip — read filters over a resident batch (include/ppgpu.h "read filters"): per record
// the Sequence length, its bytes that are not A C G T, the Quality length, its sum and its bytes below
// a threshold; from those the quality-control criteria every FASTQ pipeline starts with (length, N
// content, mean quality, fraction of low-quality bases) as one pass bit per record, plus the census of
// the Quality bytes.  The reference has no such filter: its consumer would walk FastqRecord.Sequence
// and FastqRecord.Quality on the host; here the numbers are made where the text already is and only
// the records that pass need to leave the device (record selection, ppg_seqselect.hip).
//
//   layout   as the packed reads and the queries: P_j = 32 * ceil(L_j / 32) per record, per-chunk sums,
//            their scan, seq_off / seq_len per record (ppg_seq_totals, ppg_seq_scan, ppg_seq_offsets,
//            unchanged; made once per batch for the query, the filter and the trim: shard_layout).
//   measure  one thread per 32-base unit (ppg_rf_measure), chunk and record by unit_lookup
//            (ppg_seqload.h).  The unit reads its <= 32 bytes of S_j and the bytes of Q_j at the same
//            indices.  Consecutive lanes belong to the same or to successive records, so the per-lane
//            (other, low, qsum) are summed within the wave segmented by record (a Hillis-Steele scan
//            whose step adds the lane `o` below only when it has the same record), and the last lane
//            of each segment adds the segment's sums into the record's scratch: two 64-bit atomics per
//            record and wave (other and low share one word), not two per unit.  Records longer than
//            2,048 bases span waves, longer than 8,192 blocks: the scratch adds are what joins them.
//            The Quality bytes also go to a 256-bin histogram in LDS (see "histogram" below), flushed
//            with one 64-bit atomic per block and non-empty bin.
//   decide   a block per chunk, a thread per record (ppg_rf_decide).  The unit map leaves Quality bytes
//            uncovered: those at index >= P_j, which is every Quality byte of a record with L_j = 0.
//            The record's thread reads them bytewise here.  Then the criteria in signed 64-bit integers,
//            the 24-byte metrics row, the mask words from the wave's ballot (a wave's 64 records touch
//            at most three words; records of other chunks and batches share them, so the words are
//            changed by atomicOr / atomicAnd of this wave's bits alone), the chunk's passes to pinned
//            host memory and the totals into the run's accumulators.
//   totals   ppg_rf_totals stores the accumulators, laid out as a ppg_read_filter_result, to pinned host
//            memory by kernel stores (as ppg_seq_query_totals: no DMA engine).
//
// histogram: kRfHistRuns (the default) counts, per lane, runs of equal consecutive Quality bytes in a
// register and touches LDS once per run; kRfHistBytes adds every byte to LDS on its own.  On text
// whose Quality is mostly one value the first issues a fraction of the same-address LDS adds, which
// serialise over the 64 lanes; tools/readfilter_probe.py times both.
//
// Bytes moved per 150 bp record (P = 160, five units), derived from the formats, not measured: 150 B of
// Sequence and 150 B of Quality, 16 B of descriptor x 2 layout passes + 12 B of seq_off / seq_len
// written and read back (56 B), 16 B of descriptor in the decide pass, 16 B of scratch zeroed, added to
// and read (24-48 B), 24 B of metrics row when asked for: ~420-440 B, twice the query's ~210 B.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_seqload.h"

// One thread per 32-base unit of the batch.  seq_off / seq_len / recs / rsc point at the batch's first
// record; cbase, seq_off are batch-relative (carry 0).  Record j of the batch gets rsc[2 j] += other |
// low << 32 and rsc[2 j + 1] += qsum over the indices [0, P_j) of S_j and Q_j; acc[9 + v] += Quality
// bytes of value v among them.  thr = qual_base + low_q (0 .. 256).
template <int HIST>
__global__ __launch_bounds__(256) void ppg_rf_measure(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const uint8_t *__restrict__ offs,
    const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info, const uint64_t *__restrict__ base,
    const uint32_t *__restrict__ recs, const uint64_t *__restrict__ cbase, const int64_t *__restrict__ seq_off,
    const uint32_t *__restrict__ seq_len, uint64_t units, uint32_t thr, unsigned long long *rsc,
    unsigned long long *acc, int nchunks) {
    __shared__ uint32_t hist[256];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    hist[t] = 0;
    __syncthreads();

    unsigned long long jkey = ~0ull;   // the unit's record; lanes past the last unit share one key and add nothing
    unsigned long long ol = 0, qs = 0;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + t;
    if (u < units) {
        const uint64_t rel = 32 * u;
        int k;
        uint64_t j;
        unit_lookup(cbase, base, info, seq_off, nchunks, rel, 0, k, j);
        jkey = j;
        const uint32_t i0 = (uint32_t)((int64_t)rel - seq_off[j]);   // the unit's first index within the record
        const uint32_t L = seq_len[j];
        const uint32_t n1 = recs[4 * j], n3 = recs[4 * j + 2], n4 = recs[4 * j + 3];
        const uint32_t Lq = n4 > n3 ? n4 - n3 - 1 : 0u;
        const uint8_t *off = offs + oref[k].start, *body = out + jobs[k].out_off;
        const uint64_t olen = oref[k].len;
        const uint32_t cnt = L > i0 ? min(L - i0, 32u) : 0u;
        const uint32_t qcnt = Lq > i0 ? min(Lq - i0, 32u) : 0u;
        uint32_t x[8];
        load_raw32(off, olen, body, (uint64_t)n1 + 1 + i0, cnt, x);
        uint32_t acgt = 0;
#pragma unroll
        for (int i = 0; i < 32; i++) acgt += is_acgt((x[i >> 2] >> (8 * (i & 3))) & 255u);   // (bytes past cnt are 0)
        load_raw32(off, olen, body, (uint64_t)n3 + 1 + i0, qcnt, x);
        uint32_t low = 0, sum = 0, prev = 0, run = 0;
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 255u;
            const bool in = (uint32_t)i < qcnt;
            sum += c;                                                // (bytes past qcnt are 0)
            low += in && c < thr;
            if (HIST == kRfHistBytes) {
                if (in) atomicAdd(&hist[c], 1u);
            } else if (in) {
                if (c != prev && run) {
                    atomicAdd(&hist[prev], run);
                    run = 0;
                }
                prev = c;
                run++;
            }
        }
        if (HIST != kRfHistBytes && run) atomicAdd(&hist[prev], run);
        ol = (unsigned long long)(cnt - acgt) | (unsigned long long)low << 32;
        qs = sum;
    }
    // sums over the lanes of one record: after the step `o` a lane holds its segment's lanes [lane - 2o + 1, lane]
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long jo = __shfl_up(jkey, o, 64), a = __shfl_up(ol, o, 64), b = __shfl_up(qs, o, 64);
        if (lane >= (uint32_t)o && jo == jkey) {
            ol += a;
            qs += b;
        }
    }
    const unsigned long long jn = __shfl_down(jkey, 1, 64);
    if (jkey != ~0ull && (lane == 63u || jn != jkey)) {   // the segment's last lane
        if (ol) atomicAdd(rsc + 2 * jkey, ol);
        if (qs) atomicAdd(rsc + 2 * jkey + 1, qs);
    }
    __syncthreads();
    if (hist[t]) atomicAdd(acc + 9 + t, (unsigned long long)hist[t]);
}

// A block per chunk k of the batch, a thread per record.  Finishes the Quality bytes the units do not
// cover, evaluates the criteria and writes: the metrics row of shard record rec0 + j (metrics != null),
// the record's bit rec0 + j of words (words != null; and_mask: the bit is cleared when the record
// fails and left alone otherwise, else the words were zeroed and the bit is set when it passes),
// host_chunk_passed[k] (pinned) and the run's accumulators acc[0] records, acc[1] passed, acc[2..5]
// failed per criterion, acc[6] bases, acc[7] other, acc[8] Quality bytes, acc[9 + v] Quality bytes of value v.
extern "C" __global__ __launch_bounds__(256) void ppg_rf_decide(
    const uint8_t *__restrict__ out, const PpgInflateJob *__restrict__ jobs, const PpgInflateResult *__restrict__ ires,
    const uint8_t *__restrict__ offs, const PpgOffsetRef *__restrict__ oref, const PpgParseInfo *__restrict__ info,
    const uint64_t *__restrict__ base, const uint32_t *__restrict__ recs, const unsigned long long *__restrict__ rsc,
    PpgReadFilter f, uint32_t *words, uint64_t rec0, uint8_t *metrics, unsigned long long *acc,
    int64_t *host_chunk_passed, int nchunks) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t cnt[5];                  // passed, failed[4]
    __shared__ unsigned long long sums[3];       // bases, other, Quality bytes
    const int k = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (k >= nchunks) return;
    hist[t] = 0;
    if (t < 5) cnt[t] = 0;
    if (t < 3) sums[t] = 0;
    __syncthreads();
    const bool ok = ires[k].status == 0;
    const uint64_t nrec = info[k].records, rb = base[k];
    const uint8_t *off = offs + oref[k].start, *body = out + jobs[k].out_off;
    const uint64_t olen = oref[k].len;
    const int64_t thr = f.qual_base + f.low_q;
    const bool and_mask = (f.criteria & 0x100) != 0;
    unsigned long long sL = 0, sO = 0, sQ = 0;
    for (uint64_t j0 = 0; j0 < nrec; j0 += 256) {
        const uint64_t j = j0 + t;
        const bool valid = j < nrec;
        uint32_t L = 0, Lq = 0, other = 0, low = 0;
        unsigned long long qsum = 0;
        if (valid && ok) {   // (a failed chunk's descriptors are not defined: its rows are 0)
            const uint4 d = *(const uint4 *)(recs + 4 * (rb + j));
            L = d.y > d.x ? d.y - d.x - 1 : 0u;
            Lq = d.w > d.z ? d.w - d.z - 1 : 0u;
            const unsigned long long w = rsc[2 * (rb + j)];
            other = (uint32_t)w;
            low = (uint32_t)(w >> 32);
            qsum = rsc[2 * (rb + j) + 1];
            // the Quality bytes no unit owns: index >= P_j (all of them when L_j = 0)
            const uint64_t P = ((uint64_t)L + 31) & ~(uint64_t)31;
            for (uint64_t i = P; i < Lq; i++) {
                const uint64_t p = (uint64_t)d.z + 1 + i;
                const uint32_t c = p < olen ? off[p] : body[p - olen];
                qsum += c;
                low += (int64_t)c < thr;
                atomicAdd(&hist[c], 1u);
            }
        }
        const int64_t sl = (int64_t)L, sq = (int64_t)Lq;
        const bool c_len = f.min_len <= sl && (f.max_len < 0 || sl <= f.max_len);
        const bool c_oth = (int64_t)other <= f.max_other;
        const bool c_mean = 1000 * ((int64_t)qsum - f.qual_base * sq) >= f.min_mean_milli * sq;
        const bool c_low = 1000 * (int64_t)low <= f.max_low_milli * sq;
        const bool live = valid && ok;
        const bool f0 = live && (f.criteria & 1) && !c_len, f1 = live && (f.criteria & 2) && !c_oth;
        const bool f2 = live && (f.criteria & 4) && !c_mean, f3 = live && (f.criteria & 8) && !c_low;
        const bool pass = live && !(f0 || f1 || f2 || f3);
        if (valid && metrics) {
            uint8_t *row = metrics + 24 * (rec0 + rb + j);
            *(uint2 *)row = make_uint2(L, other);
            *(uint2 *)(row + 8) = make_uint2(Lq, low);
            *(unsigned long long *)(row + 16) = qsum;
        }
        sL += L;
        sO += other;
        sQ += Lq;
        const unsigned long long bp = __ballot(pass);
        const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1), b2 = __ballot(f2), b3 = __ballot(f3);
        if (words) {
            // the wave's records are bits [R, R + 64) of the mask: at most three words, one lane each
            const unsigned long long bits = and_mask ? __ballot(valid && !pass) : bp;
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
            if (bp) atomicAdd(&cnt[0], (uint32_t)__popcll(bp));
            if (b0) atomicAdd(&cnt[1], (uint32_t)__popcll(b0));
            if (b1) atomicAdd(&cnt[2], (uint32_t)__popcll(b1));
            if (b2) atomicAdd(&cnt[3], (uint32_t)__popcll(b2));
            if (b3) atomicAdd(&cnt[4], (uint32_t)__popcll(b3));
        }
    }
    sL = wave_sum64(sL);
    sO = wave_sum64(sO);
    sQ = wave_sum64(sQ);
    if (lane == 0) {
        if (sL) atomicAdd(&sums[0], sL);
        if (sO) atomicAdd(&sums[1], sO);
        if (sQ) atomicAdd(&sums[2], sQ);
    }
    __syncthreads();
    if (t == 0) {
        *(volatile int64_t *)(host_chunk_passed + k) = (int64_t)cnt[0];
        if (nrec) atomicAdd(acc + 0, (unsigned long long)nrec);
    }
    if (t < 5 && cnt[t]) atomicAdd(acc + 1 + t, (unsigned long long)cnt[t]);
    if (t < 3 && sums[t]) atomicAdd(acc + 6 + t, sums[t]);
    if (hist[t]) atomicAdd(acc + 9 + t, (unsigned long long)hist[t]);
}

// The run's accumulators (kRfAcc values, the layout of a ppg_read_filter_result) into pinned host memory
// by kernel stores.
extern "C" __global__ __launch_bounds__(256) void ppg_rf_totals(const unsigned long long *__restrict__ acc,
                                                                 int64_t *host_result) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)kRfAcc; i += 256) *(volatile int64_t *)(host_result + i) = (int64_t)acc[i];
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); v: the batch (ppg_device.h)
// ------------------------------------------------------------------------------------------
// total: the batch's padded bases (ppg_seq_scan)
hipError_t ppg_launch_rf_measure(hipStream_t s, const PpgBatchView &v, const uint64_t *cbase, const int64_t *seq_off,
                                 const uint32_t *seq_len, uint64_t total, uint32_t thr, uint64_t *rsc, uint64_t *acc,
                                 int hist) {
    const uint64_t units = total / 32;
    if (v.n <= 0 || units == 0) return hipSuccess;
    const dim3 grid((unsigned)((units + 255) / 256));
    if (hist == kRfHistBytes)
        hipLaunchKernelGGL(ppg_rf_measure<kRfHistBytes>, grid, dim3(256), 0, s, v.out, v.jobs, v.offs, v.oref, v.info, v.base,
                           v.recs, cbase, seq_off, seq_len, units, thr, (unsigned long long *)rsc, (unsigned long long *)acc,
                           v.n);
    else
        hipLaunchKernelGGL(ppg_rf_measure<kRfHistRuns>, grid, dim3(256), 0, s, v.out, v.jobs, v.offs, v.oref, v.info, v.base,
                           v.recs, cbase, seq_off, seq_len, units, thr, (unsigned long long *)rsc, (unsigned long long *)acc,
                           v.n);
    return hipGetLastError();
}

// metrics: row 0 of the plane (the batch's rows start at rec0); words: the mask's word 0
hipError_t ppg_launch_rf_decide(hipStream_t s, const PpgBatchView &v, const uint64_t *rsc, const PpgReadFilter *f,
                                uint32_t *words, uint64_t rec0, uint8_t *metrics, uint64_t *acc,
                                int64_t *host_chunk_passed) {
    if (v.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_rf_decide, dim3(v.n), dim3(256), 0, s, v.out, v.jobs, v.res, v.offs, v.oref, v.info, v.base,
                       v.recs, (const unsigned long long *)rsc, *f, words, rec0, metrics, (unsigned long long *)acc,
                       host_chunk_passed, v.n);
    return hipGetLastError();
}

hipError_t ppg_launch_rf_totals(hipStream_t s, const uint64_t *acc, int64_t *host_result) {
    hipLaunchKernelGGL(ppg_rf_totals, dim3(1), dim3(256), 0, s, (const unsigned long long *)acc, host_result);
    return hipGetLastError();
}
