// ppg_seqload.h — device helpers shared by the record-stage kernels: the lookup of a 32-base unit's chunk
// and record and the loads of up to 32 bytes of raw_k = offset_k ++ body_k, for the kernels that read record
// slices of a resident batch per unit (ppg_seqpack.hip, ppg_seqquery.hip, ppg_readfilter.hip,
// ppg_readtrim.hip, ppg_readprofile.hip, ppg_readdedup.hip); is_acgt (ppg_seqpack.hip, ppg_readfilter.hip);
// wave_sum64 (ppg_readfilter.hip, ppg_readtrim.hip, ppg_readprofile.hip, ppg_readdedup.hip, ppg_seqselect.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ppg_device.h"

namespace {

// 1 for 'A' 'C' 'G' 'T': the byte is 0x40..0x5F and its low five bits are 1, 3, 7 or 20
__device__ __forceinline__ uint32_t is_acgt(uint32_t c) {
    return (c >> 5) == 2u ? (0x0010008Au >> (c & 31u)) & 1u : 0u;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // lane 0 holds the sum
}

// The chunk k and the record j (counted from the batch's first) of the unit at batch-relative base
// position rel, by two binary searches: the last k with cbase[k] <= rel (chunks without bases share their
// successor's base), then the last j of that chunk with seq_off[j] <= carry + rel (records without bases
// likewise).  seq_off points at the batch's first record and was laid out from `carry`.
__device__ __forceinline__ void unit_lookup(const uint64_t *__restrict__ cbase, const uint64_t *__restrict__ base,
                                            const PpgParseInfo *__restrict__ info, const int64_t *__restrict__ seq_off,
                                            int nchunks, uint64_t rel, int64_t carry, int &k, uint64_t &j) {
    int lo = 0, hi = nchunks;                    // invariant: cbase[lo] <= rel < cbase[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cbase[mid] <= rel) lo = mid; else hi = mid;
    }
    k = lo;
    const int64_t b = carry + (int64_t)rel;
    uint64_t jl = base[k], jh = jl + info[k].records;   // seq_off[jl] <= b < seq_off[jh]
    while (jh - jl > 1) {
        const uint64_t mid = (jl + jh) >> 1;
        if (seq_off[mid] <= b) jl = mid; else jh = mid;
    }
    j = jl;
}

// 32 bytes at p (any alignment, readable up to p + 35 rounded down to a dword) as 8 dwords
__device__ __forceinline__ void load32(const uint8_t *p, uint32_t (&u)[8]) {
    const uint32_t *w = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
    uint32_t x[9];
#pragma unroll
    for (int k = 0; k < 9; k++) x[k] = w[k];
#pragma unroll
    for (int k = 0; k < 8; k++) u[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], sh);
}

// raw bytes [p0, p0 + cnt) of raw_k = offset_k ++ body_k, cnt <= 32, into u (bytes past cnt: 0).
// Every byte read lies inside raw_k when p0 + cnt <= |raw_k|, apart from the dword over-read of the
// aligned path, which stays inside the output buffer and its tail.
__device__ __forceinline__ void load_raw32(const uint8_t *off, uint64_t olen, const uint8_t *body, uint64_t p0,
                                           uint32_t cnt, uint32_t (&u)[8]) {
    if (cnt == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) u[k] = 0;
        return;
    }
    if (p0 >= olen) {
        load32(body + (p0 - olen), u);
    } else {   // the unit touches the offset carry: bytewise
#pragma unroll
        for (int k = 0; k < 8; k++) u[k] = 0;
        for (uint32_t i = 0; i < cnt; i++) {
            const uint64_t p = p0 + i;
            const uint32_t c = p < olen ? off[p] : body[p - olen];
            u[i >> 2] |= c << (8 * (i & 3));
        }
    }
    // zero the bytes at and past cnt
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int32_t keep = (int32_t)cnt - 4 * k;   // bytes of dword k that stay
        u[k] = keep >= 4 ? u[k] : keep <= 0 ? 0u : u[k] & (0xFFFFFFFFu >> (32 - 8 * keep));
    }
}

}  // namespace
