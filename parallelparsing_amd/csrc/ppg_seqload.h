// ppg_seqload.h — device loads of up to 32 bytes of raw_k = offset_k ++ body_k, shared by the kernels that
// read record slices of a resident batch per 32-base unit (ppg_seqpack.hip, ppg_seqquery.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

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
