// ppg_mix.h — the 64-bit mixer the hash tables share (include/ppgpu.h "read dedup" defines it): the read dedup
// (ppg_readdedup.hip) makes its fingerprints with it, the k-mer counter (ppg_kmercount.hip) the home row of a key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr unsigned long long kDdMul = 0xD6E8FEB86659FD93ull;

__device__ __forceinline__ unsigned long long dd_mix(unsigned long long x) {
    x ^= x >> 32;
    x *= kDdMul;
    x ^= x >> 32;
    x *= kDdMul;
    x ^= x >> 32;
    return x;
}
