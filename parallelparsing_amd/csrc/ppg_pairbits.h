// ppg_pairbits.h — the bit operations on packed reads (2 bits per base, 32 bases per 64-bit word) that the
// pair stages share: ppg_pairoverlap.hip and ppg_pairmerge.hip both look at read 1 against the reverse
// complement of read 2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint64_t kPoEven = 0x5555555555555555ull;

// bit b of m at bit 2 b
__device__ __forceinline__ uint64_t po_spread(uint32_t m) {
    uint64_t x = m;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    return (x | (x << 1)) & kPoEven;
}

// the 32 bases of w in reverse order: all 64 bits reversed, then the two bits of every base swapped back
__device__ __forceinline__ uint64_t po_reverse(uint64_t w) {
    const uint64_t r = __brevll(w);
    return ((r >> 1) & kPoEven) | ((r & kPoEven) << 1);
}

// lo >> s with hi's low bits above it, s = 0 .. 62
__device__ __forceinline__ uint64_t po_funnel(uint64_t lo, uint64_t hi, uint32_t s) {
    return s ? (lo >> s) | (hi << (64u - s)) : lo;
}
