// ppg_kmercount.hip — k-mer counts of a packed read set (include/ppgpu.h "k-mer counts"): every valid k-mer of
// every participating record, inside its window, counted in a hash table of {key, count} rows in caller device
// memory; from the table the spectrum, the rows above a count and the counts of given keys.  The reference has
// nothing of the kind: a consumer would hash every read's text on the host.  Here the reads are packed
// (ppg_seqpack.hip: 2 bits per base and an N bit, 32 bases per 64-bit word), so a k-mer with k <= 31 is a funnel
// shift and a mask of two resident words, and only the totals and 1,024 spectrum bins leave the device.
//
//   split    one lane per 32-base unit of the set, not per record and not per start: a unit's 64-bit word and
//            the next one of the same record cover its 32 starts and their k - 1 <= 30 spill bases, two mask
//            words go with them, so a lane loads 24 B once and makes 32 keys from registers.  A lane per start
//            would load the same two words 32 times; a record per lane leaves the wave waiting for its longest
//            read.  Records start on units, so unit -> record is a table: ppg_km_records (a lane per record)
//            writes the record's number to each of its units and adds the record's totals, which a record
//            without bases needs anyway (it has no unit).  4 B per unit written and read once; no search.
//   keys     start t of the unit: LE = funnel(w0, w1, 2 t) & M, the little-endian value the planes give.  The
//            key (first base most significant) is LE with its k bases reversed, po_reverse(LE) >> (64 - 2 k);
//            the reverse complement's key is ~LE & M; canonical is the smaller.  Valid: none of the k mask bits
//            from t on is set.
//   insert   ppg_km_insert walks the 32 starts in step across the wave.  Equal keys are combined before they
//            reach memory, twice: along the read a lane keeps (key, run) and hands the run on only when the key
//            changes (a poly-X run of a unit is one insert); across the wave the lanes that hand on equal keys
//            in one step are grouped in registers as ppg_dd_insert groups fingerprints, their runs summed in
//            LDS, and the lowest lane inserts once for all.  The table is touched by device-scope atomics
//            alone: CAS ~0 -> key on the key word from the home row on, linear with wrap and bounded by `slots`,
//            then atomicAdd on the count.  No lane waits for another lane's write.
//   capacity a device counter of claimed rows (acc[kKmClaimed]; with ACCUMULATE it starts from the occupied
//            rows, ppg_km_init counts them).  One add per claim on one word would serialise an all-distinct
//            input, so a wave counts its claims in a scalar and adds them once it holds `flush_at` of them,
//            which the launcher sizes so that all waves in flight together hide at most an eighth of the table
//            from the counter.  The leaders of a wave probe in step, one row per round; a wave whose probe
//            takes 64 rounds adds what it holds at once and looks at the counter, so a table that fills up
//            anyway (a small one can within one step of all waves) is reported by the waves it holds up.  A
//            wave that sees the counter above slots / 2 (when it adds, or before a tile) starts no further
//            insert.  An undersized table so costs about what filling it costs, not a probe of `slots` rows
//            per lane.
//   passes   one read of the table each, a lane per row, grid-stride: ppg_km_stats (the spectrum's bins and the
//            totals in LDS, flushed once per block), ppg_km_maxkey (the lowest key among the rows of the
//            greatest count), ppg_km_select (compaction through an atomic cursor, one add per block and 2,048 rows) and
//            ppg_km_lookup (a lane per key, the same probe without writes).  A kernel boundary orders the
//            insert's atomics before them.
//
// Per 150 bp record at k = 21 (five units), derived from the formats, not measured: 40 B of bases, 20 B of mask,
// 12 B of seq_off / seq_len, 2 x 20 B of unit table: ~112 B streamed; 130 starts, each a CAS and an add on one
// 16-B row at random (one 64-B sector): 260 atomics and 130 sectors.  The table accesses bound the insert.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ppg_device.h"
#include "ppg_launch.h"
#include "ppg_mix.h"
#include "ppg_pairbits.h"

namespace {

constexpr unsigned long long kKmEmpty = ~0ull;
constexpr uint32_t kKmNoRec = ~0u;   // a unit of no record (the table is filled with it first)

// LDS operations of one wave complete in order: between a wave's writes and its reads of other lanes' words
// only the compiler has to keep the order
__device__ __forceinline__ void km_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long km_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned long long km_peek(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the window (s, w) of record r of length L: row r clamped as in the profile, or (0, L)
__device__ __forceinline__ void km_window(const uint2 *__restrict__ rows, int64_t r, uint32_t L, uint32_t &s, uint32_t &w) {
    s = 0;
    w = L;
    if (rows) {
        const uint2 row = rows[r];
        s = min(row.x, L);
        w = min(row.y, L - s);
    }
}

__device__ __forceinline__ bool km_bit(const uint32_t *__restrict__ words, int64_t r) {
    return !words || ((words[r >> 5] >> (uint32_t)(r & 31)) & 1u);
}

// lane `l`'s value in every lane (l the same in every lane)
__device__ __forceinline__ unsigned long long km_from(unsigned long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

}  // namespace

// accumulate == 0: every row of the table empty.  Else acc[kKmClaimed] += the occupied rows.
extern "C" __global__ __launch_bounds__(256) void ppg_km_init(unsigned long long *table, uint64_t slots, int accumulate,
                                                               unsigned long long *acc) {
    __shared__ uint32_t occ;
    if (threadIdx.x == 0) occ = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < slots; r += (uint64_t)gridDim.x * 256) {
        if (accumulate) {
            mine += table[2 * r] != kKmEmpty;
        } else {
            *(ulonglong2 *)(table + 2 * r) = make_ulonglong2(kKmEmpty, 0ull);
        }
    }
    if (!accumulate) return;
    mine = (uint32_t)km_wave_sum(mine);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&occ, mine);
    __syncthreads();
    if (threadIdx.x == 0 && occ) atomicAdd(acc + kKmClaimed, (unsigned long long)occ);
}

// A lane per record: umap[u] = the record of unit u for the record's units (below `units`), and the totals of the
// call: acc[0] records, acc[1] participating, acc[2] short_reads, acc[3] bases, acc[4] positions.
extern "C" __global__ __launch_bounds__(256) void ppg_km_records(const PpgPackedView set, const uint32_t *__restrict__ words,
                                                                  const uint2 *__restrict__ rows, uint32_t k, uint64_t units,
                                                                  uint32_t *umap, unsigned long long *acc) {
    __shared__ unsigned long long tot[5];
    const uint32_t t = threadIdx.x;
    if (t < 5) tot[t] = 0;
    __syncthreads();
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    for (int64_t r = (int64_t)blockIdx.x * 256 + t; r < set.records; r += (int64_t)gridDim.x * 256) {
        const int64_t b0 = set.seq_off[r], b1 = set.seq_off[r + 1];
        const uint64_t u0 = (uint64_t)b0 >> 5, nu = b1 > b0 ? (uint64_t)(b1 - b0) >> 5 : 0;
        for (uint64_t i = 0; i < nu && u0 + i < units; i++) umap[u0 + i] = (uint32_t)r;
        v[0]++;
        if (km_bit(words, r)) {
            const uint32_t L = (uint32_t)min((uint64_t)set.seq_len[r], 32 * nu);
            uint32_t s, w;
            km_window(rows, r, L, s, w);
            v[1]++;
            v[2] += w < k;
            v[3] += w;
            v[4] += w >= k ? w - k + 1 : 0;
        }
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        v[i] = km_wave_sum(v[i]);
        if ((t & 63u) == 0 && v[i]) atomicAdd(&tot[i], v[i]);
    }
    __syncthreads();
    if (t < 5 && tot[t]) atomicAdd(acc + t, tot[t]);
}

// A lane per 32-base unit; block b takes the tiles of 256 units b, b + grid, ...  shift = 64 - log2 slots; limit =
// slots / 2.  acc[5] += the valid positions, acc[12] += the inserts given up, acc[kKmClaimed] the claimed rows.
// Neither LDS (1 KiB) nor registers limit the waves per CU; the table's latency is what a wave waits for, and the
// default grid of eight blocks per CU keeps 32 waves per CU on it.
extern "C" __global__ __launch_bounds__(256) void ppg_km_insert(
    const PpgPackedView set, const uint32_t *__restrict__ words, const uint2 *__restrict__ rows,
    const uint32_t *__restrict__ umap, uint32_t k, int canonical, uint64_t units, unsigned long long *table, uint64_t slots,
    uint32_t shift, unsigned long long limit, uint32_t flush_at, unsigned long long *acc) {
    __shared__ uint32_t gsum[4][64];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    uint32_t *const sum = gsum[__builtin_amdgcn_readfirstlane(t >> 6)];
    const uint64_t M = (1ull << (2 * k)) - 1, KM = (1ull << k) - 1;
    const uint64_t ntiles = (units + 255) / 256;
    unsigned long long nvalid = 0;
    uint32_t pending = 0;   // the wave's claims not yet in the counter; the same in every lane
    bool dead = false;      // the counter passed the limit; the same in every lane

    for (uint64_t tile = blockIdx.x; tile < ntiles && !dead; tile += gridDim.x) {
        if (__builtin_amdgcn_readfirstlane((int)(km_peek(acc + kKmClaimed) > limit))) {
            dead = true;
            break;
        }
        const uint64_t u = tile * 256 + t;
        uint64_t w0 = 0, w1 = 0, mw = 0;
        int t0 = 0, t1 = 0;   // the unit's starts [t0, t1) that are positions
        if (u < units) {
            const uint32_t j = umap[u];
            if (j != kKmNoRec && (int64_t)j < set.records && km_bit(words, j)) {
                const int64_t b0 = set.seq_off[j], b1 = set.seq_off[j + 1];
                const int64_t i0 = 32 * (int64_t)u - b0;                 // the unit's first base within the record
                if (i0 >= 0 && 32 * (int64_t)u < b1) {
                    const uint32_t L = (uint32_t)min((int64_t)set.seq_len[j], b1 - b0);
                    uint32_t s, w;
                    km_window(rows, j, L, s, w);
                    const int64_t lo = max((int64_t)s, i0), hi = min(i0 + 32, (int64_t)s + w - k + 1);
                    if (hi > lo) {
                        t0 = (int)(lo - i0);
                        t1 = (int)(hi - i0);
                        w0 = ((const uint64_t *)set.bases)[u];
                        mw = set.mask[u];
                        if (i0 + 32 < (int64_t)L) {   // the record's next unit: u + 1 < units
                            w1 = ((const uint64_t *)set.bases)[u + 1];
                            mw |= (uint64_t)set.mask[u + 1] << 32;
                        }
                    }
                }
            }
        }
        unsigned long long run_key = kKmEmpty;
        uint32_t run = 0;
        for (int st = 0; st <= 32; st++) {   // (step 32 hands on what is left)
            unsigned long long key = kKmEmpty;
            if (st >= t0 && st < t1 && ((mw >> st) & KM) == 0) {
                const uint64_t le = po_funnel(w0, w1, 2u * (uint32_t)st) & M;
                key = po_reverse(le) >> (64u - 2u * k);
                if (canonical) key = min(key, (unsigned long long)(~le & M));
                nvalid++;
            }
            const bool hand = run != 0 && key != run_key;   // the run ends here
            const unsigned long long fk = run_key;
            const uint32_t fc = run;
            if (key != run_key) {
                run_key = key;
                run = 0;
            }
            if (key != kKmEmpty) run++;
            unsigned long long rem = __ballot(hand);
            if (!rem) continue;
            // the wave's groups of equal keys: as many steps as it hands on distinct ones, registers alone
            uint32_t leader = lane;
            while (rem) {
                const int l = __ffsll((long long)rem) - 1;
                const bool same = hand && fk == km_from(fk, l);
                if (same) leader = (uint32_t)l;
                rem &= ~__ballot(same);
            }
            sum[lane] = 0;
            km_wave_sync();
            if (hand) atomicAdd(&sum[leader], fc);
            km_wave_sync();
            // the leaders probe in step, one row per round, so the wave can report while some of them are still
            // on their way: every 64 rounds (a probe that long means a table fuller than it may be) it adds its
            // claims to the counter and looks at it, and so does every other wave that is held up
            bool active = hand && leader == lane, claimed = false;
            const unsigned long long total = sum[lane];
            uint64_t slot = dd_mix(fk) >> shift;
            km_wave_sync();   // (sum[] has been read before the next step clears it)
            uint64_t round = 0;
            while (__ballot(active)) {
                if (active) {
                    unsigned long long *row = table + 2 * slot;
                    const unsigned long long old = atomicCAS(row, kKmEmpty, fk);
                    if (old == kKmEmpty || old == fk) {
                        atomicAdd(row + 1, total);
                        claimed = old == kKmEmpty;
                        active = false;
                    }
                    slot = (slot + 1) & (slots - 1);
                }
                round++;
                if ((round & 63u) == 0 || round == slots) {
                    pending += (uint32_t)__popcll(__ballot(claimed));
                    claimed = false;
                    unsigned long long before = 0;
                    if (lane == 0) before = atomicAdd(acc + kKmClaimed, (unsigned long long)pending);
                    dead = km_from(before, 0) + pending > limit || (round == slots && __ballot(active) != 0);
                    pending = 0;
                    if (dead) break;   // (the lanes still active have found no row)
                }
            }
            const unsigned long long ob = __ballot(active);
            pending += (uint32_t)__popcll(__ballot(claimed));
            if (ob && lane == 0) atomicAdd(acc + 12, (unsigned long long)__popcll(ob));
            if (pending >= flush_at) {
                unsigned long long before = 0;
                if (lane == 0) before = atomicAdd(acc + kKmClaimed, (unsigned long long)pending);
                dead = dead || km_from(before, 0) + pending > limit;
                pending = 0;
            }
            if (dead) break;
        }
    }
    if (pending && lane == 0) atomicAdd(acc + kKmClaimed, (unsigned long long)pending);
    if (dead && lane == 0) atomicAdd(acc + 12, 1ull);   // what this wave left out is not counted: the call fails
    nvalid = km_wave_sum(nvalid);
    if (lane == 0 && nvalid) atomicAdd(acc + 5, nvalid);
}

// A lane per row, after the insert has completed: acc[7] distinct, acc[8] singletons, acc[9] = the greatest count,
// acc[11] the sum of all counts, acc[kKmSpecAt + c] the spectrum.
extern "C" __global__ __launch_bounds__(256) void ppg_km_stats(const unsigned long long *__restrict__ table, uint64_t slots,
                                                                unsigned long long *acc) {
    __shared__ uint32_t bins[kKmSpectrum];
    __shared__ unsigned long long top, total;
    const uint32_t t = threadIdx.x;
    for (uint32_t e = t; e < (uint32_t)kKmSpectrum; e += 256) bins[e] = 0;
    if (t == 0) top = total = 0;
    __syncthreads();
    unsigned long long best = 0, sumc = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + t; r < slots; r += (uint64_t)gridDim.x * 256) {
        const ulonglong2 row = *(const ulonglong2 *)(table + 2 * r);
        if (row.x != kKmEmpty) {
            atomicAdd(&bins[min(row.y, (unsigned long long)(kKmSpectrum - 1))], 1u);
            best = max(best, row.y);
            sumc += row.y;
        }
    }
    sumc = km_wave_sum(sumc);
    if ((t & 63u) == 0 && sumc) atomicAdd(&total, sumc);
    if (best) atomicMax(&top, best);
    __syncthreads();
    uint32_t rows_here = 0;
    for (uint32_t e = t; e < (uint32_t)kKmSpectrum; e += 256) {
        if (bins[e]) atomicAdd(acc + kKmSpecAt + e, (unsigned long long)bins[e]);
        rows_here += bins[e];
    }
    rows_here = (uint32_t)km_wave_sum(rows_here);
    if ((t & 63u) == 0 && rows_here) atomicAdd(acc + 7, (unsigned long long)rows_here);
    if (t == 0) {
        if (bins[1]) atomicAdd(acc + 8, (unsigned long long)bins[1]);
        if (total) atomicAdd(acc + 11, total);
        if (top) atomicMax(acc + 9, top);
    }
}

// ... and after ppg_km_stats has completed: acc[10] (all ones before) = the lowest key among the rows whose count
// is acc[9].
extern "C" __global__ __launch_bounds__(256) void ppg_km_maxkey(const unsigned long long *__restrict__ table, uint64_t slots,
                                                                 unsigned long long *acc) {
    const unsigned long long top = acc[9];
    if (top == 0) return;
    unsigned long long best = kKmEmpty;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < slots; r += (uint64_t)gridDim.x * 256) {
        const ulonglong2 row = *(const ulonglong2 *)(table + 2 * r);
        if (row.x != kKmEmpty && row.y == top) best = min(best, row.x);
    }
    if (best != kKmEmpty) atomicMin(acc + 10, best);
}

// The rows with count >= min_count go to out[cursor++] while below out_cap; *cursor counts all.  A block takes
// kKmSelRows rows per round, eight per lane, kept in registers; the waves' ballots give each its share, the waves
// add theirs in LDS and the block adds once to the cursor: one add on that word per 2,048 rows.  (One per wave, a
// returning add on one word for nearly every 64 rows, took 46.7 ms for 11 M of 268 M rows where the table's read
// takes 1.5 ms: tools/kmercount_probe.py.)  Every lane of a block takes every round, so the ballots are whole.
constexpr int kKmSelPer = 8, kKmSelRows = 256 * kKmSelPer;
extern "C" __global__ __launch_bounds__(256) void ppg_km_select(const unsigned long long *__restrict__ table, uint64_t slots,
                                                                 unsigned long long min_count, unsigned long long *out,
                                                                 uint64_t out_cap, unsigned long long *cursor) {
    __shared__ unsigned long long block_base;
    __shared__ uint32_t block_count;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint64_t r0 = (uint64_t)blockIdx.x * kKmSelRows; r0 < slots; r0 += (uint64_t)gridDim.x * kKmSelRows) {
        if (t == 0) block_count = 0;
        __syncthreads();
        ulonglong2 row[kKmSelPer];
        unsigned long long bal[kKmSelPer];
        uint32_t wave_count = 0;
#pragma unroll
        for (int i = 0; i < kKmSelPer; i++) {
            const uint64_t r = r0 + 256ull * i + t;
            row[i] = make_ulonglong2(kKmEmpty, 0ull);
            if (r < slots) row[i] = *(const ulonglong2 *)(table + 2 * r);
            bal[i] = __ballot(row[i].x != kKmEmpty && row[i].y >= min_count);
            wave_count += (uint32_t)__popcll(bal[i]);
        }
        uint32_t wave_base = 0;
        if (lane == 0 && wave_count) wave_base = atomicAdd(&block_count, wave_count);
        wave_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_base);
        __syncthreads();
        if (t == 0 && block_count) block_base = atomicAdd(cursor, (unsigned long long)block_count);
        __syncthreads();
        if (wave_count) {
            uint64_t at = block_base + wave_base;
#pragma unroll
            for (int i = 0; i < kKmSelPer; i++) {
                const uint64_t mine = at + (uint64_t)__popcll(bal[i] & below);
                if (((bal[i] >> lane) & 1ull) && mine < out_cap) *(ulonglong2 *)(out + 2 * mine) = row[i];
                at += (uint64_t)__popcll(bal[i]);
            }
        }
        __syncthreads();   // (block_count and block_base are read before the next round resets them)
    }
}

// A lane per key: counts[i] = the count of keys[i]'s row, 0 when the probe meets an empty row first (or all slots).
extern "C" __global__ __launch_bounds__(256) void ppg_km_lookup(const unsigned long long *__restrict__ table, uint64_t slots,
                                                                 uint32_t shift, const unsigned long long *__restrict__ keys,
                                                                 int64_t nkeys, int64_t *counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nkeys) return;
    const unsigned long long key = keys[i];
    int64_t c = 0;
    if (key != kKmEmpty) {
        uint64_t slot = dd_mix(key) >> shift;
        for (uint64_t n = 0; n < slots; n++) {
            const ulonglong2 row = *(const ulonglong2 *)(table + 2 * slot);
            if (row.x == key) c = (int64_t)row.y;
            if (row.x == key || row.x == kKmEmpty) break;
            slot = (slot + 1) & (slots - 1);
        }
    }
    counts[i] = c;
}

// ------------------------------------------------------------------------------------------
// launchers (ppg_stages.cpp); table: slots rows of {key, count}, slots a power of two; acc: kKmAccAll values
// ------------------------------------------------------------------------------------------
static unsigned km_row_blocks(uint64_t slots) { return (unsigned)std::min<uint64_t>((slots + 255) / 256, 4096); }

static uint32_t km_shift(uint64_t slots) {
    uint32_t lg = 0;
    while ((1ull << lg) < slots) lg++;
    return 64u - lg;
}

hipError_t ppg_launch_km_init(hipStream_t s, uint64_t *table, uint64_t slots, int accumulate, uint64_t *acc) {
    hipLaunchKernelGGL(ppg_km_init, dim3(km_row_blocks(slots)), dim3(256), 0, s, (unsigned long long *)table, slots, accumulate,
                       (unsigned long long *)acc);
    return hipGetLastError();
}

hipError_t ppg_launch_km_records(hipStream_t s, const PpgPackedView &set, const uint32_t *words, const uint32_t *rows,
                                 const PpgKmerCount *kc, uint64_t units, uint32_t *umap, uint64_t *acc) {
    if (set.records <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>((set.records + 255) / 256, 4096);
    hipLaunchKernelGGL(ppg_km_records, dim3(blocks), dim3(256), 0, s, set, words, (const uint2 *)rows, (uint32_t)kc->k, units,
                       umap, (unsigned long long *)acc);
    return hipGetLastError();
}

// blocks: the grid (<= 0: the default, eight blocks per CU), cut to the tiles of 256 units.  flush_at: a wave adds
// its claims to the counter once it holds slots / (8 x the grid's waves) of them (at least one), so all waves
// together hide at most an eighth of the table.
hipError_t ppg_launch_km_insert(hipStream_t s, const PpgPackedView &set, const uint32_t *words, const uint32_t *rows,
                                const uint32_t *umap, const PpgKmerCount *kc, uint64_t units, uint64_t *table, uint64_t slots,
                                uint64_t *acc, int blocks, int cus) {
    if (units == 0) return hipSuccess;
    if (blocks <= 0) blocks = 8 * std::max(cus, 1);
    const uint64_t ntiles = (units + 255) / 256;
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, (uint64_t)blocks);
    const uint32_t flush_at = (uint32_t)std::max<uint64_t>(1, slots / (8ull * 4 * grid));
    hipLaunchKernelGGL(ppg_km_insert, dim3(grid), dim3(256), 0, s, set, words, (const uint2 *)rows, umap, (uint32_t)kc->k,
                       (int)(kc->flags & 1), units, (unsigned long long *)table, slots, km_shift(slots),
                       (unsigned long long)(slots / 2), flush_at, (unsigned long long *)acc);
    return hipGetLastError();
}

// acc[7 .. 9], acc[11] and the spectrum must be zero, acc[10] all ones before
hipError_t ppg_launch_km_stats(hipStream_t s, const uint64_t *table, uint64_t slots, uint64_t *acc) {
    hipLaunchKernelGGL(ppg_km_stats, dim3(km_row_blocks(slots)), dim3(256), 0, s, (const unsigned long long *)table, slots,
                       (unsigned long long *)acc);
    hipLaunchKernelGGL(ppg_km_maxkey, dim3(km_row_blocks(slots)), dim3(256), 0, s, (const unsigned long long *)table, slots,
                       (unsigned long long *)acc);
    return hipGetLastError();
}

// *cursor must be zero before
hipError_t ppg_launch_km_select(hipStream_t s, const uint64_t *table, uint64_t slots, int64_t min_count, uint64_t *out,
                                int64_t out_cap, uint64_t *cursor) {
    const unsigned blocks = (unsigned)std::min<uint64_t>((slots + kKmSelRows - 1) / kKmSelRows, 4096);
    hipLaunchKernelGGL(ppg_km_select, dim3(blocks), dim3(256), 0, s, (const unsigned long long *)table, slots,
                       (unsigned long long)min_count, (unsigned long long *)out, (uint64_t)out_cap,
                       (unsigned long long *)cursor);
    return hipGetLastError();
}

hipError_t ppg_launch_km_lookup(hipStream_t s, const uint64_t *table, uint64_t slots, const uint64_t *keys, int64_t nkeys,
                                int64_t *counts) {
    if (nkeys <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppg_km_lookup, dim3((unsigned)((nkeys + 255) / 256)), dim3(256), 0, s,
                       (const unsigned long long *)table, slots, km_shift(slots), (const unsigned long long *)keys, nkeys,
                       counts);
    return hipGetLastError();
}
