// ppg_find.h — the block search of ppg_chunk.cpp's launches (ppg_find.cpp): lone chunks' inner deflate block
// starts found on the GPU.  It knows a stream and its own scratch, nothing of the service's slots or threads.
#pragma once
#include "ppg_host.h"
#include <chrono>
#include <stdlib.h>

// PPG_CHUNK_VERBOSE=1: a launch's phases (ms) on stderr -- where a lone chunk's latency goes
struct PhaseClock {
    bool on;
    std::chrono::steady_clock::time_point t0, t;
    char buf[512];
    int n = 0;
    PhaseClock() : on(getenv("PPG_CHUNK_VERBOSE") != nullptr) { t0 = t = std::chrono::steady_clock::now(); buf[0] = 0; }
    void mark(const char *what, hipStream_t s = nullptr) {
        if (!on) return;
        if (s) (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        n += snprintf(buf + n, sizeof buf - (size_t)n, " %s %.3f", what,
                      std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
        if (n >= (int)sizeof buf) n = (int)sizeof buf - 1;
    }
    // (at: the launch's start, ms on the steady clock -- overlapping launches of several slots line up)
    void dump(size_t reqs, int slot) {
        if (on)
            fprintf(stderr, "PPG_CHUNK launch of %zu: total %.3f ms: slot %d at %.3f:%s\n", reqs,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), slot,
                    std::chrono::duration<double, std::milli>(t0.time_since_epoch()).count(), buf);
    }
};

// One chunk to search.  Coordinates: bits in the launch's gathered comp buffer, outputs in the
// launch's output (the shard's virtual ones).
struct FindChunk {
    uint64_t bit0, bit1;                // compressed bits of the chunk: [from's start bit, slice end)
    uint64_t bit_end;                   // to's block start (8 to.Input - to.Bits), or bit1 for the last chunk
    int64_t out0;                       // the chunk's first output byte (launch coordinates)
    int64_t len;                        // the chunk's output bytes
    uint32_t win;                       // the Point's 32 KiB: window `win` of the shard's device dicts
};

// device scratch of the block search, both paths (grow only)
struct FindScratch {
    DevBuf<uint16_t> sym;                  // materialise path: every piece's pass-1 symbols, whole
    DevBuf<PpgMatInfo> mi;                 // ... and each materialised piece's info
    DevBuf<uint64_t> lo, hi, cand;
    DevBuf<PpgInflateJob> jobs;
    DevBuf<PpgInflateResult> res;
    DevBuf<PpgBlockEnd> blk;
    DevBuf<uint8_t> ring, ta, ident, W;
    DevBuf<PpgGather> gat;
    DevBuf<uint32_t> slots, pick;
    DevBuf<uint4> chains;
    DevBuf<uint8_t> packed;
};

size_t find_max_pieces();         // what a launch reserves per searched chunk: pieces at most (either path),
size_t find_max_side_windows();   // and side windows at most (the two-decode path; the materialise path fills none)

// the two-decode path: side points (bit, output, 32 KiB window) appended for the chunks `ch`;
// nsplit counts the chunks that got any
int find_side_points(hipStream_t s, FindScratch &F, const uint32_t *comp, uint64_t nwords, const uint8_t *dwin,
                     const std::vector<FindChunk> &ch, std::vector<int64_t> &sbit, std::vector<int64_t> &sout,
                     ByteVec &swin, int64_t &nsplit, PhaseClock &clk);
// the materialise path: per chunk whether its pieces cover it, and then their materialise info (symbols in F.sym,
// histories in F.W) and side points.  PPG_MEM_ERROR: no room for the scratch, the caller decodes the chunks whole
int find_mat(hipStream_t s, FindScratch &F, const uint32_t *comp, uint64_t nwords, const uint8_t *dwin,
             const std::vector<FindChunk> &ch, std::vector<uint8_t> &covered, std::vector<std::vector<PpgMatInfo>> &pmi,
             std::vector<std::vector<int64_t>> &pbit, std::vector<std::vector<int64_t>> &pout, PhaseClock &clk);
