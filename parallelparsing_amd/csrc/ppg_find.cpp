// ppg_find.cpp — the block search of the per-chunk Decompress (ppg_chunk.cpp's launches).
//
// Side points for chunks whose index has none (a .gzi carries only the Points): the inner deflate
// block starts of each chunk found on the GPU the way the GPU CreateIndex finds them
// (ppg_index_gpu.cpp) -- candidate dynamic-block headers every ~1/16 of the chunk's compressed bytes
// (ppg_block_find_kernel), each piece but the last decoded with symbolic output until a block ends
// at or past the next candidate (the inflate kernel's IX mode, the same kernels as CreateIndex pass
// 1), the chain of block ends walked from the chunk's own Point (a block end that is not the next
// candidate's start ends the chain there: that end is still a real block start), and the 32 KiB
// history at every verified block start resolved from the pieces' symbolic tails starting from the
// Point's window (ppg_resolve_*).  A lone chunk then decodes as ~16 waves instead of one: the
// speculative pass costs about one piece's decode, the split decode another.  That is the
// two-decode path, find_side_points; the materialise path, find_mat, keeps pass 1's symbols whole
// and writes the chunk out from them.  Both run the stages written once each below.
#include "ppg_find.h"
#include "ppg_launch.h"
#include <numeric>

namespace {

constexpr uint64_t kPieceRing = 65536;     // CreateIndex pass 1's symbolic output ring per piece (IX_RING_BYTES)
constexpr uint64_t kSideRanges = 16, kSideMinRange = 48 * 1024;   // the two-decode path's ranges (as kMat* below)
constexpr uint64_t kMatRatio = 10;        // symbol capacity per compressed byte of a piece (FASTQ: ~4)
// candidate ranges per chunk and their least compressed size: a zlib -6 FASTQ block is ~16 K symbols,
// ~20 KB of gzip, so ranges of ~1/16 chunk (60 KB) held 2-3 block starts of which the finder keeps
// the first, and the slowest piece was several blocks long.  r05 (tools/chunk_latency.py, one box):
// 16 ranges / 48 KiB: T = 1 5.68 ms (pass 1 3.8); 24 / 32: 4.72; 32 / 24: 3.94 (2.36); 48 / 16:
// 2.90 (1.60); 64 / 12: 2.85 (1.61) -- pieces of one block each from 48 on; a 256-chunk launch
// ~45 ms at every setting (the search grows as pass 1 shrinks)
constexpr uint64_t kMatRanges = 48;
constexpr uint64_t kMatMinRange = 16 * 1024;

#define TRY(x) do { const int rc_ = (x); if (rc_ != PPG_OK) return rc_; } while (0)

// grow a big scratch buffer of the block search; out of device memory (e.g. beside a resident
// DecompressAll shard) is not a failure of the requests: the caller decodes them whole instead
#define GROW_OR_SKIP(b, n)                                                                      \
    do {                                                                                        \
        const hipError_t grow_e = grow_buf(b, n);                                               \
        if (grow_e == hipErrorOutOfMemory) {                                                    \
            (void)hipGetLastError();                                                            \
            fprintf(stderr, "ppgpu: block search scratch %s of %zu elements: out of device memory, " \
                    "the launch's chunks decoded whole\n", #b, (size_t)(n));                   \
            return PPG_MEM_ERROR;                                                               \
        }                                                                                       \
        if (grow_e != hipSuccess) {                                                             \
            fprintf(stderr, "ppgpu: grow %s failed: %s\n", #b, hipGetErrorString(grow_e));     \
            return PPG_DEVICE_ERROR;                                                            \
        }                                                                                       \
    } while (0)

// waves per candidate range of the block search: enough for ~16,384 waves in all, two generations of
// the GPU's wave slots (a lone chunk's 48 ranges are searched by 32 waves each; r05: at 4,096 waves a
// launch of 256 chunks searched its 3,840 ranges with one wave each, 7.0 ms)
int find_sub(int ranges) { return std::max(1, std::min(32, 16384 / std::max(1, ranges))); }

// ---- the stages both paths share ----
// candidates: the first dynamic-block header in each of up to `ranges` ranges of >= min_range
// compressed bytes per chunk.  Chunk c's are cand[cfirst[c] .. cfirst[c + 1]), ~0 where none is found.
int find_candidates(hipStream_t s, FindScratch &F, const uint32_t *comp, uint64_t nwords,
                    const std::vector<FindChunk> &ch, uint64_t ranges, uint64_t min_range, std::vector<size_t> &cfirst,
                    std::vector<uint64_t> &cand) {
    std::vector<uint64_t> lo, hi;
    cfirst.assign(ch.size() + 1, 0);
    for (size_t c = 0; c < ch.size(); c++) {
        const uint64_t span = ch[c].bit1 - ch[c].bit0;
        const uint64_t pb = std::max<uint64_t>(8ull * min_range, span / ranges);
        for (uint64_t a = ch[c].bit0 + pb; a + 8ull * 1024 < ch[c].bit1; a += pb) {
            lo.push_back(a);
            hi.push_back(std::min(a + pb, ch[c].bit1));
        }
        cfirst[c + 1] = lo.size();
    }
    const size_t nc = lo.size();
    cand.resize(nc);
    if (!nc) return PPG_OK;
    HIPCHK(grow_buf(F.lo, nc));
    HIPCHK(grow_buf(F.hi, nc));
    HIPCHK(grow_buf(F.cand, nc));
    HIPCHK(hipMemcpyAsync(F.lo.p, lo.data(), 8 * nc, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(F.hi.p, hi.data(), 8 * nc, hipMemcpyHostToDevice, s));
    HIPCHK(ppg_launch_block_find(s, comp, nwords, F.lo.p, F.hi.p, F.cand.p, (int)nc, find_sub((int)nc)));
    HIPCHK(hipMemcpyAsync(cand.data(), F.cand.p, 8 * nc, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PPG_OK;
}

// u16 0..32767, uploaded once per scratch (a blocking copy: `id` dies here): position p < 0 of a piece
// is history symbol 32768 + p
int upload_ident(FindScratch &F) {
    if (F.ident.p) return PPG_OK;
    std::vector<uint16_t> id(kWin);
    std::iota(id.begin(), id.end(), 0);
    HIPCHK(F.ident.alloc(2 * kWin));
    HIPCHK(hipMemcpy(F.ident.p, id.data(), 2 * kWin, hipMemcpyHostToDevice));
    return PPG_OK;
}

// One pass-1 job: symbolic decode from bit `start` until a block ends at or past `stop`, reading
// no further than bit_limit; its block ends from slot nblk on (one per 2 KiB of compressed bytes up
// to the stop, and 64), which advances past them.
PpgInflateJob pass1_job(uint64_t start, uint64_t stop, uint64_t bit_limit, uint64_t out_off, uint64_t out_len,
                        uint64_t &nblk) {
    PpgInflateJob J{};
    J.bit_start = start;
    J.bit_limit = bit_limit;
    J.out_off = out_off;
    J.out_len = out_len;
    J.expect_end = ~0ull;
    J.stop_bit = stop;
    J.blk_off = (uint32_t)nblk;
    J.blk_cap = (uint32_t)((stop - start) / 8 / 2048 + 64);
    nblk += J.blk_cap;
    return J;
}

// pass 1 of jobs [first, first + n): uploaded, decoded into `out` (full: every symbol kept, IXF;
// else the last 64 KiB of each piece in its ring, IX), their results and block ends fetched
int run_pass1(hipStream_t s, FindScratch &F, const uint32_t *comp, uint64_t nwords,
              const std::vector<PpgInflateJob> &jobs, size_t first, size_t n, bool full, uint8_t *out,
              std::vector<PpgInflateResult> &res, std::vector<PpgBlockEnd> &blk) {
    const size_t b0 = jobs[first].blk_off, b1 = (size_t)jobs[first + n - 1].blk_off + jobs[first + n - 1].blk_cap;
    HIPCHK(hipMemcpyAsync(F.jobs.p + first, jobs.data() + first, sizeof(PpgInflateJob) * n, hipMemcpyHostToDevice, s));
    HIPCHK((full ? ppg_launch_inflate_ixf : ppg_launch_inflate_ix)(s, comp, nwords, F.jobs.p + first, F.ident.p, out,
                                                                   F.res.p + first, F.blk.p, (int)n));
    res.resize(first + n);   // (MBs of block ends zeroed while the kernel runs)
    blk.resize(b1);
    HIPCHK(hipMemcpyAsync(res.data() + first, F.res.p + first, sizeof(PpgInflateResult) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(blk.data() + b0, F.blk.p + b0, sizeof(PpgBlockEnd) * (b1 - b0), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PPG_OK;
}

// the symbolic tails: the last 32 Ki symbols of each piece (from byte 2 * out_off of `out`; mask: the
// ring's, or ~0 for whole symbols) as two 32 KiB byte halves in F.ta.  g, the copy's source, is the
// caller's: it lives until the stream is next waited for (resolve_chains).
int gather_tails(hipStream_t s, FindScratch &F, const uint8_t *out, const std::vector<PpgInflateJob> &jobs,
                 const std::vector<PpgInflateResult> &res, uint64_t mask, std::vector<PpgGather> &g) {
    const size_t n = jobs.size();
    g.resize(2 * n);
    for (size_t q = 0; q < n; q++) {
        const uint64_t endb = 2 * res[q].produced, base = 2 * jobs[q].out_off;
        g[2 * q] = PpgGather{base, (uint64_t)kWin, endb - kWin, mask, 0};
        g[2 * q + 1] = PpgGather{base, (uint64_t)kWin, endb, mask, 0};
    }
    HIPCHK(grow_buf(F.gat, 2 * n));
    HIPCHK(hipMemcpyAsync(F.gat.p, g.data(), sizeof(PpgGather) * 2 * n, hipMemcpyHostToDevice, s));
    HIPCHK(ppg_launch_gather(s, out, F.ident.p, F.gat.p, F.ta.p, nullptr, nullptr, (int)(2 * n)));
    return PPG_OK;
}

// histories along every non-empty chain, in one launch: chunk c's W[wbase[c]] = its Point's window,
// W[wbase[c] + j + 1] = T_chain[c][j](W[wbase[c] + j]) -- up to the start of the chain's last piece, or
// with `past_last` to its end too.  F.W holds nslots windows (grown by the caller).  Waits for the
// stream: the H2D sources here and in gather_tails are pageable vectors that die with their frames
// (the phase clock syncs only when verbose).
int resolve_chains(hipStream_t s, FindScratch &F, const std::vector<FindChunk> &ch,
                   const std::vector<std::vector<uint32_t>> &chain, const std::vector<size_t> &wbase, size_t nslots,
                   bool past_last, const uint8_t *dwin) {
    HIPCHK(grow_buf(F.slots, nslots));
    std::vector<uint32_t> slots(nslots, 0);
    std::vector<uint4> cs;
    for (size_t c = 0; c < ch.size(); c++) {
        if (chain[c].empty()) continue;
        std::copy(chain[c].begin(), chain[c].end(), slots.begin() + (ptrdiff_t)wbase[c]);
        cs.push_back(uint4{(uint32_t)wbase[c], (uint32_t)chain[c].size() + past_last, ch[c].win, 0});
    }
    HIPCHK(grow_buf(F.chains, cs.size()));
    HIPCHK(hipMemcpyAsync(F.slots.p, slots.data(), 4 * nslots, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(F.chains.p, cs.data(), sizeof(uint4) * cs.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ppg_launch_resolve_chains(s, F.ta.p, F.slots.p, F.chains.p, (int)cs.size(), dwin, F.W.p));
    HIPCHK(hipStreamSynchronize(s));
    return PPG_OK;
}

}  // namespace

size_t find_max_pieces() { return (size_t)std::max(kMatRanges, kSideRanges); }
size_t find_max_side_windows() { return (size_t)kSideRanges; }   // (15 inner starts per chunk at most)

int find_side_points(hipStream_t s, FindScratch &F, const uint32_t *comp, uint64_t nwords, const uint8_t *dwin,
                     const std::vector<FindChunk> &ch, std::vector<int64_t> &sbit, std::vector<int64_t> &sout,
                     ByteVec &swin, int64_t &nsplit, PhaseClock &clk) {
    // candidates: the chunk cut into up to 16 pieces of >= 48 KiB of compressed bytes
    std::vector<size_t> cfirst;
    std::vector<uint64_t> cand;
    TRY(find_candidates(s, F, comp, nwords, ch, kSideRanges, kSideMinRange, cfirst, cand));
    if (cand.empty()) return PPG_OK;
    clk.mark("f.cand");
    // pieces: chunk c's Point, then its candidates; every piece but the last decoded to the next
    std::vector<PpgInflateJob> jobs;
    std::vector<size_t> pfirst(ch.size() + 1, 0);
    uint64_t nblk = 0;
    for (size_t c = 0; c < ch.size(); c++) {
        std::vector<uint64_t> st{ch[c].bit0};
        for (size_t k = cfirst[c]; k < cfirst[c + 1]; k++)
            if (cand[k] != ~0ull && cand[k] > st.back()) st.push_back(cand[k]);
        for (size_t j = 0; j + 1 < st.size(); j++)
            jobs.push_back(pass1_job(st[j], st[j + 1], ch[c].bit1, jobs.size() * kPieceRing, 0, nblk));
        pfirst[c + 1] = jobs.size();
    }
    const size_t np = jobs.size();
    if (!np) return PPG_OK;
    HIPCHK(grow_buf(F.jobs, np));
    HIPCHK(grow_buf(F.res, np));
    HIPCHK(grow_buf(F.blk, (size_t)nblk));
    HIPCHK(grow_buf(F.ring, np * 2 * kPieceRing));
    HIPCHK(grow_buf(F.ta, np * 2 * kWin));
    TRY(upload_ident(F));
    std::vector<PpgInflateResult> res;
    std::vector<PpgBlockEnd> blk;
    TRY(run_pass1(s, F, comp, nwords, jobs, 0, np, false, F.ring.p, res, blk));
    clk.mark("f.pass1");
    std::vector<PpgGather> g;
    TRY(gather_tails(s, F, F.ring.p, jobs, res, 2 * kPieceRing - 1, g));
    // the chains: piece j of a chunk is followed when its last block end is piece j+1's start
    std::vector<std::vector<uint32_t>> chain(ch.size());
    // the side point of a chain end is the FIRST block end of its piece with the same output: a
    // sync flush's empty stored block (pigz, Z_SYNC_FLUSH) ends at the same output as the block
    // before it, and the split decode of the piece before a side point stops (pos == len, the
    // end-of-block consumed) at that first end, not past the empty block (a side point there was
    // a DATA_ERROR in ppg_split_merge).  An end that adds no output, or reaches the chunk's end,
    // is walked through but gets no side point (keep = 0).
    struct End { uint64_t bit, out; bool keep; };
    std::vector<std::vector<End>> ends(ch.size());   // chunk-relative output
    for (size_t c = 0; c < ch.size(); c++) {
        uint64_t outc = 0, last_kept = 0;
        for (size_t q = pfirst[c]; q < pfirst[c + 1]; q++) {
            const PpgInflateResult &r = res[q];
            const uint32_t nb = std::min(r.nblocks, jobs[q].blk_cap);
            if (r.status != 0 || nb == 0 || r.last || (r.flags & (PPG_FLAG_BLK_FULL | PPG_FLAG_OVERRUN))) break;
            const PpgBlockEnd *bl = blk.data() + jobs[q].blk_off;
            const uint64_t E = bl[nb - 1].end_bit;
            if (E >= ch[c].bit_end || bl[nb - 1].out_end != r.produced) break;
            uint32_t f = nb - 1;
            while (f > 0 && bl[f - 1].out_end == bl[nb - 1].out_end) f--;
            outc += r.produced;
            const bool keep = outc > last_kept && (int64_t)outc < ch[c].len;
            if (keep) last_kept = outc;
            chain[c].push_back((uint32_t)q);
            ends[c].push_back(End{bl[f].end_bit, outc, keep});
            if (q + 1 >= pfirst[c + 1] || jobs[q + 1].bit_start != E) break;   // the next candidate was false
        }
    }
    // histories at the verified block ends, every chain in one launch: W[0] = the Point's window,
    // W[j+1] = T_j(W[j]); the kept ones packed on the device and copied back at once
    size_t wmax = 0;
    for (size_t c = 0; c < ch.size(); c++) wmax = std::max(wmax, chain[c].size() + 1);
    if (wmax < 2) return PPG_OK;
    HIPCHK(grow_buf(F.W, ch.size() * wmax * kWin));
    std::vector<size_t> wbase(ch.size());
    for (size_t c = 0; c < ch.size(); c++) wbase[c] = c * wmax;
    TRY(resolve_chains(s, F, ch, chain, wbase, ch.size() * wmax, true, dwin));
    const size_t base = sbit.size();
    std::vector<uint32_t> pick;
    for (size_t c = 0; c < ch.size(); c++) {
        bool any = false;
        for (size_t j = 0; j < ends[c].size(); j++) {
            const End &e = ends[c][j];
            if (!e.keep) continue;
            pick.push_back((uint32_t)(wbase[c] + j + 1));   // W[j + 1]: the history at the end of chain piece j
            sbit.push_back((int64_t)e.bit);
            sout.push_back(ch[c].out0 + (int64_t)e.out);
            any = true;
        }
        nsplit += any;
    }
    swin.resize((base + pick.size()) * kWin);
    if (!pick.empty()) {
        HIPCHK(grow_buf(F.pick, pick.size()));
        HIPCHK(grow_buf(F.packed, pick.size() * kWin));
        HIPCHK(hipMemcpyAsync(F.pick.p, pick.data(), 4 * pick.size(), hipMemcpyHostToDevice, s));
        HIPCHK(ppg_launch_pick_windows(s, F.W.p, F.pick.p, (int)pick.size(), F.packed.p));
        HIPCHK(hipMemcpyAsync(swin.data() + base * kWin, F.packed.p, pick.size() * kWin, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));   // pick's upload, the windows' copy back
    }
    clk.mark("f.resolve");
    return PPG_OK;
}

// ---- the materialise path: one symbolic decode per piece instead of two (r05) ----
// A launch of chunks of plain indexes (no side points of their own) splits each chunk at the inner
// block starts found on the GPU as find_side_points does, but its pass 1 covers the WHOLE chunk --
// the last piece too, up to the chunk's end -- and keeps every piece's symbolic output whole
// (ppg_inflate_kernel IXF).  A chunk whose chain of block ends is verified from its Point to its
// end gets its pieces' exact starting histories resolved from the symbolic tails and is then
// written out from the symbols (ppg_materialize_kernel, with the fused newline census) -- no second
// decode; any other chunk is decoded whole, one wave, in the same launch.
// A lone 10,000-record chunk: find ~0.5 ms + one symbolic decode of a single deflate block (~4 ms)
// + resolve + materialise, instead of that plus a second decode of the same block.
int find_mat(hipStream_t s, FindScratch &F, const uint32_t *comp, uint64_t nwords, const uint8_t *dwin,
             const std::vector<FindChunk> &ch, std::vector<uint8_t> &covered, std::vector<std::vector<PpgMatInfo>> &pmi,
             std::vector<std::vector<int64_t>> &pbit, std::vector<std::vector<int64_t>> &pout, PhaseClock &clk) {
    covered.assign(ch.size(), 0);
    pmi.assign(ch.size(), {});
    pbit.assign(ch.size(), {});
    pout.assign(ch.size(), {});
    std::vector<size_t> cfirst;
    std::vector<uint64_t> cand;
    TRY(find_candidates(s, F, comp, nwords, ch, kMatRanges, kMatMinRange, cfirst, cand));
    clk.mark("f.cand");
    // pieces: the Point, the candidates, up to the chunk's end; symbol capacity by compressed size
    auto sym_cap = [](uint64_t start, uint64_t stop) {
        // (at least 192 Ki symbols, ~1.5 zlib -6 FASTQ blocks: a piece whose next candidate is false
        // decodes on to the next real block end, a whole block past a stop that may be only a few
        // KB away; a piece of a typical ~20 KB range gets its 10x anyway, so the floor costs little)
        return std::max<uint64_t>(192 * 1024, kMatRatio * ((stop - start) / 8 + 64));
    };
    std::vector<PpgInflateJob> jobs;   // a piece is its job: bits [bit_start, stop_bit), symbols out_off / out_len
    std::vector<size_t> pfirst(ch.size() + 1, 0);
    uint64_t syms = 0, nblk = 0, maxcap = 0;
    for (size_t c = 0; c < ch.size(); c++) {
        std::vector<uint64_t> st{ch[c].bit0};
        for (size_t k = cfirst[c]; k < cfirst[c + 1]; k++)
            if (cand[k] != ~0ull && cand[k] > st.back() && cand[k] < ch[c].bit_end) st.push_back(cand[k]);
        st.push_back(ch[c].bit_end);
        for (size_t j = 0; j + 1 < st.size(); j++) {
            const uint64_t cap = sym_cap(st[j], st[j + 1]);
            // the piece may read up to its chunk's slice end (the last block of a non-final piece
            // ends past its stop when the next candidate was false)
            jobs.push_back(pass1_job(st[j], st[j + 1], ch[c].bit1, syms, cap, nblk));
            syms += cap + 2048;   // flushes may run up to a unit past the capacity check
            maxcap = std::max(maxcap, cap);
        }
        pfirst[c + 1] = jobs.size();
    }
    const size_t np = jobs.size();
    if (!np) return PPG_OK;
    // a repair piece per chunk at most (below): its symbols, block ends and job reserved up front
    // (grow_buf does not keep contents, and a hipFree mid-launch waits for the whole device)
    const size_t nrep_cap = ch.size();
    const uint64_t rep_syms = std::max<uint64_t>(4 * (maxcap + 2048), syms / 16);
    const uint64_t rep_blk = 64 * nrep_cap + rep_syms / (kMatRatio * 2048) + 64;
    HIPCHK(grow_buf(F.jobs, np + nrep_cap));
    HIPCHK(grow_buf(F.res, np + nrep_cap));
    GROW_OR_SKIP(F.blk, (size_t)(nblk + rep_blk));
    GROW_OR_SKIP(F.sym, (size_t)(syms + rep_syms) + 64);
    GROW_OR_SKIP(F.ta, (np + nrep_cap) * 2 * kWin);
    clk.mark("f.grow");
    TRY(upload_ident(F));
    std::vector<PpgInflateResult> res;
    std::vector<PpgBlockEnd> blk;
    TRY(run_pass1(s, F, comp, nwords, jobs, 0, np, true, (uint8_t *)F.sym.p, res, blk));
    clk.mark("f.pass1");
    // a chunk is covered when its pieces chain from its Point to its end: each piece's last block
    // end is where the chain's next piece starts -- normally the next candidate; after a false
    // candidate (its piece fails, or the piece before it decodes on to the next real block end) the
    // first later piece that starts there, the false ones skipped (r05: ~0.6% of chunks at 48
    // ranges fell back to a one-wave decode of ~45 ms) --, the chain's last piece ends exactly at
    // the chunk's end (or with the final block, for the file's last chunk), and their outputs add up.
    // Two more cases chain (r05: 2 chunks in 1,024 were still left to the one-wave decode):
    //  - the real block start after a false candidate is no candidate at all (the finder keeps one
    //    per range): a repair piece from that block end to the next good piece's start, decoded in
    //    a second, small pass 1;
    //  - an index's last chunk, whose end is known only as its slice's last byte (no R-E5 end check:
    //    expect_end ~0): its last piece ends a block inside that byte, with every byte of the chunk,
    //    and decodes on into a next block header the slice does not hold, failing -- the piece is
    //    taken up to that block end (r05: index chunk 1023 of the bench's per-chunk legs).
    std::vector<size_t> wbase(ch.size(), 0);
    std::vector<std::vector<uint32_t>> chain(ch.size());
    std::vector<uint64_t> E(np, 0);
    std::vector<uint8_t> cut(np, 0);                      // last pieces taken up to a block end in the slice's last byte
    std::vector<std::vector<uint32_t>> reps(ch.size());   // each chunk's repair pieces (indexes >= np)
    struct Repair { size_t c; uint64_t start, stop; };
    std::vector<Repair> want;
    // chunk c's chain; 0 when covered, else why not (PPG_CHUNK_VERBOSE)
    auto walk = [&](size_t c, bool may_repair) -> int {
        chain[c].clear();
        uint64_t tot = 0;
        size_t q = pfirst[c];
        for (;;) {
            PpgInflateResult &r = res[q];
            const uint32_t nb = std::min(r.nblocks, jobs[q].blk_cap);
            if (r.status != 0 && nb > 0 && ch[c].bit_end == ch[c].bit1) {   // an index's last chunk
                const PpgBlockEnd &e = blk[jobs[q].blk_off + nb - 1];
                if (e.end_bit <= ch[c].bit_end && ch[c].bit_end - e.end_bit < 8 &&
                    tot + e.out_end == (uint64_t)ch[c].len && e.out_end <= jobs[q].out_len) {
                    r.status = 0;
                    r.flags = 0;
                    r.produced = e.out_end;
                    r.nblocks = nb;
                    r.last = 0;
                    cut[q] = 1;
                }
            }
            if (r.status != 0 || nb == 0 || (r.flags & (PPG_FLAG_BLK_FULL | PPG_FLAG_OVERRUN)))
                return r.status != 0 ? 1 : nb == 0 ? 2 : (r.flags & PPG_FLAG_BLK_FULL) ? 3 : 4;
            const PpgBlockEnd &e = blk[jobs[q].blk_off + nb - 1];
            if (e.out_end != r.produced) return 5;
            E[q] = e.end_bit;
            chain[c].push_back((uint32_t)q);
            tot += r.produced;
            if (e.end_bit == ch[c].bit_end || cut[q] || (r.last && ch[c].bit_end == ch[c].bit1))
                return (int64_t)tot == ch[c].len ? 0 : 9;
            if (r.last) return 6;
            size_t nx = q < np ? q + 1 : pfirst[c];   // the piece that starts at this end
            while (nx < pfirst[c + 1] && jobs[nx].bit_start < e.end_bit) nx++;
            if (nx < pfirst[c + 1] && jobs[nx].bit_start == e.end_bit) {
                q = nx;
                continue;
            }
            size_t rq = ~(size_t)0;
            for (uint32_t x : reps[c])
                if (jobs[x].bit_start == e.end_bit) rq = x;
            if (rq != ~(size_t)0) {
                q = rq;
                continue;
            }
            if (may_repair) {   // up to the next piece that decoded, or the chunk's end
                while (nx < pfirst[c + 1] && res[nx].status != 0) nx++;
                want.push_back(Repair{c, e.end_bit, nx < pfirst[c + 1] ? jobs[nx].bit_start : ch[c].bit_end});
            }
            return 7;
        }
    };
    std::vector<int> why(ch.size(), 0);
    for (size_t c = 0; c < ch.size(); c++) why[c] = walk(c, true);
    if (!want.empty()) {   // the repair pass
        uint64_t rs = syms, rb = nblk;
        std::vector<size_t> rc;
        for (const Repair &w : want) {
            if (w.stop <= w.start) continue;
            const uint64_t cap = sym_cap(w.start, w.stop);
            uint64_t rb1 = rb;
            const PpgInflateJob J = pass1_job(w.start, w.stop, ch[w.c].bit1, rs, cap, rb1);
            if (rs + cap + 2048 > syms + rep_syms || rb1 > nblk + rep_blk) continue;   // the reserve is used up
            rb = rb1;
            reps[w.c].push_back((uint32_t)jobs.size());
            jobs.push_back(J);
            rc.push_back(w.c);
            rs += cap + 2048;
        }
        const size_t nr = jobs.size() - np;
        if (nr) {
            E.resize(np + nr, 0);
            cut.resize(np + nr, 0);
            TRY(run_pass1(s, F, comp, nwords, jobs, np, nr, true, (uint8_t *)F.sym.p, res, blk));
            std::sort(rc.begin(), rc.end());
            rc.erase(std::unique(rc.begin(), rc.end()), rc.end());
            for (size_t c : rc) why[c] = walk(c, false);
        }
        clk.mark("f.repair");
    }
    size_t nw = 0;
    for (size_t c = 0; c < ch.size(); c++) {
        const bool ok = why[c] == 0;
        if (!ok && clk.on) {
            fprintf(stderr, "PPG_CHUNK not covered: chunk %zu reason %d after %zu chained of %zu pieces\n", c, why[c],
                    chain[c].size(), pfirst[c + 1] - pfirst[c]);
            for (size_t x = pfirst[c]; x < pfirst[c + 1]; x++) {
                const PpgInflateResult &r = res[x];
                const uint32_t nb = std::min(r.nblocks, jobs[x].blk_cap);
                fprintf(stderr, "  piece %zu bits [%llu,%llu) chunk [%llu,%llu) cap %llu: status %d flags %u produced %llu "
                        "blocks %u last_end %llu\n", x - pfirst[c], (unsigned long long)jobs[x].bit_start,
                        (unsigned long long)jobs[x].stop_bit, (unsigned long long)ch[c].bit0, (unsigned long long)ch[c].bit_end,
                        (unsigned long long)jobs[x].out_len, (int)r.status, (unsigned)r.flags, (unsigned long long)r.produced, nb,
                        nb ? (unsigned long long)blk[jobs[x].blk_off + nb - 1].end_bit : 0ull);
            }
        }
        covered[c] = ok;
        if (ok) {
            wbase[c] = nw;
            nw += chain[c].size();
        } else {
            chain[c].clear();   // (resolve_chains takes the non-empty ones)
        }
    }
    if (!nw) return PPG_OK;
    // symbolic tails (the last 32 Ki symbols of each piece, as two 32 KiB byte halves); while they are
    // gathered, the pieces' materialise info, side points at every later piece's start (launch
    // coordinates); then every covered chunk's starting histories: W[0] = the Point's window, W[j+1] = T_j(W[j])
    GROW_OR_SKIP(F.W, nw * kWin);
    std::vector<PpgGather> g;
    TRY(gather_tails(s, F, (const uint8_t *)F.sym.p, jobs, res, ~0ull, g));
    for (size_t c = 0; c < ch.size(); c++) {
        if (!covered[c]) continue;
        uint64_t outc = 0, last_end = 0;
        for (size_t j = 0; j < chain[c].size(); j++) {
            const size_t q = chain[c][j];
            last_end = E[q];
            if (res[q].produced == 0) continue;   // an empty piece (a flush block) adds nothing
            if (!pmi[c].empty()) {
                pbit[c].push_back((int64_t)jobs[q].bit_start);
                pout[c].push_back(ch[c].out0 + (int64_t)outc);
            }
            PpgMatInfo m{};
            m.sym_off = jobs[q].out_off;
            m.win_off = (wbase[c] + j) * (uint64_t)kWin;
            m.nblocks = res[q].nblocks;
            m.last = res[q].last;
            m.prev = pmi[c].empty() ? 0x100u : 0x1FFu;   // 0x100: the chunk job's own (set by the caller)
            pmi[c].push_back(m);
            outc += res[q].produced;
        }
        // each piece's end: where the next starts, the last one's block end
        for (size_t i = 0; i < pmi[c].size(); i++)
            pmi[c][i].end_bit = i + 1 < pmi[c].size() ? (uint64_t)pbit[c][i] : last_end;
        if (pmi[c].empty()) covered[c] = 0;
    }
    TRY(resolve_chains(s, F, ch, chain, wbase, nw, false, dwin));
    clk.mark("f.resolve");
    return PPG_OK;
}
