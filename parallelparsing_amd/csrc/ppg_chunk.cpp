// ppg_chunk.cpp — README "Decompress": one checkpoint at a time, thread safe
// (/root/reference/README.md:38-50 "must be thread safe"; Core.ExtractDeflateIndex,
// Decompressor/Core.cs:133-192, + Parsing.Parse as BatchedFASTQ.cs:63-74 runs them per task).
//
// The reference calls this once per chunk from a ThreadPool task per chunk (BatchedFASTQ.cs:62-77),
// each with its own ZStream.  On the GPU one chunk alone is one wave of the 8,192 the chip holds,
// so concurrent calls are *combined*: a call queues its request, and whichever waiting caller finds
// one of the ctx's four launch slots free takes the queued requests (up to 256) into one launch
// (flat combining).  A second launch starts beside a running one only once 16 requests queue, so
// the queue that builds during a launch goes into the next one.  Asynchronous requests
// (ppg_decompress_chunk_submit) are launched the same way by a launcher thread of the ctx, and
// their results copied out by a copier thread while the next launch runs.
//
// A slot owns everything a launch touches -- its stream, a one-batch ppg_shard, the gathered
// compressed slices (pinned + device), the pinned copy of the outputs and descriptors, the block
// search's scratch -- and its buffers only grow (geometrically), so a warm ctx makes no
// hipMalloc/hipFree per call: hipFree waits for the whole device.  Each synchronous caller copies
// its own chunk out of the slot's pinned results in parallel with the others; the slot is reused
// only after every such copy is done.
//
// Chunks whose index carries side points (ppg_index_build_gpu_side) are decoded as one wave per
// piece between their inner block starts (ppg_shard_set_split), exactly as DecompressAll does; the
// others get theirs found on the GPU (find_side_points, find_mat: ppg_find.cpp).
#include "ppg_host.h"
#include "ppg_find.h"
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <sys/mman.h>

namespace {

constexpr int kChunkSlots = 4;             // launches in flight / results being copied out
constexpr size_t kSliceAlign = 64;   // each gathered slice starts on its own 64-B line
// chunks per launch: the materialise path's limit (find_mat), whose launch of 256 warm chunks takes
// 41 ms against 63 ms for 258 on the two-decode path (r05g); no launch is too large for the block search
constexpr size_t kMaxBatch = 256;
// a second launch starts while one is decoding only with this many requests queued: otherwise the
// queue grows during the running launch and the next one takes all of it (r04: with two slots taken
// as soon as free, 64 callers were served ~12 at a time)
constexpr size_t kMinSecond = 16;
// launcher threads of asynchronous requests.  r05 (tools/chunk_latency.py, async depth 1024, three
// runs): one 19 / 31 / 39 M records/s, two 16 / 18 / 30 -- the second overlaps a launch's PCIe
// copies with the other's kernels, but the two launches' host copies (slices gathered, results
// copied out into fresh pages) then contend, and more slots are grown
constexpr int kLaunchers = 1;

struct ChunkReq {
    const ppg_index *ix;
    int32_t k;
    const uint8_t *slice;
    int64_t slice_len;
    // asynchronous requests (ppg_decompress_chunk_submit): where wait() copies the results
    bool async = false;
    uint8_t *out = nullptr;
    int64_t out_cap = 0;
    uint32_t *recs = nullptr;
    int64_t rec_cap = 0;
    // results, set by the launching caller
    bool done = false;
    int rc = PPG_OK;
    int slot = -1;
    const uint8_t *src = nullptr;       // chunk bytes in the slot's pinned results
    int64_t got = 0;
    const uint32_t *src_recs = nullptr;
    int64_t nrec = 0;
    // an async request's results already copied into out/recs by the launcher (fin_*: what wait() returns)
    bool copied = false;
    int fin_rc = PPG_OK;
    int64_t fin_len = 0;
    bool fin_nrec = false;
};

// memcpy of many (dst, src, len) spans: on the calling thread when small, else spread over up to
// 8 threads in 1 MiB pieces -- a launch gathers up to 256 slices into the pinned staging buffer and
// the async path copies up to a GiB of results into fresh caller pages (page faults included), which
// one thread does at a few GB/s
struct Span {
    uint8_t *dst;
    const uint8_t *src;
    size_t len;
};

void parallel_copy(const std::vector<Span> &v, bool caller_dst = false) {
    constexpr size_t kPiece = 1 << 20;
    size_t tot = 0;
    for (const Span &x : v) tot += x.len;
    if (tot < 8 * kPiece) {
        for (const Span &x : v)
            if (x.len) memcpy(x.dst, x.src, x.len);
        return;
    }
    // caller_dst: the caller's (often fresh) pages -- 2 MiB pages where a span covers them (advice
    // only, never on the slots' pinned buffers; r05, tools/chunk_latency.py: a 256-chunk launch's
    // 1 GB of results copied out in 30-36 ms instead of 62-70, async depth 256 30-33 M records/s
    // instead of 19-22)
    for (const Span &x : v) {
        if (!caller_dst) break;
        const uintptr_t a = ((uintptr_t)x.dst + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
        const uintptr_t b = ((uintptr_t)x.dst + x.len) & ~(uintptr_t)((2u << 20) - 1);
        if (b > a) (void)madvise((void *)a, b - a, MADV_HUGEPAGE);
    }
    std::vector<Span> pieces;
    for (const Span &x : v)
        for (size_t o = 0; o < x.len; o += kPiece) pieces.push_back(Span{x.dst + o, x.src + o, std::min(kPiece, x.len - o)});
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < pieces.size();) memcpy(pieces[i].dst, pieces[i].src, pieces[i].len);
    };
    std::vector<std::thread> th;
    const size_t nt = std::min<size_t>(8, tot / (4 * kPiece));
    try {
        for (size_t t = 1; t < nt; t++) th.emplace_back(work);
    } catch (...) {   // no threads: the calling thread copies everything
    }
    work();
    for (auto &t : th) t.join();
}

// What a decoded request hands its caller: the status (PPG_BUF_ERROR when a buffer is too small),
// the byte count, whether the record count is reported, and the copies out of the slot's results.
int result_spans(const ChunkReq &req, uint8_t *out, int64_t out_cap, uint32_t *recs, int64_t rec_cap, int64_t &len,
                 bool &with_nrec, std::vector<Span> &cp) {
    len = req.got;
    with_nrec = false;
    if (out) {
        if (req.got > out_cap) {
            len = 0;
            return PPG_BUF_ERROR;
        }
        if (req.got) cp.push_back(Span{out, req.src, (size_t)req.got});
    }
    with_nrec = true;
    if (recs) {
        if (req.nrec > rec_cap) return PPG_BUF_ERROR;
        if (req.nrec) cp.push_back(Span{(uint8_t *)recs, (const uint8_t *)req.src_recs, 16 * (size_t)req.nrec});
    }
    return PPG_OK;
}

struct ChunkSlot {
    hipStream_t s = nullptr;
    ppg_shard *sh = nullptr;
    PinnedBuf in;                       // the launch's slices, gathered
    DevBuf<uint8_t> comp;
    PinnedBuf res;                      // outputs, then descriptors
    FindScratch fs;
    bool busy = false;
    int readers = 0;                    // callers still copying out of `res`
};

}  // namespace

struct ChunkService {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<ChunkReq *> pending;
    ChunkSlot slot[kChunkSlots];
    int64_t calls = 0, launches = 0, max_batch = 0;
    int in_flight = 0;                                         // launches decoding now
    std::atomic<int64_t> found_chunks{0}, found_points{0};   // find_side_points' splits
    // the launcher of asynchronous requests (started by the first ppg_decompress_chunk_submit)
    ppg_ctx *ctx = nullptr;
    std::thread worker[kLaunchers];
    bool stop = false;
    std::chrono::steady_clock::time_point last_submit{};
    // the copier of asynchronous results: a launch's async requests are copied out here (holding a
    // reader on their slot) while the launcher leads the next launch on another slot
    struct CopyTask {
        int slot;
        std::vector<ChunkReq *> reqs;
    };
    std::deque<CopyTask> copies;
    std::thread copier;
};

ChunkService *chunk_service_new() { return new ChunkService; }

void chunk_service_free(ChunkService *svc) {
    if (!svc) return;
    {
        std::lock_guard<std::mutex> lk(svc->mu);
        svc->stop = true;
    }
    svc->cv.notify_all();
    for (auto &w : svc->worker)
        if (w.joinable()) w.join();
    if (svc->copier.joinable()) svc->copier.join();   // (it drains the queued copies first)
    for (auto &sl : svc->slot) {
        if (sl.sh) ppg_shard_free(sl.sh);
        if (sl.s) (void)hipStreamDestroy(sl.s);
    }
    delete svc;
}

namespace {

// side points of chunk k of ix (strictly inside it), in the launch's virtual coordinates: output =
// the chunk's offset in the launch output + its own offset, bit = the chunk's job bit + the same
// distance in the file
void side_points_of(const ppg_index *ix, int32_t k, uint64_t job_bit, int64_t out_base, std::vector<int64_t> &bit,
                    std::vector<int64_t> &out, ByteVec &win) {
    const auto &O = ix->side_out;
    if (O.empty()) return;
    const PpgPoint &from = ix->pts[(size_t)k], &to = ix->pts[(size_t)k + 1];
    const int64_t from_bit = 8 * from.input - from.bits;
    const size_t a = (size_t)(std::upper_bound(O.begin(), O.end(), from.output) - O.begin());
    const size_t b = (size_t)(std::lower_bound(O.begin(), O.end(), to.output) - O.begin());
    for (size_t q = a; q < b; q++) {
        bit.push_back((int64_t)job_bit + (ix->side_bit[q] - from_bit));
        out.push_back(out_base + (O[q] - from.output));
        win.insert(win.end(), ix->side_win.data() + q * kWin, ix->side_win.data() + (q + 1) * kWin);
    }
}

// The index's side points of chunk k lie strictly inside it in both output and compressed bits
// (side_points_of selects them by output).  Checked per request before the launch is built, so a bad
// side point fails only its own request, never the others sharing the launch (one bad
// point made ppg_shard_set_split fail the whole launch).
bool side_points_inside(const ppg_index *ix, int32_t k) {
    const auto &O = ix->side_out;
    if (O.empty()) return true;
    const PpgPoint &from = ix->pts[(size_t)k], &to = ix->pts[(size_t)k + 1];
    const int64_t from_bit = 8 * from.input - from.bits, to_bit = 8 * to.input - to.bits;
    const size_t a = (size_t)(std::upper_bound(O.begin(), O.end(), from.output) - O.begin());
    const size_t b = (size_t)(std::lower_bound(O.begin(), O.end(), to.output) - O.begin());
    int64_t prev = from_bit;
    for (size_t q = a; q < b; q++) {
        if (ix->side_bit[q] <= prev || ix->side_bit[q] >= to_bit) return false;
        prev = ix->side_bit[q];
    }
    return true;
}

// One launch of the requests `batch` on slot `sl` (the caller holds the slot, not the lock).  Sets
// every request's rc and, for a decoded chunk, where its bytes and descriptors sit in sl.res.
int run_launch(ppg_ctx *ctx, ChunkService &svc, ChunkSlot &sl, std::vector<ChunkReq *> &batch) {
    HIPCHK(hipSetDevice(ctx->device));
    PhaseClock pc;
    if (!sl.s) HIPCHK(hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking));
    if (!sl.sh) {
        sl.sh = new ppg_shard;
        sl.sh->ctx = ctx;
        sl.sh->stream = sl.s;
    }
    // requests the kernels can take, laid out slice after slice
    std::vector<ChunkReq *> go;
    std::vector<ChunkSpec> spec;
    std::vector<int64_t> at;
    size_t comp_len = 0;
    for (ChunkReq *r : batch) {
        const auto &P = r->ix->pts;
        int rc = ppg_index_validate(r->ix, r->k, 1);
        if (rc == PPG_OK && r->slice_len != P[(size_t)r->k + 1].input - P[(size_t)r->k].input + 1) rc = PPG_ARG_ERROR;
        if (rc == PPG_OK && r->ix->windows.size() < ((size_t)r->k + 1) * kWin) rc = PPG_ARG_ERROR;
        if (rc == PPG_OK && !side_points_inside(r->ix, r->k)) rc = PPG_ARG_ERROR;
        if (rc != PPG_OK) {
            r->rc = rc;
            continue;
        }
        go.push_back(r);
        at.push_back((int64_t)comp_len);
        spec.push_back(ChunkSpec{&P[(size_t)r->k], &P[(size_t)r->k + 1], r->ix->win((size_t)r->k), (int64_t)comp_len,
                                 (size_t)r->k + 2 == P.size()});
        comp_len += ((size_t)r->slice_len + kSliceAlign - 1) / kSliceAlign * kSliceAlign;
    }
    if (go.empty()) return PPG_OK;
    // the materialise path (find_mat) takes launches of plain indexes (of any size: kMaxBatch above)
    bool mat = !getenv("PPG_CHUNK_NO_FIND") && !getenv("PPG_CHUNK_NO_MAT");
    for (size_t i = 0; mat && i < go.size(); i++) mat = go[i]->ix->side_out.empty();
    {   // the shard's buffers with headroom, so launches of growing size do not reallocate each time
        size_t n = go.size(), offb = 0, tot = 0, nsub = 0, nwin = 0;
        for (ChunkReq *r : go) {
            const PpgPoint &from = r->ix->pts[(size_t)r->k], &to = r->ix->pts[(size_t)r->k + 1];
            offb += from.offset.size();
            tot += (size_t)std::max<int64_t>(to.output - from.output, 0);
            const auto &O = r->ix->side_out;
            const size_t own = (size_t)std::max<std::ptrdiff_t>(0, std::lower_bound(O.begin(), O.end(), to.output) -
                                                                      std::upper_bound(O.begin(), O.end(), from.output));
            nsub += own;
            nwin += own;
            if (O.empty()) {
                nsub += find_max_pieces();   // the block search's pieces at most
                // side windows: the materialise path fills none (its pieces start from resolved
                // histories, not dictionaries); find_side_points at most 15 per chunk (ADVICE r05:
                // 48 windows of 32 KiB per chunk were reserved and never written, ~400 MB per slot)
                if (!mat) nwin += find_max_side_windows();
            }
        }
        ppg_shard *sh = sl.sh;
        HIPCHK(grow_buf(sh->jobs, n));
        HIPCHK(grow_buf(sh->dicts, (n + nwin) * kWin));
        HIPCHK(grow_buf(sh->offs, offb + 16));
        HIPCHK(grow_buf(sh->oref, n));
        HIPCHK(grow_buf(sh->res, n));
        HIPCHK(grow_buf(sh->info, n));
        HIPCHK(grow_buf(sh->base, n));
        HIPCHK(grow_buf(sh->total, 1));
        HIPCHK(grow_buf(sh->out, tot + 64));
        HIPCHK(grow_buf(sh->recs, 4 * (tot / 256 + 1024)));
        HIPCHK(grow_buf(sh->nls, 2 * (tot / kNlBytesPerEntry + 64 * (n + nsub)) + 64));
        if (nsub) {
            HIPCHK(grow_buf(sh->sjobs, n + nsub));
            HIPCHK(grow_buf(sh->sres, n + nsub));
            HIPCHK(grow_buf(sh->sidx, n + 1));
        }
    }
    HIPCHK(grow_buf(sl.in, comp_len + 256));
    HIPCHK(grow_buf(sl.comp, comp_len + 256));
    {   // the slices, the alignment gaps and the 256-B tail zeroed (the kernels read whole words past a slice)
        std::vector<Span> cp;
        for (size_t i = 0; i < go.size(); i++) {
            const size_t end = (size_t)at[i] + (size_t)go[i]->slice_len;
            memset(sl.in.p + end, 0, (i + 1 < go.size() ? (size_t)at[i + 1] : comp_len + 256) - end);
            cp.push_back(Span{sl.in.p + at[i], go[i]->slice, (size_t)go[i]->slice_len});
        }
        parallel_copy(cp);
    }
    HIPCHK(hipMemcpyAsync(sl.comp.p, sl.in.p, comp_len + 256, hipMemcpyHostToDevice, sl.s));
    ppg_shard *sh = sl.sh;
    pc.mark("h2d", sl.s);
    int rc = shard_prepare_specs(sh, spec.data(), (int32_t)go.size(), sl.comp.p, (int64_t)comp_len, 0, sl.s, nullptr);
    if (rc != PPG_OK) return rc;
    pc.mark("prepare");
    auto find_chunk = [&](size_t i) {   // chunk i of the launch, for the block search
        const PpgInflateJob &J = sh->h_jobs[i];
        return FindChunk{J.bit_start, J.bit_limit, J.expect_end != ~0ull ? J.expect_end : J.bit_limit, sh->h_pout[i],
                         (int64_t)J.out_len, (uint32_t)i};
    };
    if (mat) {   // the materialise path (find_mat, ppg_find.cpp)
        std::vector<FindChunk> find;
        for (size_t i = 0; i < go.size(); i++) find.push_back(find_chunk(i));
        std::vector<uint8_t> covered;
        std::vector<std::vector<PpgMatInfo>> pmi;
        std::vector<std::vector<int64_t>> pbit, pout;
        rc = find_mat(sl.s, sl.fs, (const uint32_t *)sl.comp.p, sh->nwords, sh->dicts.p, find, covered, pmi, pbit, pout, pc);
        if (rc == PPG_MEM_ERROR) {   // no room for the search's scratch: every chunk decoded whole
            covered.assign(go.size(), 0);
            rc = PPG_OK;
        }
        if (rc != PPG_OK) return rc;
        std::vector<int64_t> sbit, sout;
        size_t ncov = 0;
        for (size_t i = 0; i < go.size(); i++) {
            if (!covered[i]) continue;
            ncov++;
            sbit.insert(sbit.end(), pbit[i].begin(), pbit[i].end());
            sout.insert(sout.end(), pout[i].begin(), pout[i].end());
        }
        svc.found_chunks += (int64_t)ncov;
        svc.found_points += (int64_t)sbit.size();
        if (!sbit.empty()) {   // (chunks of one piece each only: decoded as usual)
            rc = shard_set_split_impl(sh, (int32_t)sbit.size(), sbit.data(), sout.data(), nullptr, false);
            if (rc != PPG_OK) return rc;
            // launch order: the chunks decoded whole first (longest first), then the materialised pieces
            const auto &X = sh->h_sidx;
            const size_t ns = X[go.size()];
            std::vector<uint32_t> order;
            for (size_t i = 0; i < go.size(); i++)
                if (!covered[i]) order.push_back(X[i]);
            std::stable_sort(order.begin(), order.end(),
                             [&](uint32_t a, uint32_t b) { return sh->h_sjobs[a].out_len > sh->h_sjobs[b].out_len; });
            const uint32_t ndec = (uint32_t)order.size();
            std::vector<PpgMatInfo> lmi;
            for (size_t i = 0; i < go.size(); i++) {
                if (!covered[i]) continue;
                if (X[i + 1] - X[i] != pmi[i].size()) return PPG_DATA_ERROR;   // side points and pieces disagree
                for (uint32_t j = X[i]; j < X[i + 1]; j++) {
                    order.push_back(j);
                    PpgMatInfo m = pmi[i][j - X[i]];
                    if (m.prev == 0x100u) m.prev = sh->h_sjobs[j].prev_byte;   // the chunk's first piece
                    lmi.push_back(m);
                }
            }
            std::vector<PpgInflateJob> lj(ns);
            std::vector<uint32_t> inv(ns);
            for (size_t q = 0; q < ns; q++) {
                lj[q] = sh->h_sjobs[order[q]];
                inv[order[q]] = (uint32_t)q;
            }
            HIPCHK(grow_buf(sh->ljobs, ns));   // (grow-only with headroom: a hipFree waits for the
            HIPCHK(grow_buf(sh->linv, ns));    // whole device, every other slot's launch included)
            HIPCHK(grow_buf(sl.fs.mi, lmi.size()));
            HIPCHK(hipMemcpyAsync(sh->ljobs.p, lj.data(), sizeof(PpgInflateJob) * ns, hipMemcpyHostToDevice, sl.s));
            HIPCHK(hipMemcpyAsync(sh->linv.p, inv.data(), 4 * ns, hipMemcpyHostToDevice, sl.s));
            HIPCHK(hipMemcpyAsync(sl.fs.mi.p, lmi.data(), sizeof(PpgMatInfo) * lmi.size(), hipMemcpyHostToDevice, sl.s));
            sh->lpt = true;
            sh->mat_first = ndec;
            sh->mat_n = (uint32_t)lmi.size();
            sh->mat_sym = sl.fs.sym.p;
            sh->mat_win = sl.fs.W.p;
            sh->mat_info = sl.fs.mi.p;
            HIPCHK(hipStreamSynchronize(sl.s));   // the host staging vectors die here
        }
        pc.mark("split");
    } else {   // side points of the chunks that have them (the index's, shifted into this launch); the
        // others' found on the GPU when the launch is too small to fill it
        std::vector<int64_t> sbit, sout;
        ByteVec swin;
        std::vector<FindChunk> find;
        const bool findable = !getenv("PPG_CHUNK_NO_FIND");
        for (size_t i = 0; i < go.size(); i++) {
            if (!go[i]->ix->side_out.empty()) {
                side_points_of(go[i]->ix, go[i]->k, sh->h_jobs[i].bit_start, sh->h_pout[i], sbit, sout, swin);
            } else if (findable && sh->h_jobs[i].out_len > 0) {
                // sorted by output with the others: flush the found ones in launch order
                find.push_back(find_chunk(i));
            }
            if (!find.empty() && (i + 1 == go.size() || !go[i + 1]->ix->side_out.empty())) {
                const size_t before = sbit.size();
                int64_t nsplit = 0;
                rc = find_side_points(sl.s, sl.fs, (const uint32_t *)sl.comp.p, sh->nwords, sh->dicts.p, find, sbit, sout, swin,
                                      nsplit, pc);
                if (rc != PPG_OK) return rc;
                svc.found_chunks += nsplit;
                svc.found_points += (int64_t)(sbit.size() - before);
                find.clear();
            }
        }
        pc.mark("find");
        if (!sbit.empty()) {
            rc = ppg_shard_set_split(sh, (int32_t)sbit.size(), sbit.data(), sout.data(), swin.data());
            if (rc != PPG_OK) return rc;
        }
        pc.mark("split");
    }
    shard_reset(sh);
    float total_ms = 0;
    rc = batch_launch(sh, 0, sh->n);
    if (rc == PPG_OK) rc = batch_collect(sh, 0, sh->n, total_ms);
    if (sh->mat_n) {   // the slot's shard is reused: the next launch sets its own split
        sh->mat_n = 0;
        sh->nsub = 0;
        sh->lpt = false;
    }
    if (rc != PPG_OK) return rc;
    pc.mark("decode");
    // shard_finish returns the first chunk's zlib status (each request gets its own below) or a
    // device failure, which fails every request of the launch
    if ((rc = shard_finish(sh, total_ms)) <= PPG_INDEX_OUT_OF_RANGE) return rc;
    // results: the whole output, then every descriptor, into the slot's pinned buffer
    const size_t out_bytes = (size_t)sh->h_pout[(size_t)sh->n];
    const size_t rec_bytes = 16 * (size_t)sh->total_records;
    const size_t rec_at = (out_bytes + 15) / 16 * 16;
    HIPCHK(grow_buf(sl.res, rec_at + rec_bytes + 16));
    if (out_bytes) HIPCHK(hipMemcpyAsync(sl.res.p, sh->out.p, out_bytes, hipMemcpyDeviceToHost, sl.s));
    if (rec_bytes) HIPCHK(hipMemcpyAsync(sl.res.p + rec_at, sh->recs.p, rec_bytes, hipMemcpyDeviceToHost, sl.s));
    HIPCHK(hipStreamSynchronize(sl.s));
    pc.mark("d2h");
    pc.dump(go.size(), (int)(&sl - svc.slot));
    for (size_t i = 0; i < go.size(); i++) {
        ChunkReq *r = go[i];
        const PpgInflateResult &res = sh->h_res[i];
        r->rc = res.status;
        r->got = (int64_t)res.produced;
        r->src = sl.res.p + sh->h_jobs[i].out_off;
        r->nrec = (int64_t)sh->h_info[i].records;
        r->src_recs = (const uint32_t *)(sl.res.p + rec_at) + 4 * sh->h_base[i];
    }
    return PPG_OK;
}

// a free slot (not decoding, nobody copying out of it), or -1
int free_slot(const ChunkService &svc) {
    for (int i = 0; i < kChunkSlots; i++)
        if (!svc.slot[i].busy && svc.slot[i].readers == 0) return i;
    return -1;
}

// the batching rule: a launch when nothing decodes, or a full enough queue beside a running one
bool may_lead(const ChunkService &svc) {
    return !svc.pending.empty() && (svc.in_flight == 0 || svc.pending.size() >= kMinSecond);
}

// async requests' results into the buffers given at submit, all at once (up to 8 threads); their
// wait() then only hands back the status and counts
int copy_async_results(const std::vector<ChunkReq *> &reqs) {
    try {
        std::vector<Span> cp;
        for (ChunkReq *r : reqs)
            r->fin_rc = result_spans(*r, r->out, r->out_cap, r->recs, r->rec_cap, r->fin_len, r->fin_nrec, cp);
        parallel_copy(cp, true);
    } catch (...) {
        return PPG_MEM_ERROR;
    }
    for (ChunkReq *r : reqs) r->copied = true;
    return PPG_OK;
}

// the copier thread (started by the first launch with async requests): drains the copy queue, then
// exits once the service stops
void copier_loop(ChunkService *svc) {
    std::unique_lock<std::mutex> lk(svc->mu);
    for (;;) {
        // (a launch still in flight may queue one more task: exit only after it)
        svc->cv.wait(lk, [&] { return !svc->copies.empty() || (svc->stop && svc->in_flight == 0); });
        if (svc->copies.empty()) return;
        ChunkService::CopyTask t = std::move(svc->copies.front());
        svc->copies.pop_front();
        lk.unlock();
        PhaseClock clk;
        const int rc = copy_async_results(t.reqs);
        if (clk.on) {
            int64_t b = 0;
            for (ChunkReq *r : t.reqs) b += r->fin_len + 16 * (r->recs ? r->nrec : 0);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - clk.t0).count();
            fprintf(stderr, "PPG_CHUNK copy of %zu: %.1f MB in %.3f ms (slot %d)\n", t.reqs.size(), b / 1e6, ms, t.slot);
        }
        lk.lock();
        for (ChunkReq *r : t.reqs) {
            if (rc != PPG_OK) r->rc = rc;
            r->done = true;
        }
        svc->slot[t.slot].readers--;
        svc->cv.notify_all();
    }
}

// Lead one launch of the queued requests on slot i (lk held on entry and on return, released
// while the launch runs).  Every request of the batch is marked done; a decoded one holds a reader
// on the slot until its results are copied out.
void lead(ppg_ctx *ctx, ChunkService &svc, std::unique_lock<std::mutex> &lk, int i) {
    const size_t nb = std::min(svc.pending.size(), kMaxBatch);
    std::vector<ChunkReq *> batch(svc.pending.begin(), svc.pending.begin() + (ptrdiff_t)nb);
    svc.pending.erase(svc.pending.begin(), svc.pending.begin() + (ptrdiff_t)nb);
    ChunkSlot &sl = svc.slot[i];
    sl.busy = true;
    svc.in_flight++;
    svc.launches++;
    svc.max_batch = std::max<int64_t>(svc.max_batch, (int64_t)batch.size());
    lk.unlock();
    int rc;
    try {
        rc = run_launch(ctx, svc, sl, batch);
    } catch (const std::bad_alloc &) {   // host vectors: never out through the C ABI, never a stuck slot
        rc = PPG_MEM_ERROR;
    } catch (...) {
        rc = PPG_DEVICE_ERROR;
    }
    lk.lock();
    // async requests go to the copier, which marks them done once their results are in the caller's
    // buffers (the copies of a 256-chunk launch take about as long as the launch: done here, they
    // kept the launcher from leading the next one)
    ChunkService::CopyTask task{i, {}};
    for (ChunkReq *r : batch) {
        if (rc != PPG_OK) r->rc = rc;
        if (r->rc == PPG_OK && r->async) {
            task.reqs.push_back(r);
            continue;
        }
        if (r->rc == PPG_OK) {
            r->slot = i;
            sl.readers++;
        }
        r->done = true;
    }
    if (!task.reqs.empty()) {
        bool queued = false;
        try {
            if (!svc.copier.joinable()) svc.copier = std::thread(copier_loop, &svc);
            svc.copies.push_back(std::move(task));
            sl.readers++;   // the copier's
            queued = true;
        } catch (...) {
        }
        if (!queued) {   // no copier: copy here, the lock released
            lk.unlock();
            const int crc = copy_async_results(task.reqs);
            lk.lock();
            for (ChunkReq *r : task.reqs) {
                if (crc != PPG_OK) r->rc = crc;
                r->done = true;
            }
        }
    }
    sl.busy = false;
    svc.in_flight--;
    svc.cv.notify_all();
}

// copy a done request's results out of its slot (callers copy in parallel), release the slot
int finish(ChunkService &svc, ChunkReq &req, uint8_t *out, int64_t out_cap, int64_t *produced, uint32_t *recs,
           int64_t rec_cap, int64_t *nrec) {
    if (req.copied) {   // an async request the launcher already copied out
        if (produced) *produced = req.fin_len;
        if (nrec && req.fin_nrec) *nrec = req.nrec;
        return req.fin_rc;
    }
    int rc = req.rc;
    if (rc == PPG_OK) {
        int64_t len = 0;
        bool with_nrec = false;
        std::vector<Span> cp;
        try {
            rc = result_spans(req, out, out_cap, recs, rec_cap, len, with_nrec, cp);
            parallel_copy(cp, true);
        } catch (...) {
            rc = PPG_MEM_ERROR;
        }
        if (produced) *produced = len;
        if (nrec && with_nrec) *nrec = req.nrec;
        std::lock_guard<std::mutex> lk(svc.mu);
        if (--svc.slot[req.slot].readers == 0) svc.cv.notify_all();
    }
    return rc;
}

// the launcher of asynchronous requests: whenever requests are queued and the batching rule allows,
// after letting a burst of submissions settle (a caller queueing hundreds of chunks gets them into
// one launch, not the first few into a launch of their own)
void worker_loop(ChunkService *svc) {
    using namespace std::chrono;
    std::unique_lock<std::mutex> lk(svc->mu);
    for (;;) {
        svc->cv.wait(lk, [&] { return svc->stop || (may_lead(*svc) && free_slot(*svc) >= 0); });
        if (svc->stop) return;
        while (svc->pending.size() < kMaxBatch && steady_clock::now() - svc->last_submit < microseconds(200))
            svc->cv.wait_for(lk, microseconds(100));
        const int i = free_slot(*svc);
        if (i < 0 || !may_lead(*svc)) continue;
        lead(svc->ctx, *svc, lk, i);
    }
}

}  // namespace

extern "C" {

// README "Decompress" (see the top of this file).  Safe to call from any number of host threads
// on one ctx at once.
int ppg_decompress_chunk(ppg_ctx *ctx, const ppg_index *ix, int32_t k, const uint8_t *slice, int64_t slice_len,
                         uint8_t *out, int64_t out_cap, int64_t *produced, uint32_t *recs, int64_t rec_cap,
                         int64_t *nrec) {
    if (!ctx || !ix || !slice || k < 0 || (size_t)k + 1 >= ix->pts.size() || !ctx->chunks) return PPG_ARG_ERROR;
    ChunkService *svc = ctx->chunks;
    ChunkReq req{ix, k, slice, slice_len};
    std::unique_lock<std::mutex> lk(svc->mu);
    svc->calls++;
    svc->pending.push_back(&req);
    svc->cv.notify_all();
    while (!req.done) {
        const int i = free_slot(*svc);
        if (i < 0 || !may_lead(*svc)) {
            svc->cv.wait(lk);
            continue;
        }
        // lead a launch of the queued requests (this one among them, unless another caller took it)
        lead(ctx, *svc, lk, i);
    }
    lk.unlock();
    return finish(*svc, req, out, out_cap, produced, recs, rec_cap, nrec);
}

int ppg_decompress_chunk_submit(ppg_ctx *ctx, const ppg_index *ix, int32_t k, const uint8_t *slice, int64_t slice_len,
                                uint8_t *out, int64_t out_cap, uint32_t *recs, int64_t rec_cap, ppg_chunk_req **req) {
    if (!ctx || !ix || !slice || !req || k < 0 || (size_t)k + 1 >= ix->pts.size() || !ctx->chunks) return PPG_ARG_ERROR;
    ChunkService *svc = ctx->chunks;
    auto *r = new (std::nothrow) ChunkReq{ix, k, slice, slice_len};
    if (!r) return PPG_MEM_ERROR;
    r->async = true;
    r->out = out;
    r->out_cap = out_cap;
    r->recs = recs;
    r->rec_cap = rec_cap;
    {
        std::lock_guard<std::mutex> lk(svc->mu);
        if (!svc->worker[0].joinable()) {
            svc->ctx = ctx;
            try {
                svc->worker[0] = std::thread(worker_loop, svc);
            } catch (...) {
                delete r;
                return PPG_MEM_ERROR;
            }
            for (int w = 1; w < kLaunchers; w++) {   // (more launchers are an optimisation only)
                try {
                    svc->worker[w] = std::thread(worker_loop, svc);
                } catch (...) {
                }
            }
        }
        svc->calls++;
        svc->pending.push_back(r);
        svc->last_submit = std::chrono::steady_clock::now();
    }
    svc->cv.notify_all();
    *req = (ppg_chunk_req *)r;
    return PPG_OK;
}

int ppg_decompress_chunk_wait(ppg_ctx *ctx, ppg_chunk_req *ticket, int64_t *produced, int64_t *nrec) {
    if (!ctx || !ticket || !ctx->chunks) return PPG_ARG_ERROR;
    ChunkService *svc = ctx->chunks;
    ChunkReq *r = (ChunkReq *)ticket;
    {
        std::unique_lock<std::mutex> lk(svc->mu);
        svc->cv.wait(lk, [&] { return r->done; });
    }
    const int rc = finish(*svc, *r, r->out, r->out_cap, produced, r->recs, r->rec_cap, nrec);
    delete r;
    return rc;
}

int ppg_decompress_chunk_stats(ppg_ctx *ctx, int64_t *calls, int64_t *launches, int64_t *max_batch) {
    if (!ctx || !ctx->chunks) return PPG_ARG_ERROR;
    std::lock_guard<std::mutex> lk(ctx->chunks->mu);
    if (calls) *calls = ctx->chunks->calls;
    if (launches) *launches = ctx->chunks->launches;
    if (max_batch) *max_batch = ctx->chunks->max_batch;
    return PPG_OK;
}

int ppg_decompress_chunk_split_stats(ppg_ctx *ctx, int64_t *chunks, int64_t *side_points) {
    if (!ctx || !ctx->chunks) return PPG_ARG_ERROR;
    if (chunks) *chunks = ctx->chunks->found_chunks.load();
    if (side_points) *side_points = ctx->chunks->found_points.load();
    return PPG_OK;
}

}  // extern "C"
