/*
 * ppgpu.h — C ABI of libppgpu.so, the MI355X (gfx950) replacement for the native layer under
 * Quantumzhao/ParallelParsing's chunked-gzip DecompressAll path.
 *
 * The reference reaches native code only through Interop/PlatformInterop.cs:6-35
 * ([DllImport("libz")] inflateInit2_/inflatePrime/inflateSetDictionary/inflate/inflateEnd/
 * inflateReset, driven by Decompressor/Core.cs).  This ABI replaces that layer one level up:
 * a C# host keeps Core/IndexIO/BatchedFASTQ's API surface and binds these entry points with a
 * [DllImport("ppgpu")] class of the same shape as LibZ (INTEGRATION.md shows the stub).
 *
 * Conventions (mirroring Interop/Conventions.cs):
 *  - every entry point returns an int status: PPG_OK (0) or a negative code; the ZResult values
 *    (Conventions.cs:9-20) keep their meaning, device failures get their own codes;
 *  - no exceptions cross the ABI; caller-owned buffers are pinned by the caller (as Core.cs:162,
 *    171 pins Memory<byte>) and never retained; library-owned objects have explicit _free/_close;
 *  - one ppg_ctx per GPU; a ctx is used by one host thread at a time (the reference's
 *    per-call ZStream, Core.cs:136, is likewise single-threaded) -- except ppg_decompress_chunk,
 *    the README's thread-safe "Decompress", which any number of threads may call on one ctx at
 *    once (alongside the one thread using the ctx's other entry points).
 */
#ifndef PPGPU_H
#define PPGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: ZResult (Interop/Conventions.cs:9-20) + library codes ---- */
#define PPG_OK 0
#define PPG_STREAM_END 1
#define PPG_NEED_DICT 2
#define PPG_ERRNO (-1)
#define PPG_STREAM_ERROR (-2)
#define PPG_DATA_ERROR (-3)
#define PPG_MEM_ERROR (-4)
#define PPG_BUF_ERROR (-5)
#define PPG_VERSION_ERROR (-6)
#define PPG_INDEX_OUT_OF_RANGE (-50) /* C# IndexOutOfRangeException (>32 KiB without '@') */
#define PPG_IO_ERROR (-51)
#define PPG_ARG_ERROR (-52)
#define PPG_UNSUPPORTED (-53)        /* input the GPU CreateIndex does not take (not single-member gzip) */
#define PPG_DEVICE_ERROR (-100)
#define PPG_NO_DEVICE (-101)

#define PPG_WINSIZE 32768 /* Common/Constants.cs:9  */
#define PPG_CHUNK 16384   /* Common/Constants.cs:12 */

/* ======================= Index (Common/Index.cs, Common/IndexIO.cs) ======================= */
typedef struct ppg_ctx ppg_ctx;       /* one GPU (see "device context" below) */
typedef struct ppg_index ppg_index;

/* CreateIndex: Core.BuildDeflateIndex(FileStream, uint chunksize) — Decompressor/Core.cs:14-131.
 * Host-side (serial zlib pass, as in the reference).  _mem takes the whole .gz in memory. */
int ppg_index_build_file(const char *gz_path, uint32_t chunksize, ppg_index **out);
int ppg_index_build_mem(const uint8_t *gz, int64_t gz_len, uint32_t chunksize, ppg_index **out);

/* CreateIndex on the GPU: the same Points as ppg_index_build_* (Core.BuildDeflateIndex,
 * Decompressor/Core.cs:14-131) from a block-parallel decode (ppg_index_gpu.cpp): candidate block
 * headers per piece of piece_bytes (0: automatic), a verified chain of block ends, exact output
 * per piece, then the '@' census.  gz: the whole single-member .gz, in host memory or (gz_on_device,
 * 4-byte aligned) in device memory.  out_capacity bounds the exact-output buffer (0: 96 GiB or free HBM less 4 GiB,
 * whichever is smaller; larger members are decoded in batches).
 * Returns PPG_UNSUPPORTED for zlib-wrapped / multi-member input (use ppg_index_build_file). */
int ppg_index_build_gpu(ppg_ctx *ctx, const void *gz, int64_t gz_len, int gz_on_device, uint32_t chunksize,
                        int64_t piece_bytes, int64_t out_capacity, ppg_index **out);

/* ppg_index_build_gpu that also records side points for ppg_shard_set_split: at every block end
 * at least side_bytes of output past the previous Point or side point (and not itself a Point),
 * its absolute bit, output offset and 32 KiB window, gathered on the GPU while the batch's output
 * is resident.  side_bytes <= 0: none.  Side points are not part of the .gzi (IndexIO). */
int ppg_index_build_gpu_side(ppg_ctx *ctx, const void *gz, int64_t gz_len, int gz_on_device, uint32_t chunksize,
                             int64_t piece_bytes, int64_t out_capacity, int64_t side_bytes, ppg_index **out);
int ppg_index_side_count(const ppg_index *ix);
/* copies the side points (any pointer may be NULL): count entries, windows count * 32768 bytes */
int ppg_index_side_points(const ppg_index *ix, int64_t *bit, int64_t *output, uint8_t *windows);
/* replaces the index's side points (a host that found inner block starts itself); sorted by output
 * and bit.  ppg_decompress_chunk splits every chunk at them (ppg_file_decompress_all and ppg_cursor
 * when a piece or batch is too small to fill the GPU). */
int ppg_index_set_side_points(ppg_index *ix, int32_t n, const int64_t *bit, const int64_t *output,
                              const uint8_t *windows);

int ppg_index_build_gpu_file(ppg_ctx *ctx, const char *gz_path, uint32_t chunksize, int64_t piece_bytes,
                             ppg_index **out);
/* Last GPU CreateIndex on ctx: [0] finder ms, [1] pass-1 ms, [2] chain check ms, [3] pass-2 ms,
 * [4] census + windows ms, [5] total ms, [6] pieces, [7] real pieces, [8] pass-1 redos,
 * [9] history resolve ms, [10] pass-2 batches, [11] blocks, [12] points, [13] output bytes,
 * [14] file upload ms (ppg_index_build_gpu_file), [15] pass-2 buffer allocation ms,
 * [16] speculative redos (false starts decoded again from their predecessor's end, one launch),
 * [17] serial redos (false starts the speculation missed).  n <= 18 values are written. */
int ppg_index_build_gpu_stats(ppg_ctx *ctx, double *vals, int32_t n);

/* Serialize / Deserialize — Common/IndexIO.cs:7-27 / :29-53 (byte-identical .gzi format). */
int ppg_index_serialize(const ppg_index *ix, const char *path);
int ppg_index_deserialize(const char *path, ppg_index **out);

/* Build an Index from caller arrays (the form a C# host holding an Index would pass; Point
 * fields of Common/Index.cs:51-82).  windows: count*32768 bytes; offsets concatenated with
 * offset_len[i] bytes each. */
int ppg_index_from_points(int32_t count, const int64_t *output, const int64_t *input, const int32_t *bits,
                          const uint8_t *windows, const int32_t *offset_len, const uint8_t *offsets,
                          int32_t chunk_max_bytes, ppg_index **out);

int32_t ppg_index_count(const ppg_index *ix);                 /* Index.Count (Index.cs:21) */
int32_t ppg_index_chunk_max_bytes(const ppg_index *ix);       /* Index.ChunkMaxBytes (Index.cs:10) */
int ppg_index_point(const ppg_index *ix, int32_t i, int64_t *output, int64_t *input, int32_t *bits,
                    int32_t *offset_len);                     /* Index[i] (Index.cs:20) */
const uint8_t *ppg_index_window(const ppg_index *ix, int32_t i);  /* Point.Window */
const uint8_t *ppg_index_offset(const ppg_index *ix, int32_t i);  /* Point.offset */
void ppg_index_free(ppg_index *ix);

/* Whether chunks [first, first+n) fit the decode kernels (checked by ppg_shard_create and every
 * decode entry point): PPG_OK; PPG_UNSUPPORTED for a chunk whose output (+ its offset carry) is
 * 2^31 bytes or more -- where the reference's (int)(to.Output - from.Output) (Core.cs:140) already
 * breaks -- or whose compressed span is 2^32 - 2^12 bits or more; PPG_ARG_ERROR for Points out of
 * order or a range outside the index.  Host-only; needs no device. */
int ppg_index_validate(const ppg_index *ix, int32_t first, int32_t n);

/* ================================= device context ================================= */

int ppg_device_count(int *n);
int ppg_open(int device, ppg_ctx **out);
void ppg_close(ppg_ctx *ctx);
void *ppg_ctx_stream(ppg_ctx *ctx); /* the hipStream_t every kernel of this ctx runs on */

/* Stream-ordered handoff between the ctx's stream and a caller's hipStream_t (torch's current
 * stream, a host's own), with no host synchronisation -- the device-side counterpart of the
 * reference's per-call ZStream ownership (Interop/Conventions.cs:43-127):
 *   ppg_ctx_wait_stream: work queued on the ctx from now on waits for everything already queued on
 *     `stream` (call it before a ppg call reads device memory that `stream` writes, or writes
 *     memory that `stream` may still read, e.g. a block a caching allocator recycled);
 *   ppg_stream_wait_ctx: work queued on `stream` from now on waits for everything already queued
 *     on the ctx.
 * Every ppg entry point that reads caller device memory (comp_on_device, gz_on_device) or writes it
 * (ppg_shard_keys, ppg_shard_counts_to_device, ppg_shard_copy_output) does so on the ctx's
 * stream, so one ppg_ctx_wait_stream before the call orders it after the caller's producers. */
int ppg_ctx_wait_stream(ppg_ctx *ctx, void *stream);
int ppg_stream_wait_ctx(ppg_ctx *ctx, void *stream);

/* ====================== Decompress one checkpoint (README "Decompress") ======================
 * Core.ExtractDeflateIndex(fileBuffer, from=Index[k], to=Index[k+1], buf) — Core.cs:133-192,
 * plus Parsing.Parse of offset_k ++ chunk (BatchedFASTQ.cs:67-68).  `slice` holds file bytes
 * [Index[k].Input-1, Index[k+1].Input-1] exactly as LazyFileReader reads them
 * (LazyFileReader.cs:63-69).  out receives to.Output-from.Output bytes; `produced` the count
 * (Core.cs:191).  If recs is non-NULL, up to rec_cap records are written as 4 uint32 newline
 * positions (n1..n4) relative to raw = offset_k ++ out; *nrec gets the record count.
 * Thread safe (README.md:38-50): concurrent calls on one ctx are combined into shared launches (four
 * launch slots, each with its own stream and buffers that only grow: no hipMalloc/hipFree per call
 * once warm; a second launch starts beside a decoding one only once 16 calls queue, so the queue
 * that builds up during a launch goes into the next one); every call gets its own chunk's results.
 * A chunk of an index with side points
 * (ppg_index_build_gpu_side) is decoded as one wave per piece; in a launch of at most 4,096 chunks,
 * a chunk of an index without them gets its inner block starts found on the GPU first (candidate
 * block headers, a speculative symbolic decode, the verified chain of block ends from the chunk's
 * Point and their resolved 32 KiB histories -- CreateIndex's own kernels) and is decoded as up to
 * 16 pieces too; in a launch of at most 256 such chunks the search's symbolic decode covers each
 * whole chunk and a chunk whose chain is verified end to end is written out from its symbols, with
 * no second decode.  Environment PPG_CHUNK_NO_FIND=1 turns the search off (PPG_CHUNK_NO_MAT=1 only
 * the write-out from symbols). */
int ppg_decompress_chunk(ppg_ctx *ctx, const ppg_index *ix, int32_t k, const uint8_t *slice, int64_t slice_len,
                         uint8_t *out, int64_t out_cap, int64_t *produced, uint32_t *recs, int64_t rec_cap,
                         int64_t *nrec);
/* The same, asynchronous: one caller keeps many chunks in flight, as the reference's reader keeps 32
 * partitions queued (LazyFileReader.cs:14) for its tasks.  submit queues the request and returns a
 * ticket at once; a launcher thread of the ctx (started by the first submit) combines the queued
 * requests -- a burst of submissions goes into one launch of up to 256 chunks --, a copier thread
 * copies each decoded chunk's bytes / records into the buffers given at submit (up to 8 threads per
 * launch) while the next launch runs, and ppg_decompress_chunk_wait blocks until that is done,
 * returns the status and counts, and frees the ticket (slice, out and recs must stay valid until
 * then).  Every ticket must be waited for, each once, on the ctx it was submitted to.  (Both forms:
 * where results of a launch are copied out together, the whole 2 MiB pages inside each caller
 * buffer get madvise(MADV_HUGEPAGE) first -- advice only, the copy is ~2x faster into fresh pages.) */
typedef struct ppg_chunk_req ppg_chunk_req;
int ppg_decompress_chunk_submit(ppg_ctx *ctx, const ppg_index *ix, int32_t k, const uint8_t *slice, int64_t slice_len,
                                uint8_t *out, int64_t out_cap, uint32_t *recs, int64_t rec_cap, ppg_chunk_req **req);
int ppg_decompress_chunk_wait(ppg_ctx *ctx, ppg_chunk_req *req, int64_t *produced, int64_t *nrec);
/* ppg_decompress_chunk (and _submit) calls on this ctx so far, the launches that served them, the
 * most calls one launch served. */
int ppg_decompress_chunk_stats(ppg_ctx *ctx, int64_t *calls, int64_t *launches, int64_t *max_batch);
/* Chunks split by the search for inner block starts above, and the side points it found. */
int ppg_decompress_chunk_split_stats(ppg_ctx *ctx, int64_t *chunks, int64_t *side_points);

/* ======================= DecompressAll over a shard (README "DecompressAll") =======================
 * A shard is chunks [first, first+n) of an index, with their compressed bytes resident on the
 * ctx's GPU: comp holds file bytes [Index[first].Input-1, Index[first+n].Input-1]
 * (comp_len = Index[first+n].Input - Index[first].Input + 1).  comp_on_device != 0 means comp
 * is already a device pointer on this GPU (4-byte aligned, readable 64 bytes past comp_len);
 * otherwise it is copied.  out_capacity bounds the device output buffer: chunks are decoded
 * in batches whose outputs fit, the buffer being reused (0 = whole shard at once).
 * A range that ends early is taken when it ends inside the last chunk's own bytes (at least 8 bytes
 * past Index[first+n-1].Input-1: a file that ends early): that chunk needs bits past the slice it was
 * handed and fails with PPG_DATA_ERROR (Core.cs:174), every other chunk is unaffected.  Any other
 * comp_len is PPG_ARG_ERROR.
 * A failed chunk (status != 0) has no records: it takes no record numbers, no units and no rows, the
 * chunks after it are numbered as if it were empty, and every record stage below counts 0 for it.
 * ppg_shard_run goes through every batch and every hook before it returns the first failed chunk's
 * status, so nothing a hook wrote counts as ready; the one-shot stage calls on a one-batch shard
 * work after such a run and see the good chunks' records alone. */
typedef struct ppg_shard ppg_shard;

int ppg_shard_create(ppg_ctx *ctx, const ppg_index *ix, int32_t first, int32_t n, const void *comp, int64_t comp_len,
                     int comp_on_device, int64_t out_capacity, ppg_shard **out);
void ppg_shard_free(ppg_shard *sh);

/* Inflate + parse every chunk of the shard (BatchedFASTQ's populateCache body, BatchedFASTQ.cs:
 * 63-74, for all chunks).  Returns 0, or the first chunk error (ZResult code).  Blocking. */
int ppg_shard_run(ppg_shard *sh);

/* Parallelism inside chunks (no reference counterpart: the reference decodes a chunk on one
 * thread, Core.cs:133-192; SURVEY §8f #1 "a denser side-index for sub-chunk parallelism").
 * nsub side points, sorted by output, each a deflate block start strictly inside one of the
 * shard's chunks: absolute file bit position (8*Input - Bits in Point terms), absolute output
 * offset, and the 32 KiB of output before it (host array, nsub * 32768 bytes).  Later runs decode
 * each chunk as one wave per piece between its Point, its side points and the next Point, and
 * fold the pieces back into the chunk (ppg_split_merge): results, records and bytes are
 * identical to the unsplit run.  A side point that is not where the previous piece's blocks end
 * fails the chunk with PPG_DATA_ERROR.  Works with any number of output batches (each batch
 * launches its chunks' pieces); nsub = 0 restores one wave per chunk. */
int ppg_shard_set_split(ppg_shard *sh, int32_t nsub, const int64_t *bit, const int64_t *output,
                        const uint8_t *windows);

/* Per-chunk results of the last run (host arrays of length n; any may be NULL). */
int ppg_shard_results(ppg_shard *sh, int64_t *records, int64_t *produced, int32_t *status, int32_t *flags,
                      int64_t *end_bit);
int64_t ppg_shard_total_records(ppg_shard *sh);
int32_t ppg_shard_batches(ppg_shard *sh);

/* Chunk bytes (only when the shard ran as one batch: the output buffer is reused by the next
 * batch; ppg_cursor streams bytes of any size) / record descriptors (any number of batches: the
 * descriptors of every batch stay resident) to the host.
 * Descriptor j of chunk k = 4 uint32 (n1,n2,n3,n4) relative to raw_k = offset_k ++ chunk_k:
 * Identifier=[r+1,n1) Sequence=[n1+1,n2) Other=[n2+2,n3) Quality=[n3+1,n4), where r = 0 for
 * the chunk's first record and the previous n4+1 otherwise (Parsing.cs:11-51). */
int ppg_shard_copy_chunk(ppg_shard *sh, int32_t k, uint8_t *dst, int64_t cap, int64_t *len);
int ppg_shard_copy_records(ppg_shard *sh, int32_t k, uint32_t *dst, int64_t cap, int64_t *nrec);
int ppg_shard_record_base(ppg_shard *sh, int64_t *base); /* n record bases (exclusive scan) */
/* Bytes [off, off+len) of a one-batch shard's decompressed output (off relative to
 * Index[first].Output; chunks are contiguous) into host memory or (dst_on_device) device memory
 * on this GPU, on the ctx stream. */
int ppg_shard_copy_output(ppg_shard *sh, int64_t off, int64_t len, void *dst, int dst_on_device);

/* Paired reads (the reference only names the goal, README.md:9): the spot number
 * of every record of a one-batch shard, in record order, into caller device memory (cap int64s):
 * the digits between the first two '.' of the Identifier ("SRR<id>.<spot>.<mate> ..."), -1 when
 * absent, -2 for a record the reference parses twice, which a pairing drops. */
int ppg_shard_keys(ppg_shard *sh, int64_t *dev_keys, int64_t cap);
/* The same keys for a shard of any number of batches: from the next ppg_shard_run on, each batch
 * writes its records' keys to dev_keys[shard record number] (caller device memory on this GPU, cap
 * entries) on the ctx stream while its output is resident.  NULL / 0 turns it off.  A run with
 * more records than cap fails with PPG_BUF_ERROR. */
int ppg_shard_set_keys(ppg_shard *sh, int64_t *dev_keys, int64_t cap);

/* Whether the last ppg_shard_run of the shard filled the ppg_shard_set_keys buffer (1) or not (0:
 * none attached, attached after that run, or the run failed). */
int ppg_shard_keys_ready(ppg_shard *sh);

/* ---- packed reads: 2-bit sequences, an N mask and qualities as a structure of arrays ----
 * What a read consumer (a k-mer counter, an aligner) builds from every FastqRecord.Sequence /
 * .Quality (Common/FastqRecord.cs; Parsing.cs:41-47 slices them), made on the GPU from the resident
 * output and descriptors.  Records are numbered as above (ppg_shard_record_base[k] + j); records
 * the reference parses twice (key -2) are included, a consumer drops them by their keys.
 * For record j with descriptor (n1,n2,n3,n4) relative to raw_k:
 *   L_j = n2 - n1 - 1   the Sequence slice [n1+1, n2) exactly (a CRLF file's '\r' is part of it);
 *   P_j = 32 * ceil(L_j / 32);  seq_off[0] = 0, seq_off[j+1] = seq_off[j] + P_j (int64, in bases);
 *   seq_len[j] = L_j (uint32).
 * Base i < L_j has position b = seq_off[j] + i and byte c = raw_k[n1+1+i]:
 *   bases  uint32 words of 16 bases: bits [2(b&15), 2(b&15)+2) of bases[b>>4] = A 0, C 1, G 2, T 3
 *          (upper case only; any other byte gives 0);
 *   mask   uint32 words of 32 bases: bit b&31 of mask[b>>5] = 1 iff c is none of ACGT;
 *   qual   bytes (optional): qual[b] = raw_k[n3+1+i] if n3+1+i < n4, else 0 -- the Quality string,
 *          cut or zero-filled to the sequence's length for a malformed record.
 * Positions L_j <= i < P_j are 0 in all planes, and every word / byte below seq_off[nrecords] is
 * written: the planes are a function of the text alone.  Every record starts on a 32-base unit
 * (8 B of bases, one mask word, 32 B of qual).  Derived from the formats, per 150 bp record:
 * 401 B of text + descriptors, ~232 B packed with qualities, ~72 B without.
 * Buffers are caller device memory on this GPU, written on the ctx stream: dev_seq_off rec_cap + 1
 * entries (8-byte aligned), dev_seq_len rec_cap, dev_bases base_cap / 16 words (8-byte aligned),
 * dev_mask base_cap / 32 words, dev_qual base_cap bytes (16-byte aligned) or NULL for no quality
 * plane; base_cap counts bases and is a multiple of 32.  PPG_BUF_ERROR when the records or the
 * padded bases exceed the caps: nothing is written then.  PPG_ARG_ERROR for a NULL shard, one that
 * has not run, a base_cap that is no multiple of 32, misaligned or missing planes.
 *  ppg_shard_seq_bases     after a run of any number of batches (the descriptors stay resident):
 *                          the sum of P_j and the record count -- the caps a pack needs.
 *  ppg_shard_pack_seq      a one-batch shard after its run, blocking like the keys call above
 *                          (PPG_ARG_ERROR on a multi-batch shard); *total_bases = seq_off[records].
 *  ppg_shard_set_seqpack   any number of batches: from the next run on every batch is packed while
 *                          its output is resident, record numbers and base offsets carried across
 *                          batches.  All pointers NULL and caps 0 turn it off.
 *  ppg_shard_seqpack_ready 1 when the last run filled the buffers (*total_bases: their padded
 *                          bases), else 0: none attached, attached after that run, or it failed
 *                          (PPG_ARG_ERROR, a negative value, for a NULL shard). */
int ppg_shard_seq_bases(ppg_shard *sh, int64_t *total_bases, int64_t *records);
int ppg_shard_pack_seq(ppg_shard *sh, int64_t *dev_seq_off, uint32_t *dev_seq_len, int64_t rec_cap,
                       uint32_t *dev_bases, uint32_t *dev_mask, uint8_t *dev_qual, int64_t base_cap,
                       int64_t *total_bases);
int ppg_shard_set_seqpack(ppg_shard *sh, int64_t *dev_seq_off, uint32_t *dev_seq_len, int64_t rec_cap,
                          uint32_t *dev_bases, uint32_t *dev_mask, uint8_t *dev_qual, int64_t base_cap);
int ppg_shard_seqpack_ready(ppg_shard *sh, int64_t *total_bases);

/* ---- sequence queries: pattern search and base census over every FastqRecord.Sequence ----
 * The reference's consumers beside Count(): RunPattern (Benchmark/Naive.cs: the records whose
 * Sequence.Contains(pattern)) and the base count of Decompressor/Program.cs:20-21
 * (Sequence.Count(c => c == 'A')), computed on the GPU from the resident output and descriptors; the
 * answers are a few integers and one bit per record, no text leaves the device.
 * For shard record j (numbered as above) with descriptor (n1,n2,n3,n4) relative to raw_k, S_j is the
 * Sequence slice raw_k[n1+1, n2) of length L_j = n2 - n1 - 1 (a CRLF file's '\r' is part of it;
 * records the reference parses twice, SURVEY Q1, count twice; a chunk whose status is not 0
 * contributes no hits and no bases).
 *   hit_j   1 iff the pattern occurs in S_j as a contiguous byte string (ordinal, case sensitive, as
 *           string.Contains on the ASCII decode), wholly inside S_j.  pattern_len m: 0 <= m <= 64,
 *           any byte but '\n'; m = 0 (or a NULL pattern) is a census alone and every record is a hit
 *           (Contains("") is true).  m > 64, m < 0 or a '\n' in the pattern: PPG_ARG_ERROR.
 *   census  count[0..3] bytes 'A' 'C' 'G' 'T' (upper case only) over all S_j, count[4] every other
 *           byte; bases = the sum of L_j = the sum of count.
 * dev_hit_mask (optional): caller device memory on this GPU, 4-byte aligned, written on the ctx stream;
 * bit j & 31 of word j >> 5 is hit_j.  rec_cap counts records and is a multiple of 32; every word
 * below ceil(records / 32) is written whole (bits at and past `records` are 0), no word at or past
 * rec_cap / 32 is written; records > rec_cap: PPG_BUF_ERROR, nothing written.  NULL with cap 0: no mask.
 * chunk_hits (optional): host int64[n], the hits per chunk of the shard.  `result` (optional) points
 * at a ppg_seq_query_result; it is spelled void * so that a binding passes its own struct's address.
 *  ppg_shard_query_seq       a one-batch shard after its run, blocking like ppg_shard_pack_seq
 *                            (PPG_ARG_ERROR for a NULL shard, one that has not run, a multi-batch
 *                            shard, a bad pattern, mask or cap).
 *  ppg_shard_set_seqquery    any number of batches: from the next run on every batch is scanned while
 *                            its output is resident, record numbers and totals carried across batches.
 *                            The pattern is copied at the call.  pattern NULL, pattern_len < 0, a NULL
 *                            mask and cap 0 together turn it off.  A run with more records than
 *                            rec_cap fails with PPG_BUF_ERROR.
 *  ppg_shard_seqquery_ready  1, and the outputs filled, when the last run completed the query; else 0:
 *                            none attached, attached after that run, or the run failed
 *                            (PPG_ARG_ERROR, a negative value, for a NULL shard). */
typedef struct {
    int64_t records;   /* records scanned */
    int64_t hits;      /* records whose Sequence contains the pattern */
    int64_t bases;     /* sum of L_j */
    int64_t count[5];  /* A, C, G, T, other */
} ppg_seq_query_result;
int ppg_shard_query_seq(ppg_shard *sh, const uint8_t *pattern, int32_t pattern_len, uint32_t *dev_hit_mask,
                        int64_t rec_cap, int64_t *chunk_hits, void *result);
int ppg_shard_set_seqquery(ppg_shard *sh, const uint8_t *pattern, int32_t pattern_len, uint32_t *dev_hit_mask,
                           int64_t rec_cap);
int ppg_shard_seqquery_ready(ppg_shard *sh, int64_t *chunk_hits, void *result);

/* ---- record selection: the records a mask selects, compacted on the GPU ----
 * The body of RunPattern's loop (Benchmark/Naive.cs:168-179: foreach record, if Sequence.Contains)
 * acts on the records that hit; a query above says which they are, this hands them over: the selected
 * records' text, back to back, made on the GPU while the text is resident, so that only they cross
 * the bus.  The mask is a query's hit mask or anything a consumer computed per record.
 * Shard record j (numbered as above) is record q of chunk k with descriptor (n1,n2,n3,n4) relative to
 * raw_k.  Its text is T_j = raw_k[a_j, e_j), a_j = 0 for q = 0 and (n4 of record q-1 of chunk k) + 1
 * otherwise, e_j = n4 + 1, len_j = e_j - a_j: the bytes ppg_pairs_emit_* define per record, from its
 * first byte through its quality line's '\n'.  A record the reference parses twice is
 * record 0 of the next chunk; its T_j lies wholly inside the offset carry.
 * Selected: bit j & 31 of dev_mask[j >> 5] (the hit-mask format), ANDed with "chunk k's status is 0"
 * (a failed chunk contributes nothing, as in a query).  A NULL mask with mask_cap 0 selects every
 * record.  Bits at and past `records` are ignored.  mask_cap counts records and is a multiple of 32,
 * else PPG_ARG_ERROR; records > mask_cap: PPG_BUF_ERROR.
 * Output, for the S selected records in ascending j (the i-th is j_i):
 *   recno[i] = j_i (int64);
 *   sel_off[0] = 0, sel_off[i+1] = sel_off[i] + len_{j_i} (int64: S + 1 entries, no 4 GiB limit);
 *   bytes[sel_off[i], sel_off[i+1]) = T_{j_i}, back to back, no padding;
 *   desc[4i .. 4i+3] = (n1 - a, n2 - a, n3 - a, n4 - a) (uint32), relative to the record's own first
 *   byte: the field slices of ppg_shard_copy_records apply with r = 0.
 * Nothing at or past sel_off[S] bytes or S records (S + 1 offsets) is written, and the output is a
 * function of the text and the mask alone.  Buffers are caller device memory on this GPU, written on
 * the ctx stream: dev_recno and dev_sel_off 8-byte aligned (sel_cap and sel_cap + 1 entries), dev_desc
 * and dev_bytes 16-byte aligned (4 * sel_cap words, byte_cap bytes).  When S exceeds sel_cap or
 * sel_off[S] exceeds byte_cap the call returns PPG_BUF_ERROR and nothing is written: the sizes are
 * checked before anything is moved.
 *  ppg_shard_select_size     after a run of any number of batches (the descriptors and statuses stay
 *                            resident): S and sel_off[S], the caps a selection needs.  Blocking.
 *  ppg_shard_select_records  a one-batch shard after its run, blocking like ppg_shard_query_seq;
 *                            *records = S, *bytes = sel_off[S] (also with PPG_BUF_ERROR).
 *                            PPG_ARG_ERROR for a NULL shard, one that has not run, a multi-batch
 *                            shard, a bad cap, a misaligned or missing buffer.
 *  ppg_shard_set_select      any number of batches: from the next run on every batch's selected records
 *                            are appended while its output is resident, recno, sel_off and the bytes
 *                            carried across batches.  It is the last of a batch's hooks: a
 *                            ppg_shard_set_seqquery hook that writes the same mask buffer has filled
 *                            this batch's bits before they are read.  A batch that would exceed a cap
 *                            fails the run with PPG_BUF_ERROR.  All pointers NULL and caps 0 turn it off.
 *  ppg_shard_select_ready    1, and S and sel_off[S] filled, when the last run completed the selection;
 *                            else 0: none attached, attached after that run, or the run failed
 *                            (PPG_ARG_ERROR, a negative value, for a NULL shard). */
int ppg_shard_select_size(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int64_t *records, int64_t *bytes);
int ppg_shard_select_records(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int64_t *dev_recno,
                             int64_t *dev_sel_off, uint32_t *dev_desc, int64_t sel_cap, uint8_t *dev_bytes,
                             int64_t byte_cap, int64_t *records, int64_t *bytes);
int ppg_shard_set_select(ppg_shard *sh, const uint32_t *dev_mask, int64_t mask_cap, int64_t *dev_recno,
                         int64_t *dev_sel_off, uint32_t *dev_desc, int64_t sel_cap, uint8_t *dev_bytes,
                         int64_t byte_cap);
int ppg_shard_select_ready(ppg_shard *sh, int64_t *records, int64_t *bytes);

/* ---- read filters: length, N content and quality per record, and the pass bit they give ----
 * The step a FASTQ consumer runs first is quality control: drop the reads that are too short, hold too
 * many N, have a low mean quality or too many low-quality bases.  The numbers come from the Sequence
 * and Quality slices alone, so they are made on the GPU while the text is resident; the pass bits are
 * a mask in the hit-mask format, which a selection above turns into the records themselves.
 * For shard record j (numbered as above) with descriptor (n1,n2,n3,n4) relative to raw_k:
 *   S_j      raw_k[n1+1, n2), L_j = n2 - n1 - 1: the Sequence slice of the packed reads and the queries
 *            (a CRLF file's '\r' is part of it);
 *   Q_j      raw_k[n3+1, n4), Lq_j = n4 - n3 - 1: the Quality slice itself, neither cut nor padded to L_j
 *            (the packed reads' qual plane is);
 *   other_j  the bytes of S_j that are none of 'A' 'C' 'G' 'T' (upper case): the popcount of the record's
 *            bits in the packed reads' mask plane; its sum over the records is a query's count[4];
 *   qsum_j   the sum of the bytes of Q_j as unsigned values, in 64 bits;
 *   low_j    the bytes of Q_j whose unsigned value is < qual_base + low_q.
 * A filter is a ppg_read_filter: eight int64_t, passed as const void * so that a binding passes its own
 * struct's address.  criteria is a set of bits: PPG_FILTER_LENGTH 1, PPG_FILTER_OTHER 2, PPG_FILTER_MEAN 4,
 * PPG_FILTER_LOW 8, PPG_FILTER_AND_MASK 0x100.  The criteria, in exact signed 64-bit integer arithmetic:
 *   LENGTH   min_len <= L_j and (max_len < 0 or L_j <= max_len);
 *   OTHER    other_j <= max_other;
 *   MEAN     1000 * (qsum_j - qual_base * Lq_j) >= min_mean_milli * Lq_j   (true when Lq_j = 0);
 *   LOW      1000 * low_j <= max_low_milli * Lq_j                          (true when Lq_j = 0).
 * pass_j = chunk k's status is 0 and every enabled criterion holds.  A failed chunk contributes no
 * passes, no bytes to the totals, and metrics rows of zeros, as in a query; records the reference
 * parses twice count twice.  With none of the four criteria every record of a decoded chunk
 * passes: metrics and totals alone.
 * ppg_read_filter_check is host only: PPG_ARG_ERROR for a NULL filter, unknown criteria bits,
 * min_len < 0, max_len < -1 or 0 <= max_len < min_len, OTHER with max_other < 0, qual_base outside
 * [0, 255], low_q < 0 or qual_base + low_q > 256, max_low_milli outside [0, 1000], |min_mean_milli| >
 * 255000; PPG_OK otherwise.  Every entry point below applies it.
 * dev_pass_mask (optional): the hit-mask format, 4-byte aligned, rec_cap a multiple of 32.  Without
 * AND_MASK it is written like a query's mask: every word below ceil(records / 32) whole, pad bits 0,
 * nothing at or past rec_cap / 32.  With AND_MASK a mask is required, bit j of records [0, records)
 * becomes old & pass_j and no other bit changes: one mask carries "pattern hit and passes" into a
 * selection.  dev_metrics (optional): 8-byte aligned, metrics_cap rows of 24 bytes, row j = uint32 L_j,
 * other_j, Lq_j, low_j, then uint64 qsum_j.  chunk_passed (optional): host int64[n], the passes per chunk.
 * `result` (optional) points at a ppg_read_filter_result: failed[c] counts the records of decoded chunks
 * that fail criterion c (LENGTH, OTHER, MEAN, LOW), each on its own, 0 for a disabled criterion;
 * qual_count[v] is the number of Quality bytes of value v, so the sum of v * qual_count[v] is the sum
 * of qsum_j.  records > rec_cap (with a mask) or > metrics_cap (with metrics): PPG_BUF_ERROR, nothing
 * written.  Every output is a function of the text and the filter alone.
 *  ppg_shard_filter_reads      a one-batch shard after its run, blocking; PPG_ARG_ERROR as for
 *                              ppg_shard_query_seq, for a bad filter, mask, metrics pointer or cap.
 *  ppg_shard_set_readfilter    any number of batches: from the next run on every batch is measured
 *                              while its output is resident, record numbers and totals carried across
 *                              batches.  The filter is copied at the call; a NULL filter turns it off.
 *                              A batch's hooks run in the order keys, pack, query, filter, trim, select (a
 *                              dedup hook, "read dedup" below, and a profile hook, "read profile" below,
 *                              in that order between trim and select): a filter
 *                              with AND_MASK on the query hook's mask sees this batch's hit bits, and
 *                              the select hook sees the product.  A run with more records than a cap
 *                              fails with PPG_BUF_ERROR.
 *  ppg_shard_readfilter_ready  as ppg_shard_seqquery_ready. */
typedef struct {
    int64_t criteria;        /* PPG_FILTER_* bits */
    int64_t min_len;
    int64_t max_len;         /* -1: no upper bound */
    int64_t max_other;
    int64_t qual_base;       /* the Quality byte of quality 0 (33 for Sanger / Illumina 1.8+) */
    int64_t min_mean_milli;  /* 1000 x the least mean quality */
    int64_t low_q;           /* a base is low when its quality is below this */
    int64_t max_low_milli;   /* 1000 x the largest fraction of low bases */
} ppg_read_filter;
typedef struct {
    int64_t records;         /* records measured */
    int64_t passed;
    int64_t failed[4];       /* LENGTH, OTHER, MEAN, LOW */
    int64_t bases;           /* sum of L_j */
    int64_t other;           /* sum of other_j */
    int64_t qual_bytes;      /* sum of Lq_j */
    int64_t qual_count[256];
} ppg_read_filter_result;
int ppg_read_filter_check(const void *filter);
int ppg_shard_filter_reads(ppg_shard *sh, const void *filter, uint32_t *dev_pass_mask, int64_t rec_cap,
                           void *dev_metrics, int64_t metrics_cap, int64_t *chunk_passed, void *result);
int ppg_shard_set_readfilter(ppg_shard *sh, const void *filter, uint32_t *dev_pass_mask, int64_t rec_cap,
                             void *dev_metrics, int64_t metrics_cap);
int ppg_shard_readfilter_ready(ppg_shard *sh, int64_t *chunk_passed, void *result);

/* ---- read trimming: the usable window of every record, and the keep bit it gives ----
 * Between "find the reads" and "drop what is too short" every FASTQ pipeline trims: it cuts low-quality
 * ends and the 3' adapter.  A trimmed read is a window (start, len) into the Sequence and Quality slices;
 * no text is rebuilt.  S_j, L_j, Q_j, Lq_j are those of "read filters" above.  The quality byte of base i
 * is qb(i) = Q_j[i] for i < Lq_j and 0 otherwise (the packed reads' zero-filled qual plane): a base
 * without a Quality byte is below every threshold above 0.
 * A trim is a ppg_read_trim: twelve int64_t and 64 adapter bytes, 160 bytes, passed as const void *.
 * ops is a set of bits: PPG_TRIM_LEADING 1, PPG_TRIM_TRAILING 2, PPG_TRIM_WINDOW 4, PPG_TRIM_ADAPTER 8,
 * PPG_TRIM_AND_MASK 0x100.  head, tail and min_len always apply (0: no effect).  In signed 64-bit integers:
 *   fixed     b0 = min(head, L_j), e0 = max(b0, L_j - tail).
 *   Every cut below is decided on [b0, e0) on its own: the cuts do not see each other's results, so all
 *   of them are one pass of min / max reductions.  This differs from tools that apply their steps one
 *   after another (a sliding window there sees the text an adapter cut has already shortened).
 *   LEADING   lead = the least i in [b0, e0) with qb(i) >= qual_base + lead_q; e0 when there is none.
 *             Off: b0.
 *   TRAILING  trail = 1 + the greatest i in [b0, e0) with qb(i) >= qual_base + trail_q; b0 when there is
 *             none.  Off: e0.
 *   WINDOW    W = win_size.  win = the least i with b0 <= i and i + W <= e0 whose full window has a mean
 *             below win_q: sum over t < W of qb(i + t) < W * (qual_base + win_q); e0 when no full window
 *             fails, which includes e0 - b0 < W.  Off: e0.
 *   ADAPTER   m = adapter_len, A = adapter[0, m).  For p in [b0, e0): ov(p) = min(m, e0 - p) and mis(p) =
 *             the number of t < ov(p) with S_j[p + t] != A[t], bytes compared as they are (an 'N' of the
 *             read is a mismatch).  adapt = the least p with ov(p) >= min_overlap and
 *             1000 * mis(p) <= max_err_milli * ov(p); e0 when there is none.  Off: e0.  Leftmost wins,
 *             no insertions or deletions: a 3' adapter that may be cut short by the end of the read.
 *   combine   b = max(b0, lead), e = min(trail, win, adapt), len_j = max(e - b, 0), start_j = b when
 *             len_j > 0 and 0 otherwise.
 * The trimmed read is S_j[start_j, start_j + len_j) with the quality Q_j[start_j, min(start_j + len_j, Lq_j)).
 * keep_j = chunk k's status is 0 and len_j >= min_len.  A failed chunk contributes rows of zeros, no
 * keeps and nothing to the totals; records the reference parses twice count twice, as in the
 * filters.
 * ppg_read_trim_check is host only: PPG_ARG_ERROR for a NULL trim, unknown ops bits, head, tail or
 * min_len < 0, qual_base outside [0, 255], an enabled lead_q / trail_q / win_q that is < 0 or has
 * qual_base + q > 256, WINDOW with win_size outside [1, 32], ADAPTER with adapter_len outside [1, 64], a
 * '\n' among the adapter's bytes, min_overlap outside [1, adapter_len] or max_err_milli outside
 * [0, 1000]; PPG_OK otherwise.  Every entry point below applies it.
 * dev_trim (optional): caller device memory, 8-byte aligned, trim_cap rows of two uint32: row j =
 * (start_j, len_j).  dev_keep_mask (optional): the hit-mask format under the rules of a filter's
 * dev_pass_mask: without AND_MASK every word below ceil(records / 32) is written whole, pad bits 0,
 * nothing at or past rec_cap / 32; with AND_MASK a mask is required, bit j becomes old & keep_j and no
 * other bit changes.  chunk_kept (optional): host int64[n].  `result` (optional) points at a
 * ppg_read_trim_result: trimmed counts the records of decoded chunks whose window is not (0, L_j); cut[c]
 * the records that the fixed cut (b0 > 0 or e0 < L_j), LEADING (lead > b0), TRAILING (trail < e0), WINDOW
 * (win < e0) and ADAPTER (adapt < e0) moved, each on its own.  records > rec_cap (with a mask) or >
 * trim_cap (with rows): PPG_BUF_ERROR, nothing written.  Every output is a function of the text and the
 * struct alone.
 *  ppg_shard_trim_reads      a one-batch shard after its run, blocking; PPG_ARG_ERROR as for
 *                            ppg_shard_filter_reads.
 *  ppg_shard_set_readtrim    the hook, as ppg_shard_set_readfilter: the struct is copied at the call, a
 *                            NULL trim turns it off.  A batch's hooks run in the order keys, pack, query,
 *                            filter, trim, dedup, profile, select: a trim with AND_MASK on the query's mask
 *                            gives the dedup, the profile and the selection "hit, passes, and still min_len
 *                            long after trimming".
 *  ppg_shard_readtrim_ready  as ppg_shard_readfilter_ready. */
typedef struct {
    int64_t ops;             /* PPG_TRIM_* bits */
    int64_t head;            /* bases cut from the 5' end */
    int64_t tail;            /* bases cut from the 3' end */
    int64_t qual_base;       /* the Quality byte of quality 0 (33 for Sanger / Illumina 1.8+) */
    int64_t lead_q;          /* LEADING: the first base of at least this quality starts the read */
    int64_t trail_q;         /* TRAILING: the last base of at least this quality ends it */
    int64_t win_size;        /* WINDOW: bases per window, 1 .. 32 */
    int64_t win_q;           /* ... whose mean quality must not fall below this */
    int64_t min_overlap;     /* ADAPTER: the least overlap that counts */
    int64_t max_err_milli;   /* ... and 1000 x the largest fraction of mismatches in it */
    int64_t min_len;         /* keep: the least trimmed length */
    int64_t adapter_len;
    uint8_t adapter[64];
} ppg_read_trim;
typedef struct {
    int64_t records;         /* records trimmed */
    int64_t kept;
    int64_t trimmed;         /* window != (0, L_j) */
    int64_t cut[5];          /* fixed, LEADING, TRAILING, WINDOW, ADAPTER */
    int64_t bases;           /* sum of L_j */
    int64_t bases_window;    /* sum of len_j */
    int64_t bases_kept;      /* sum of len_j over the kept records */
} ppg_read_trim_result;
int ppg_read_trim_check(const void *trim);
int ppg_shard_trim_reads(ppg_shard *sh, const void *trim, uint32_t *dev_keep_mask, int64_t rec_cap, void *dev_trim,
                         int64_t trim_cap, int64_t *chunk_kept, void *result);
int ppg_shard_set_readtrim(ppg_shard *sh, const void *trim, uint32_t *dev_keep_mask, int64_t rec_cap, void *dev_trim,
                           int64_t trim_cap);
int ppg_shard_readtrim_ready(ppg_shard *sh, int64_t *chunk_kept, void *result);

/* ---- read profile: bases and qualities per read position, lengths, GC and mean quality per read ----
 * The report of a QC tool: what the data looks like, and what it looks like after a filter and a trim.
 * It is made on the GPU while the text is resident; a table of max_pos rows and one fixed struct leave
 * the device.  S_j, L_j, Q_j, Lq_j are those of "read filters" above.
 * A profile is a ppg_read_profile: four int64_t, passed as const void *.  flags is a set of bits:
 * PPG_PROFILE_USE_MASK 1, PPG_PROFILE_USE_WINDOWS 2.  P = max_pos is the number of positions profiled.
 * The window (s_j, w_j) of record j: (0, L_j) without USE_WINDOWS; with it, from row j of dev_windows (a
 * trim's row format: two uint32 (start, len)), clamped: s_j = min(start, L_j), w_j = min(len, L_j - s_j).
 * No row makes a kernel read outside S_j.
 * profiled_j = chunk k's status is 0 and, with USE_MASK, bit j of dev_mask (the hit-mask format) is set.
 * The mask and the rows are only read.  A failed chunk contributes nothing; records the reference parses
 * twice count twice, as in the filters.  In exact integer arithmetic, for a profiled record:
 *   per position  p < min(w_j, P), i = s_j + p: the class of S_j[i] ('A' 'C' 'G' 'T' upper case, or other)
 *                 is counted in base[p]; if i < Lq_j the Quality byte c = Q_j[i] is counted: qual_n[p] += 1,
 *                 qual_sum[p] += c (the raw byte), qhist[p][b] += 1 with b = min(max(c - qual_base, 0), 63).
 *                 Quality bytes at i >= L_j belong to no base and are counted nowhere.
 *   per record    over the whole window, positions at and past P included: gc_j = its 'G' and 'C' bytes,
 *                 qn_j = the i in the window with i < Lq_j, qsum_j = the sum of those Quality bytes.
 * `table` (optional): host memory, table_cap rows of 72 int64_t (ppg_read_profile_row); the first P are
 * written.  len_here of row p counts the profiled records with w_j == p (row 0: the empty ones).
 * `result` (optional) points at a ppg_read_profile_result: records counts the records of decoded chunks;
 * longer the profiled records with w_j >= P, which no len_here counts; bases the sum of w_j,
 * bases_profiled of min(w_j, P), qual_bytes of qn_j; no_quality the profiled records with w_j > 0 and
 * qn_j == 0; gc_hist[100 * gc_j / w_j] counts the records with w_j > 0; meanq_hist counts those with
 * qn_j > 0 in bin 0 if qsum_j <= qual_base * qn_j, else min(63, (qsum_j - qual_base * qn_j) / qn_j).
 * chunk_profiled (optional): host int64[n], the profiled records per chunk.  Every output is a function
 * of the text, the struct, the mask and the rows alone.
 * ppg_read_profile_check is host only: PPG_ARG_ERROR for a NULL profile, unknown flag bits, qual_base
 * outside [0, 255], max_pos outside [1, PPG_PROFILE_MAX_POS], a reserved field that is not 0; PPG_OK
 * otherwise.  Every entry point below applies it.  PPG_ARG_ERROR as well for a flag without its buffer, a
 * buffer without its flag, a mask that is not 4-byte aligned, a mask_cap that is not a multiple of 32, rows
 * that are not 8-byte aligned.  records > mask_cap (with a mask) or > windows_cap (with rows), or a table
 * with table_cap < max_pos: PPG_BUF_ERROR, nothing written.
 *  ppg_shard_profile_reads      a one-batch shard after its run, blocking; PPG_ARG_ERROR as for
 *                               ppg_shard_trim_reads.
 *  ppg_shard_set_readprofile    the hook, as ppg_shard_set_readtrim: the struct is copied at the call, a
 *                               NULL profile turns it off; the accumulators are carried across a run's
 *                               batches and restart with its first.  A batch's hooks run in the order
 *                               keys, pack, query, filter, trim, profile, select (a dedup hook, "read
 *                               dedup" below, between trim and profile): the profile reads the mask as
 *                               those left it, so on the tensors that query, filter, trim and dedup write
 *                               with AND_MASK it describes exactly the reads the selection hands over.
 *  ppg_shard_readprofile_ready  as ppg_shard_readtrim_ready; the table of the hook's max_pos rows
 *                               (table_cap too small: PPG_BUF_ERROR, nothing written). */
enum { PPG_PROFILE_USE_MASK = 1, PPG_PROFILE_USE_WINDOWS = 2, PPG_PROFILE_MAX_POS = 1024 };
typedef struct {
    int64_t flags;           /* PPG_PROFILE_* bits */
    int64_t qual_base;       /* the Quality byte of quality 0 (33 for Sanger / Illumina 1.8+) */
    int64_t max_pos;         /* P: positions profiled, 1 .. PPG_PROFILE_MAX_POS */
    int64_t reserved;        /* 0 */
} ppg_read_profile;
typedef struct {
    int64_t base[5];         /* A, C, G, T, other */
    int64_t qual_n;
    int64_t qual_sum;
    int64_t len_here;        /* profiled records whose window is this long */
    int64_t qhist[64];
} ppg_read_profile_row;
typedef struct {
    int64_t records;         /* records of decoded chunks */
    int64_t profiled;
    int64_t longer;          /* w_j >= max_pos */
    int64_t bases;           /* sum of w_j */
    int64_t bases_profiled;  /* sum of min(w_j, max_pos) */
    int64_t qual_bytes;      /* sum of qn_j */
    int64_t no_quality;      /* w_j > 0 and qn_j == 0 */
    int64_t reserved;
    int64_t gc_hist[101];
    int64_t meanq_hist[64];
} ppg_read_profile_result;
int ppg_read_profile_check(const void *profile);
int ppg_shard_profile_reads(ppg_shard *sh, const void *profile, const uint32_t *dev_mask, int64_t mask_cap,
                            const void *dev_windows, int64_t windows_cap, int64_t *chunk_profiled, void *result,
                            int64_t *table, int64_t table_cap);
int ppg_shard_set_readprofile(ppg_shard *sh, const void *profile, const uint32_t *dev_mask, int64_t mask_cap,
                              const void *dev_windows, int64_t windows_cap);
int ppg_shard_readprofile_ready(ppg_shard *sh, int64_t *chunk_profiled, void *result, int64_t *table,
                                int64_t table_cap);

/* ---- read dedup: first occurrences by a 64-bit fingerprint, and the duplication levels ----
 * fastp's --dedup and FastQC's "Sequence Duplication Levels": the one step of a QC pipeline that needs
 * memory across reads.  Here that memory is a hash table in caller device memory that persists across the
 * batches of a run, so "has not been seen before" is one more bit in the mask that query, filter and trim
 * AND into, and the duplication report is one struct.  S_j, L_j, record numbering, failed chunks and
 * twice-parsed records (they count twice, so the second is a duplicate of the first) are as in
 * "read filters" above.
 * A dedup is a ppg_read_dedup: four int64_t, passed as const void *.  flags is a set of bits:
 * PPG_DEDUP_USE_WINDOWS 2, PPG_DEDUP_AND_MASK 0x100.
 * Key bytes D_j.  The window (s_j, w_j) of record j is the profile's: (0, L_j) without USE_WINDOWS; with it,
 * from row j of dev_windows (a trim's row format: two uint32 (start, len)), clamped: s_j = min(start, L_j),
 * w_j = min(len, L_j - s_j).  D_j = S_j[s_j, s_j + Ld_j) with Ld_j = w_j when max_bases == 0 and
 * min(w_j, max_bases) otherwise (max_bases = 50 is FastQC's rule).  No row makes a kernel read outside S_j;
 * the rows are only read.
 * Participation.  part_j = chunk k's status is 0 and, with AND_MASK, bit j of the mask is set.
 * Fingerprint.  64 bits, in exact unsigned arithmetic mod 2^64:
 *   unit i of D_j  the bytes D_j[32 i, 32 i + 32), zero-padded to 32, as four little-endian uint64 w_0 .. w_3;
 *   mix(x)         x ^= x >> 32; x *= 0xD6E8FEB86659FD93; x ^= x >> 32; x *= 0xD6E8FEB86659FD93; x ^= x >> 32;
 *   h_i            a = mix(0x9E3779B97F4A7C15 * (i + 1)), then a = mix(a ^ w_t) for t = 0, 1, 2, 3; h_i = a;
 *   G_j            the sum of h_i over i < ceil(Ld_j / 32) (0 when Ld_j = 0);
 *   F_j            mix(G_j ^ mix(Ld_j + 0x632BE59BD9B4E019)); an F_j of 0 becomes 1.
 * Two participating records are duplicates of each other if and only if their F is equal.  This is a
 * fingerprint dedup, like fastp's, not a byte compare: records with equal key bytes always have equal F, and
 * records with different key bytes have equal F with the probability of a 64-bit collision.  For N
 * participating records the chance of at least one false merge is about N^2 / 2^65: about 2e-7 at 2.88 M
 * records, about 4e-3 at 4e8.
 * The table.  dev_table is caller device memory, 8-byte aligned: `slots` rows of three uint64 {key, first,
 * count}; slots is a power of two, at least 64.  An empty row has key 0, first all ones, count 0.  The home
 * slot of F is (F * 0x9E3779B97F4A7C15) >> (64 - log2 slots), with linear probing and wrap.  After a run, for
 * every distinct F among the participants exactly one row has key = F, first = the lowest shard record number
 * with that F and count = the number of participants with it; every other row is empty.  Which row holds a
 * key is unspecified; the set of rows is a function of the text, the struct, the mask and the windows alone.
 * The run's first batch makes the whole table empty, and so does the one-shot call.
 * Capacity.  A batch that would bring 2 x (the records of the run so far, this batch included) above slots
 * fails with PPG_BUF_ERROR before the stage writes anything: the load never exceeds 1/2 and every probe ends
 * at an empty row.
 * Per-record outputs, final when the batch's hooks return (earlier batches hold the lower record numbers):
 * unique_j = part_j and first(F_j) == j.  dev_unique_mask: the hit-mask format, 4-byte aligned, mask_cap a
 * multiple of 32; optional without AND_MASK, and then written like a query's mask (every word below
 * ceil(records / 32) whole, pad bits 0, nothing at or past mask_cap / 32); with AND_MASK it is required, bit
 * j becomes old & unique_j and no other bit changes.  dev_first (optional): 8-byte aligned, first_cap rows of
 * one int64: the record number of the first occurrence of F_j (j itself when unique), -1 for a record that
 * does not participate.  chunk_unique (optional): host int64[n], the unique records per chunk.
 * `result` (optional) points at a ppg_read_dedup_result: records counts the records of decoded chunks; bases
 * the sum of Ld_j over the participants, bases_unique over the unique ones.  The levels are FastQC's bins of a
 * row's count: 1, 2, ..., 9, 10-49, 50-99, 100-499, 500-999, 1000-4999, 5000-9999, >= 10000.
 * level_distinct[b] counts the rows in bin b, level_reads[b] sums their counts: the sum of level_distinct is
 * unique, the sum of level_reads is participating.  max_count and max_first are the count and first of the
 * row with the greatest count, ties going to the lowest first; 0 and -1 for an empty table.  overflow counts
 * the inserts that found no row within slots probes: 0 under the capacity rule; it exists so that a broken
 * probe ends and shows.  The counters are carried across a run's batches; the levels and the greatest row are
 * made once, after the run's last batch.
 * ppg_read_dedup_check is host only: PPG_ARG_ERROR for a NULL dedup, unknown flag bits, max_bases < 0, a
 * reserved field that is not 0; PPG_OK otherwise.  Every entry point below applies it.  PPG_ARG_ERROR as well
 * for AND_MASK without a mask, USE_WINDOWS without windows, windows without USE_WINDOWS, a misaligned buffer,
 * a mask_cap that is not a multiple of 32, a cap without its buffer, slots that is not a power of two or is
 * below 64, a NULL table.  records > mask_cap (with a mask), > windows_cap (with windows), > first_cap (with
 * dev_first) or > slots / 2: PPG_BUF_ERROR, nothing written.
 *  ppg_shard_dedup_reads      a one-batch shard after its run, blocking; PPG_ARG_ERROR as for
 *                             ppg_shard_trim_reads.
 *  ppg_shard_set_readdedup    the hook, as ppg_shard_set_readtrim: the struct is copied at the call, a NULL
 *                             dedup turns it off; the table and the counters are carried across a run's
 *                             batches and restart with its first.  A batch's hooks run in the order keys,
 *                             pack, query, filter, trim, dedup, profile, select: the dedup sees what query,
 *                             filter and trim left of the mask, and the trim's windows; the profile and the
 *                             selection see only first occurrences.
 *  ppg_shard_readdedup_ready  as ppg_shard_readtrim_ready.
 * A rank of a multi-GPU job deduplicates its own share alone: its table sees no other rank's records. */
enum { PPG_DEDUP_USE_WINDOWS = 2, PPG_DEDUP_AND_MASK = 0x100 };
typedef struct {
    int64_t flags;           /* PPG_DEDUP_* bits */
    int64_t max_bases;       /* 0: the whole window; else the key is its first max_bases bases */
    int64_t reserved[2];     /* 0 */
} ppg_read_dedup;
typedef struct {
    int64_t records;         /* records of decoded chunks */
    int64_t participating;
    int64_t unique;          /* first occurrences: the rows of the table */
    int64_t bases;           /* sum of Ld_j over the participants */
    int64_t bases_unique;    /* ... over the unique records */
    int64_t overflow;        /* inserts that found no row: 0 */
    int64_t max_count;       /* the greatest count of a row */
    int64_t max_first;       /* ... and that row's first (ties: the lowest); -1 for an empty table */
    int64_t level_distinct[16];
    int64_t level_reads[16];
} ppg_read_dedup_result;
int ppg_read_dedup_check(const void *dedup);
int ppg_shard_dedup_reads(ppg_shard *sh, const void *dedup, uint32_t *dev_unique_mask, int64_t mask_cap,
                          const void *dev_windows, int64_t windows_cap, int64_t *dev_first, int64_t first_cap,
                          void *dev_table, int64_t slots, int64_t *chunk_unique, void *result);
int ppg_shard_set_readdedup(ppg_shard *sh, const void *dedup, uint32_t *dev_unique_mask, int64_t mask_cap,
                            const void *dev_windows, int64_t windows_cap, int64_t *dev_first, int64_t first_cap,
                            void *dev_table, int64_t slots);
int ppg_shard_readdedup_ready(ppg_shard *sh, int64_t *chunk_unique, void *result);

/* Device-resident per-chunk record counts (int64[n]) copied to caller device memory on this
 * GPU (the input of the cross-GPU all-gather). */
int ppg_shard_counts_to_device(ppg_shard *sh, int64_t *dev_dst);

/* Device time of the last run, from hipEvents on the ctx stream: inflate kernels only, parse
 * kernels only, and the whole run (ms). */
int ppg_shard_timing(ppg_shard *sh, float *inflate_ms, float *parse_ms, float *total_ms);

/* =============== DecompressAll from a .gz file: host ingest (LazyFileReader.cs:10-98) ===============
 * Streams chunks [first, first+n) of gz_path through the GPU: `threads` reader threads (0 = 8)
 * pread pieces of about piece_bytes compressed bytes (0 = 8 GiB: a launch needs thousands of
 * chunks to fill the GPU) into pinned host buffers; a copy stream moves each piece to HBM and a
 * helper thread prepares its jobs/windows while the previous piece decodes, so page cache, PCIe
 * and the kernels overlap.  Buffers persist in the ctx across calls.  records[i] (may be NULL) receives chunk first+i's record count,
 * *total_records their sum, *seconds the wall time from the first read to the last result.
 * Returns 0, PPG_IO_ERROR for an unreadable file, or the first chunk error (ZResult code). */
int ppg_file_decompress_all(ppg_ctx *ctx, const ppg_index *ix, const char *gz_path, int32_t first, int32_t n,
                            int64_t piece_bytes, int threads, int64_t *records, int64_t *total_records,
                            double *seconds);
/* Frees the buffers ppg_file_decompress_all keeps in the ctx (its device pieces and their shards'
 * outputs, tens of GB at 8 GiB pieces; the pinned staging; its streams) -- e.g. before other work
 * needs the HBM; the next call allocates them again.  Not while a ppg_file_decompress_all runs on
 * the ctx.  Returns 0, or PPG_ARG_ERROR for a NULL ctx. */
int ppg_file_release(ppg_ctx *ctx);

/* ======================= streamed records: BatchedFASTQ's enumerator =======================
 * Decompressor/BatchedFASTQ.cs:29-101 (IEnumerable<FastqRecord> over a bounded record cache fed by
 * LazyFileReader's partition queue, LazyFileReader.cs:41-97) over the GPU path, in bounded memory:
 * chunks [first, first+n) of gz_path in batches of whole chunks of at most batch_bytes of text
 * (0 = 1 GiB; a single larger chunk is its own batch).  Up to five batches are in flight, each in a
 * slot sized once at open for the largest batch: per slot ~1.13 x batch text + its compressed bytes
 * of pinned host memory and ~1.4-2.4 x that text of HBM (8 GiB batches: ~55 GB pinned in all); the
 * slot count drops (to 2 at least) where that would exceed half the available host memory or 80%
 * of the free HBM.  Each batch is pread (`threads` readers)
 * into pinned memory, decoded on the GPU and handed back as host memory: the chunks' raw bytes
 * raw_k = offset_k ++ chunk_k (Parsing.cs's CombinedMemory) concatenated in `text` at raw_off[k],
 * and the records of chunk k as desc[4*j .. 4*j+3] for j in [rec_off[k], rec_off[k+1]), each the
 * newline positions (n1,n2,n3,n4) relative to raw_k with the field slices of ppg_shard_copy_records.
 * While the caller walks batch k the library reads and decodes batch k+1; a batch is valid until
 * the next ppg_cursor_next (a FastqRecord is invalid after the next MoveNext, BatchedFASTQ.cs:56).
 * Order is canonical (chunk by chunk), not the reference's interleaving. */
typedef struct ppg_cursor ppg_cursor;
typedef struct {
    int32_t first_chunk;      /* index chunk of the batch's first chunk */
    int32_t nchunks;
    int64_t record_base;      /* records handed out by this cursor before this batch */
    int64_t nrecords;
    const uint8_t *text;      /* raw_k at text + raw_off[k] */
    const int64_t *raw_off;   /* nchunks + 1 entries */
    const uint32_t *desc;     /* 4 per record */
    const int64_t *rec_off;   /* nchunks + 1 entries */
} ppg_batch;

int ppg_cursor_open(ppg_ctx *ctx, const ppg_index *ix, const char *gz_path, int32_t first, int32_t n,
                    int64_t batch_bytes, int threads, ppg_cursor **out);
/* PPG_OK with the next batch in *b, PPG_STREAM_END after the last one, or a ZResult error. */
int ppg_cursor_next(ppg_cursor *c, ppg_batch *b);
int32_t ppg_cursor_batches(const ppg_cursor *c);
void ppg_cursor_close(ppg_cursor *c);

/* The packed enumerator: as ppg_cursor_open, but a batch carries packed reads (the format of
 * "packed reads" above, seq_off batch-relative from 0) instead of text + descriptors, so ~232 B
 * (planes bit 0 = 1: with qualities) or ~72 B (planes = 0) per 150 bp record cross PCIe instead of
 * 401 B.  In a ppg_batch of such a cursor text and desc are NULL; first_chunk, nchunks, record_base,
 * nrecords, raw_off and rec_off are filled as for a text cursor.
 *  ppg_cursor_packed          the current batch's planes in pinned host memory (valid until the
 *                             next ppg_cursor_next; any pointer may be NULL; *qual = NULL without
 *                             the quality plane) and its padded bases;
 *  ppg_cursor_packed_offsets  its nrecords + 1 offsets copied to the caller (cap entries;
 *                             PPG_BUF_ERROR when fewer).
 * Both return PPG_ARG_ERROR on a text cursor and before the first ppg_cursor_next. */
int ppg_cursor_open_packed(ppg_ctx *ctx, const ppg_index *ix, const char *gz_path, int32_t first, int32_t n,
                           int64_t batch_bytes, int threads, int32_t planes, ppg_cursor **out);
int ppg_cursor_packed(const ppg_cursor *c, uint32_t **bases, uint32_t **mask, uint8_t **qual, uint32_t **seq_len,
                      int64_t *total_bases);
int ppg_cursor_packed_offsets(const ppg_cursor *c, int64_t *seq_off, int64_t cap);

/* The filtered enumerator: as ppg_cursor_open, but every batch is queried for the pattern (the rules
 * of ppg_shard_set_seqquery: 0 <= pattern_len <= 64, no '\n'; 0 or a NULL pattern selects every
 * record), its hits are selected on the device ("record selection" above) and only the selection is
 * copied to pinned host memory: host memory and PCIe traffic follow what is selected, not the batch.
 * In a ppg_batch of such a cursor text and desc are NULL; nrecords counts the records scanned, and
 * first_chunk, nchunks, record_base, raw_off and rec_off are filled as for a text cursor.
 *  ppg_cursor_selected        the current batch's selected text and descriptors in pinned host memory
 *                             (valid until the next ppg_cursor_next; any pointer may be NULL), the
 *                             number of selected records and of their bytes;
 *  ppg_cursor_selected_index  its records + 1 offsets (batch-relative, from 0) and its `records` record
 *                             numbers copied to the caller (either may be NULL; cap counts records:
 *                             PPG_BUF_ERROR when cap < records).  A record number counts among the
 *                             records this cursor hands out: record_base + its number in the batch.
 * Both return PPG_ARG_ERROR on other cursors and before the first ppg_cursor_next. */
int ppg_cursor_open_select(ppg_ctx *ctx, const ppg_index *ix, const char *gz_path, int32_t first, int32_t n,
                           int64_t batch_bytes, int threads, const uint8_t *pattern, int32_t pattern_len,
                           ppg_cursor **out);
int ppg_cursor_selected(const ppg_cursor *c, uint8_t **bytes, uint32_t **desc, int64_t *records, int64_t *nbytes);
int ppg_cursor_selected_index(const ppg_cursor *c, int64_t *sel_off, int64_t *recno, int64_t cap);

/* The quality-controlled enumerator: the filtered enumerator whose selection is "hit and pass": every
 * batch is queried for the pattern, the hits that fail the filter ("read filters" above) are cleared
 * from the mask on the device, and what remains is selected.  A NULL filter is exactly
 * ppg_cursor_open_select; a NULL pattern or length 0 makes every record a hit, so the filter alone
 * selects.  The filter is copied at the call and its AND_MASK bit is ignored; a bad one is
 * PPG_ARG_ERROR.  ppg_cursor_selected and ppg_cursor_selected_index apply unchanged.
 *  ppg_cursor_filter_result  the current batch's ppg_read_filter_result, over all its records, hits or
 *                            not, copied to `result`; PPG_ARG_ERROR on other cursors and before the
 *                            first ppg_cursor_next. */
int ppg_cursor_open_filter(ppg_ctx *ctx, const ppg_index *ix, const char *gz_path, int32_t first, int32_t n,
                           int64_t batch_bytes, int threads, const uint8_t *pattern, int32_t pattern_len,
                           const void *filter, ppg_cursor **out);
int ppg_cursor_filter_result(const ppg_cursor *c, void *result);

/* ... and trimmed: the selection is "hit, pass and keep" ("read trimming" above), and every selected
 * record comes with its window.  A NULL trim is exactly ppg_cursor_open_filter (whose filter may be
 * NULL as well); the trim is copied at the call and its AND_MASK bit is ignored; a bad one is PPG_ARG_ERROR.
 *  ppg_cursor_selected_trim  the (start, len) rows of the current batch's selected records, in their
 *                            order, two uint32 each, in pinned host memory that stays valid until the
 *                            next ppg_cursor_next.
 *  ppg_cursor_trim_result    the current batch's ppg_read_trim_result, over all its records.
 * Both are PPG_ARG_ERROR on other cursors and before the first ppg_cursor_next. */
int ppg_cursor_open_trim(ppg_ctx *ctx, const ppg_index *ix, const char *gz_path, int32_t first, int32_t n,
                         int64_t batch_bytes, int threads, const uint8_t *pattern, int32_t pattern_len,
                         const void *filter, const void *trim, ppg_cursor **out);
int ppg_cursor_selected_trim(const ppg_cursor *c, uint32_t **trim);
int ppg_cursor_trim_result(const ppg_cursor *c, void *result);

/* ======================= multi-GPU DecompressAll (one process per GPU) =======================
 * BatchedFASTQ's fan-out (BatchedFASTQ.cs:62-77: a task per chunk) becomes a fan-out over GPUs:
 * rank r decodes the contiguous chunk range [bounds[r], bounds[r+1]) that ppg_partition balances
 * by compressed bytes, with no exchange on the data path; the one collective is an all-gather of
 * per-chunk record counts (padded to the widest range: RCCL has no all-gatherv) followed by an
 * exclusive scan, giving every chunk its global record number.
 *
 * A ppg_comm is an RCCL communicator (ncclAllGather on the ctx stream, over xGMI) -- made by the
 * library from a unique id that rank 0 creates and the host hands to every rank (ppg_comm_init),
 * or wrapping the caller's ncclComm_t (ppg_comm_from_rccl) -- or a host shared-memory transport
 * between processes of one machine (ppg_comm_init_host; name = "/something", unique per job):
 * RCCL refuses two ranks on one GPU, so that is how the N > 1 path is rehearsed on one GPU.
 * librccl is loaded at run time (dlopen librccl.so.1: the copy already in the process, if any).
 * A rank that fails still joins the gather, and every rank then returns the first failing
 * rank's status, so an error never leaves the others waiting. */
typedef struct ppg_comm ppg_comm;
#define PPG_COMM_ID_BYTES 128
int ppg_comm_unique_id(uint8_t *id);   /* PPG_COMM_ID_BYTES bytes (ncclGetUniqueId) */
int ppg_comm_init(ppg_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t *id, ppg_comm **out);
int ppg_comm_from_rccl(ppg_ctx *ctx, void *nccl_comm, int32_t nranks, int32_t rank, ppg_comm **out);
int ppg_comm_init_host(int32_t nranks, int32_t rank, const char *name, ppg_comm **out);
int ppg_comm_rank(const ppg_comm *c, int32_t *rank, int32_t *nranks);
void ppg_comm_free(ppg_comm *c);
int ppg_rccl_version(int *version);    /* ncclGetVersion of the librccl in use */

/* All-to-all-v of int64 values: counts[src * nranks + dst] values go from rank src to rank dst
 * (the whole matrix, the same on every rank); send holds this rank's outgoing values by
 * destination, recv receives by source, both in rank order.  RCCL: device buffers on the comm's GPU
 * (on_device = 1; grouped ncclSend / ncclRecv over xGMI); host transport: host or device buffers,
 * moved through shared memory in rounds.  The exchange step of ppg_pairs_check. */
int ppg_comm_alltoallv(ppg_comm *c, const int64_t *send, int64_t *recv, const int64_t *counts, int on_device);

/* bounds[0..nranks]: rank r owns chunks [bounds[r], bounds[r+1]) of [first, first+n) */
int ppg_partition(const ppg_index *ix, int32_t first, int32_t n, int32_t nranks, int32_t *bounds);
/* After ppg_shard_run of this rank's shard (chunks [bounds[rank], bounds[rank+1])): the count
 * all-gather + scan.  counts / bases (may be NULL): bounds[nranks] - bounds[0] entries. */
int ppg_shard_gather_counts(ppg_shard *sh, ppg_comm *comm, const int32_t *bounds, int64_t *counts, int64_t *bases,
                            int64_t *total_records);
/* The whole path for a C# host's BatchedFASTQ.Count() over N GPUs: partition the index's chunks,
 * pread this rank's compressed range from gz_path, decode it (out_capacity as ppg_shard_create),
 * gather.  counts / bases (may be NULL): Count-1 entries in canonical order. */
int ppg_dist_decompress_all(ppg_ctx *ctx, ppg_comm *comm, const ppg_index *ix, const char *gz_path,
                            int64_t out_capacity, int64_t *counts, int64_t *bases, int64_t *total_records);

/* ============ paired reads: R1 / R2 shards checked record by record ============
 * The reference only names the goal (README.md:9).  Pair number i = the i-th record of R1 and of
 * R2 after dropping the records the reference parses twice (key -2); a pair is good when
 * both spot keys (ppg_shard_keys) are present and equal.  ppg_pairs_check runs on the device: the
 * shards' keys (their ppg_shard_set_keys buffers when the last run filled them, else extracted now
 * from one-batch shards), the duplicates dropped through a map, the keys compared.  With a comm
 * (N ranks; rank r holds R1 and R2 shards of its own contiguous chunk ranges, which do not line up
 * between the files) pairs are owned evenly by pair number and every key moves to its owner: a
 * status + count all-gather, one all-to-all-v per file (RCCL ncclSend / ncclRecv, or the host
 * transport), the compare, a result all-gather; every rank gets the same result and a failing rank
 * never leaves the others waiting.  Both shards (and an RCCL comm) must be on one GPU.  A ppg_pairs
 * keeps its device scratch across checks. */
typedef struct {
    int64_t pairs;            /* min of the two files' records after dropping duplicates */
    int64_t records[2];       /* R1 / R2 records after dropping duplicates (all ranks) */
    int64_t duplicates[2];    /* Q1 duplicates dropped (this rank) */
    int64_t mismatches;       /* pairs whose keys differ or are missing (< 0), + |records[0] - records[1]| */
    int64_t first_bad;        /* the first such pair number, or -1 */
    int64_t first_keys[2];    /* its R1 / R2 spot keys (-1 when a file has no such record) */
} ppg_pair_result;
typedef struct ppg_pairs ppg_pairs;
int ppg_pairs_create(ppg_pairs **out);
int ppg_pairs_check(ppg_pairs *p, ppg_shard *r1, ppg_shard *r2, ppg_comm *comm, ppg_pair_result *result);
/* After a check: the shard record numbers (this rank's shard of `file`, 0 = R1) of pair numbers
 * [lo, hi), -1 for pairs whose record another rank holds -- record-aligned pair chunks are pair
 * numbers [j*K, (j+1)*K); the records themselves via ppg_shard_record_base / ppg_shard_copy_records. */
int ppg_pairs_records(const ppg_pairs *p, int32_t file, int64_t lo, int64_t hi, int64_t *shard_record);
void ppg_pairs_free(ppg_pairs *p);

/* ---- record-aligned pair chunks (BASELINE configs[4]: "chunk=50 000, record-aligned
 * pair chunks"; the reference's goal, README.md:9) ----
 * After ppg_pairs_check: pair chunk j = pairs [j*K, min((j+1)*K, pairs)).  Each half (file 0 = R1,
 * 1 = R2) is packed contiguously on the device: its records' bytes back to back -- each record from
 * its '@' to its quality line's '\n', the FastqRecord copy of Parsing.cs:41-47 -- and one 16-B
 * descriptor (n1, n2, n3, n4: the record's newline positions) per record, relative to the half's
 * first byte: the layout of one chunk's raw text + descriptors, so the same record reader applies
 * (record i starts at n4[i-1] + 1, record 0 at 0).
 *  ppg_pairs_emit_begin  the plan for this rank's pair chunks, on the shards and comm of the check.
 *      One rank: every pair chunk, in windows of at most window_bytes per half-file (0: 8 GiB; one
 *      pair chunk at least).  Multi-batch shards (configs[4]'s 2 x 25 GB on one GPU) have their
 *      batches run again as the windows advance -- both files' together, each on its own stream --
 *      and a pair chunk that straddles a batch boundary is carried across; nothing else may run the
 *      shards until the emission is done.  N ranks: rank r owns the pair chunks that start in its
 *      R1 range; the shards must be one-batch (resident; else PPG_UNSUPPORTED).
 *      The batches run again run none of the shard's hooks: neither ppg_shard_set_keys nor a record
 *      stage (ppg_shard_set_seqpack, _seqquery, _readfilter, _readtrim, _readdedup, _readprofile,
 *      _select).  From the check on -- after every window, after an emission that is stopped early,
 *      after the last window and through any further emission on the same check -- every attached
 *      stage's *_ready answer, its result struct, its per-chunk counts and every caller buffer it
 *      wrote (mask, windows rows, metrics, first rows, table, packed planes, selected records) are
 *      bit for bit what the shard's own ppg_shard_run left.
 *  ppg_pairs_emit_run    one rank, no check first: the emission drives the shards' own run.  Both
 *      shards carry a keys buffer (ppg_shard_set_keys); their batches run once each, in order, as
 *      the windows advance -- each batch's records numbered (its Q1 duplicates found from its keys)
 *      and packed while it is resident, so a multi-batch shard is decoded once, not twice.  After
 *      the last window (PPG_STREAM_END) both shards stand as ppg_shard_run leaves them and
 *      ppg_pairs_check follows (it may report mismatches the windows already emitted).  A caller
 *      that stops early leaves the shards unrun.
 *      The emission is the shards' run for their record stages too: every attached stage runs once
 *      per batch, in hook order.  From the call until the last window every stage is unready (its
 *      *_ready answer is 0), one that an earlier ppg_shard_run left ready included; after
 *      PPG_STREAM_END every attached stage is ready, with the results and buffers ppg_shard_run
 *      leaves on the same shard.  A caller that stops early, or a run that fails, leaves every stage
 *      unready.
 *  ppg_pairs_emit_next   packs the next window of this rank's pair chunks [*j0, *j1) on the device;
 *      PPG_STREAM_END when there is none.  N ranks: the first call is collective (every rank calls
 *      it: the records a rank does not hold move from their ranks over ppg_comm_alltoallv -- RCCL
 *      ncclSend / ncclRecv over xGMI, or the host transport) and is the rank's one window.
 *      A half's descriptors are 32-bit positions, so a half of 4 GiB or more (pair_chunk of ~11 M
 *      150 bp records) is PPG_UNSUPPORTED, before anything of it is packed (N ranks: agreed in the
 *      exchange's status gather, or after the exchange).  PPG_DATA_ERROR if the shards' batches cannot
 *      complete a pair chunk (never expected: the emission ends instead of looping).
 *  ppg_pairs_chunk       device pointers of a half of the current window (valid until the next call).
 *  ppg_pairs_copy_chunk  a half into caller memory (bytes and/or descriptors; NULL skips).
 *  ppg_pairs_emit_stats  [0] ms (re-)running batches, [1] ms packing, [2] ms exchanging, [3] ms in
 *      emit_next, [4] batches re-run, [5] pair chunks in all, [6..7] this rank's [j_lo, j_hi)
 *      (N ranks: after the exchange; emit_run: [5] and [7] once the last window is out). */
int ppg_pairs_emit_begin(ppg_pairs *p, ppg_shard *r1, ppg_shard *r2, ppg_comm *comm, int64_t pair_chunk,
                         int64_t window_bytes);
int ppg_pairs_emit_run(ppg_pairs *p, ppg_shard *r1, ppg_shard *r2, int64_t pair_chunk, int64_t window_bytes);
int ppg_pairs_emit_next(ppg_pairs *p, int64_t *j0, int64_t *j1);
int ppg_pairs_chunk(ppg_pairs *p, int64_t j, int32_t file, const uint8_t **bytes, int64_t *len, const uint32_t **desc,
                    int64_t *nrec);
int ppg_pairs_copy_chunk(ppg_pairs *p, int64_t j, int32_t file, uint8_t *dst, int64_t cap, int64_t *len, uint32_t *desc,
                         int64_t desc_cap, int64_t *nrec);
int ppg_pairs_emit_stats(const ppg_pairs *p, double *vals, int32_t n);

/* ---- pair overlap: the insert size of every pair, and the 3' cut of both mates that it gives ----
 * The defining step of fastp on pairs: read 1 is aligned against the reverse complement of read 2 without
 * insertions or deletions.  The alignment gives the fragment's insert size and the insert-size
 * distribution; when the fragment is shorter than a read it gives the exact 3' cut of both mates, which is
 * adapter trimming without knowing the adapter ("read trimming" above needs its bytes).  It works on two
 * packed read sets ("packed reads" above; without qualities ~72 B per 150 bp record, so both files stay
 * resident when their texts cannot), and its cut is the trim's row format: the dedup and profile hooks of
 * each file's shard take it as it is.
 * Inputs.  Set 1 and set 2 are packed read sets, each passed as a ppg_packed_view of device pointers (below);
 * qual may be NULL and is not read.  Pair i < npairs is record rec1[i] of set 1 and record rec2[i] of set 2;
 * dev_rec1 / dev_rec2 are optional device int64 arrays, 8-byte aligned.  NULL is the identity map; npairs
 * must then not exceed that set's records (PPG_ARG_ERROR).  An entry < 0 or >= the set's records makes the
 * pair unmapped (ppg_pairs_records gives -1 for another rank's record); no entry makes a kernel read outside
 * the planes.  A map must not name a record twice: that record's windows row is unspecified then.
 * Parameters.  A ppg_pair_overlap: eight int64_t, 64 bytes, passed as const void *.  flags 0; min_overlap
 * >= 1; max_diff >= 0; max_err_milli 0 .. 1000; reserved 0.  ppg_pair_overlap_check is host only:
 * PPG_ARG_ERROR for a NULL struct or a field outside these ranges, PPG_OK otherwise; every entry point
 * applies it.  fastp's values are min_overlap 30, max_diff 5, max_err_milli 200.
 * Alignment, in signed 64-bit integers.  L1 and L2 are the two reads' seq_len.  A pair with L1 or L2 above
 * PPG_OVERLAP_MAX_LEN = 1024 is long and is not analysed.  Otherwise c1(i) is the 2-bit code of base i of
 * read 1 and n1(i) its mask bit, c2 and n2 those of read 2.  The reverse complement R of read 2 has
 *   cR(t) = 3 - c2(L2 - 1 - t),  nR(t) = n2(L2 - 1 - t).
 * For an integer d with -L2 < d < L1, read-1 position i faces R position i - d.  The overlap is the i in
 * [max(0, d), min(L1, L2 + d)) and ov(d) its length.  mis(d) counts the i of the overlap where n1(i) or
 * nR(i - d) is set or c1(i) != cR(i - d): an N on either side is a mismatch, as in the trim.  d is accepted
 * when ov(d) >= min_overlap, mis(d) <= max_diff and 1000 * mis(d) <= max_err_milli * ov(d).  The candidates
 * are tried in the order d = 0, 1, ..., L1 - 1, -1, -2, ..., -(L2 - 1) -- fastp's: no adapter first, the
 * longest overlap first -- and the first accepted one wins.  A pair with an accepted d is found; its insert
 * size is I = L2 + d >= 1.
 * Outputs, all optional, each a function of the planes, the maps, the struct and the rows before alone.
 *   dev_rows        device memory, 16-byte aligned, row_cap rows of four int32: row i = (d, ov(d), mis(d), I)
 *                   for a found pair and (0, 0, 0, 0) for every other; all npairs rows are written.
 *   dev_found_mask  the hit-mask format, indexed by pair: every word below ceil(npairs / 32) is written
 *                   whole, pad bits 0, nothing at or past mask_cap / 32.
 *   dev_windows1, dev_windows2  the trim's row format (two uint32 (start, len), 8-byte aligned, win_cap1 /
 *                   win_cap2 rows), indexed by the record number in their set, so each file's shard hooks
 *                   read them directly.  Read, clipped and written for the two records of a found pair
 *                   only: with the row (s, n) and that read's length L, s' = min(s, L), n' = min(n, L - s'),
 *                   e = min(s' + n', I); the new row is (s', e - s') if e > s', else (0, 0).  No other row
 *                   changes.  A caller without a trim starts from rows (0, seq_len).
 *   result          a host ppg_pair_overlap_result, declared below.
 *   hist            host int64, hist_cap >= PPG_OVERLAP_HIST = 2048 bins: hist[I] counts the found pairs;
 *                   the first 2048 bins are written.
 * PPG_BUF_ERROR, nothing written: npairs above row_cap (with rows) or mask_cap (with a mask), a set's records
 * above its win_cap (with that plane), hist_cap below 2048 (with hist).  PPG_ARG_ERROR: a NULL ctx, view or
 * view plane other than qual, a negative count or cap, a misaligned pointer, a mask_cap that is no multiple of
 * 32.  The call runs on the ctx stream and blocks, like the other one-shot calls; the caller orders the
 * producers of the planes before it with ppg_ctx_wait_stream. */
enum { PPG_OVERLAP_MAX_LEN = 1024, PPG_OVERLAP_HIST = 2048 };
typedef struct {
    const int64_t *seq_off;  /* records + 1 entries */
    const uint32_t *seq_len;
    const uint32_t *bases;
    const uint32_t *mask;
    const uint8_t *qual;     /* the overlap: may be NULL, not read; the merge: required */
    int64_t records;
} ppg_packed_view;
typedef struct {
    int64_t flags;           /* 0 */
    int64_t min_overlap;     /* the least overlap that counts */
    int64_t max_diff;        /* the most mismatches in it */
    int64_t max_err_milli;   /* ... and 1000 x their largest fraction */
    int64_t reserved[4];     /* 0 */
} ppg_pair_overlap;
typedef struct {
    int64_t pairs;           /* pairs given */
    int64_t unmapped;
    int64_t too_long;        /* long pairs */
    int64_t analysed;
    int64_t found;
    int64_t negative;        /* found with d < 0 */
    int64_t adapter;         /* found with I < L1 or I < L2 */
    int64_t overlap_bases;   /* sum of ov over the found pairs */
    int64_t mismatches;      /* sum of mis */
    int64_t clipped[2];      /* sum over the found pairs of max(L - I, 0), per mate */
    int64_t reserved[5];
} ppg_pair_overlap_result;
int ppg_pair_overlap_check(const void *overlap);
int ppg_pairs_overlap(ppg_ctx *ctx, const void *overlap, const void *set1, const void *set2, const int64_t *dev_rec1,
                      const int64_t *dev_rec2, int64_t npairs, void *dev_rows, int64_t row_cap,
                      uint32_t *dev_found_mask, int64_t mask_cap, void *dev_windows1, int64_t win_cap1,
                      void *dev_windows2, int64_t win_cap2, void *result, int64_t *hist, int64_t hist_cap);

/* ---- pair merge: one consensus read per overlapping pair, as a third packed read set ----
 * What fastp --merge / --correction, PEAR and FLASH make of the overlap: the fragment's bases once, every
 * base that both mates cover decided by the better of the two observations.  The result is a packed read set
 * ("packed reads" above), so it feeds everything that takes one, a second pair overlap among them; no read
 * text leaves the device.
 * Inputs.  Set 1 and set 2 as ppg_packed_view, and the maps dev_rec1 / dev_rec2, exactly as in "pair overlap"
 * (NULL is the identity and npairs must then not exceed that set's records; an entry outside the set makes the
 * pair unmapped; no entry makes a kernel read outside the planes).  Both qual planes are required here and
 * 16-byte aligned (ppg_pairs_merge_size does not read them and takes NULL).  dev_rows: device memory, 16-byte
 * aligned, row_cap >= npairs rows of four int32 in the overlap's row format (d, ov, mis, I); normally the
 * overlap wrote them, a caller may zero a row to leave that pair out.  ov and mis are not read, and d and I are
 * trusted for nothing: a row that does not fit its pair is counted and skipped.
 * Parameters.  A ppg_pair_merge: eight int64_t, 64 bytes, passed as const void *.  flags 0; qual_hi and
 * qual_lo are quality bytes as they stand in the file (no offset is subtracted), 0 <= qual_lo < qual_hi <= 255;
 * reserved 0.  They only decide what is counted as corrected, never a base.  ppg_pair_merge_check is host
 * only: PPG_ARG_ERROR for a NULL struct or a field outside these ranges, PPG_OK otherwise; both other entry
 * points that take the struct apply it.  The Python layer's defaults are qual_hi 63 and qual_lo 47 ('?' and
 * '/': phred 30 and 14 at offset 33); they are defined by these values, not by another tool's behaviour.
 * Which pairs merge, in signed 64-bit integers.  Pair i has the lengths L1, L2 of the overlap and the row
 * (d, ., ., I).  It is, the first that applies:
 *   unmapped   as in the overlap;
 *   too_long   L1 or L2 above PPG_OVERLAP_MAX_LEN;
 *   unmerged   I == 0;
 *   stale      I != 0 but not (-L2 < d < L1 and I == L2 + d);
 *   merged     otherwise; then 1 <= I <= 2047.
 * The merged read has M = I bases; position p in [0, I) is a read-1 coordinate.  With c, n the 2-bit code and
 * the mask bit of the packed format and q the byte of the set's qual plane:
 *   side 1 covers p iff p < L1 and gives (c1(p), n1(p), q1(p));
 *   side R covers p iff p >= d and gives, with t = p - d, (3 - c2(L2-1-t), n2(L2-1-t), q2(L2-1-t)).
 * Every p is covered (a gap would need L1 <= p < d, but d < L1).  A p one side covers takes that side.  A p both
 * cover takes side R iff (n1 and not nR) or (n1 == nR and qR > q1), else side 1: a base beats an N, then the
 * higher quality byte wins, a tie goes to read 1 -- whether the two bases agree or not.  The output's mask bit
 * at p is the taken side's n, its code the taken side's code or 0 if that n is set, its qual byte the taken
 * side's q.  Bases of either mate outside [0, I) are read-through and are dropped (the overlap's clip).
 * Output.  The merged pairs in pair order, compacted: merged record m is the m-th merged pair.  Caller device
 * memory with the pointers, alignments and caps of ppg_shard_pack_seq: dev_seq_off (rec_cap + 1 entries),
 * dev_seq_len, dev_bases, dev_mask, dev_qual (NULL for no quality plane; the choice uses the input qualities
 * all the same), base_cap a multiple of 32; and dev_pair_of, optional, int64 [rec_cap], 8-byte aligned: the pair
 * index of each merged record.  seq_off[0] = 0, seq_off[m+1] = seq_off[m] + 32 * ceil(M_m / 32); positions
 * M <= i < P are 0 in all planes, every word / byte below seq_off[merged] is written and nothing at or past the
 * caps; entries of seq_len and pair_of from `merged` on are not written.  The planes are a function of the
 * inputs alone.
 * Result.  A host ppg_pair_merge_result, declared below, 16 int64_t.  Over the positions both sides cover
 * (overlap_bases): disagree counts those with both n clear and different codes, n_filled those with exactly
 * one n set, n_both those with both; the rest agree (overlap_bases - disagree - n_filled - n_both; not
 * stored).  Among the disagreements: from2 took side R, ties have qR == q1, corrected[0] took side R with
 * qR >= qual_hi and q1 <= qual_lo (read 1 overruled), corrected[1] took side 1 with q1 >= qual_hi and
 * qR <= qual_lo.  With rows exactly as the overlap wrote them, overlap_bases is the overlap's and
 * disagree + n_filled + n_both its mismatches.
 *  ppg_pair_merge_check   above.
 *  ppg_pairs_merge_size   *merged and *padded_bases = seq_off[merged]: the caps a merge needs.
 *  ppg_pairs_merge        sizes first; PPG_BUF_ERROR, nothing written, when npairs > row_cap, merged > rec_cap
 *                         or padded_bases > base_cap.  npairs == 0 and "nothing merged" are PPG_OK with
 *                         seq_off[0] = 0 written.
 * PPG_ARG_ERROR: a NULL ctx, view, view plane (qual as said), rows (with npairs > 0) or output plane other than
 * dev_qual and dev_pair_of, a negative count or cap, a misaligned pointer, a base_cap that is no multiple of 32.
 * An output plane of capacity 0 holds nothing and may be NULL: dev_seq_len with rec_cap 0, dev_bases and dev_mask
 * with base_cap 0 (dev_seq_off always has its entry 0), so a caller that sized a merge of nothing need not
 * invent addresses.
 * The calls run on the ctx stream and block, like the other one-shot calls; the caller orders the producers of
 * the planes and rows before them with ppg_ctx_wait_stream.  The rows are read twice, once to size and once to
 * place: the sets, the maps and the rows must not change while a call runs, or the caps that were checked are
 * not the caps that are used. */
typedef struct {
    int64_t flags;           /* 0 */
    int64_t qual_hi;         /* corrected: the taken side's quality byte is at least this ... */
    int64_t qual_lo;         /* ... and the other side's at most this */
    int64_t reserved[5];     /* 0 */
} ppg_pair_merge;
typedef struct {
    int64_t pairs;           /* pairs given */
    int64_t unmapped;
    int64_t too_long;
    int64_t unmerged;        /* I == 0 */
    int64_t stale;           /* a row that does not fit its pair */
    int64_t merged;
    int64_t merged_bases;    /* sum of M */
    int64_t padded_bases;    /* seq_off[merged] */
    int64_t overlap_bases;   /* positions both sides cover */
    int64_t disagree;        /* both bases, different codes */
    int64_t from2;           /* ... where side R was taken */
    int64_t ties;            /* ... where qR == q1 */
    int64_t n_filled;        /* exactly one side N */
    int64_t n_both;
    int64_t corrected[2];    /* read 1 overruled, read 2 overruled */
} ppg_pair_merge_result;
int ppg_pair_merge_check(const void *merge);
int ppg_pairs_merge_size(ppg_ctx *ctx, const void *set1, const void *set2, const int64_t *dev_rec1,
                         const int64_t *dev_rec2, int64_t npairs, const void *dev_rows, int64_t row_cap,
                         int64_t *merged, int64_t *padded_bases);
int ppg_pairs_merge(ppg_ctx *ctx, const void *merge, const void *set1, const void *set2, const int64_t *dev_rec1,
                    const int64_t *dev_rec2, int64_t npairs, const void *dev_rows, int64_t row_cap,
                    int64_t *dev_seq_off, uint32_t *dev_seq_len, int64_t rec_cap, uint32_t *dev_bases,
                    uint32_t *dev_mask, uint8_t *dev_qual, int64_t base_cap, int64_t *dev_pair_of, void *result);

/* ---- k-mer counts: the k-mer spectrum and the most frequent k-mers of a packed read set ----
 * The one report of a QC tool that looks across reads below the read: FastQC's "Kmer Content" and
 * "Overrepresented sequences", and the spectrum Jellyfish or KMC computes first for genome size, coverage, error
 * rate and contamination.  It works on one packed read set ("packed reads" above), so a k-mer is a shift and a
 * mask of resident words, and chains with the record stages through their mask and windows.  The reference has
 * nothing of the kind; the semantics are this library's, in exact integers.
 * Parameters.  A ppg_kmer_count: eight int64_t, 64 bytes, passed as const void *.  1 <= k <= 31; flags a
 * combination of PPG_KMER_CANONICAL, PPG_KMER_USE_WINDOWS, PPG_KMER_USE_MASK, PPG_KMER_ACCUMULATE; reserved 0.
 * ppg_kmer_count_check is host only: PPG_ARG_ERROR for a NULL struct, unknown flag bits, k out of range or a
 * non-zero reserved field, PPG_OK otherwise; every entry point that takes the struct applies it.
 * Input.  The set as a ppg_packed_view, declared in "pair overlap" above: qual may be NULL and is not read; fewer
 * than 2^32 - 1 records.  dev_mask: the hit-mask format indexed by record, mask_cap a multiple of 32; required with
 * USE_MASK and NULL without it.  dev_windows: the trim's row format, windows_cap rows, 8-byte aligned; required
 * with USE_WINDOWS and NULL without it.  A record participates when its mask bit is set or USE_MASK is off.  The
 * window (s, w) of a record of length L is (0, L) without USE_WINDOWS; with it the row (start, len) is clamped as
 * in the profile: s = min(start, L), w = min(len, L - s).  No row makes a kernel read outside the record's planes.
 * Both inputs are only read.
 * K-mers.  For a participating record every start p with s <= p and p + k <= s + w is a position.  A position is
 * valid when none of the mask-plane bits of bases p .. p + k - 1 is set: N, lower case and a CRLF file's '\r'
 * break k-mers, as they are mismatches elsewhere.  The key of the word x_0 .. x_{k-1} with 2-bit codes c_i is
 *   K(x) = sum of c_i * 4^(k - 1 - i):
 * the first base is most significant, so unsigned order is lexicographic order with A < C < G < T.  With
 * CANONICAL the key is min(K(x), K(revcomp x)), where revcomp x has the codes 3 - c_{k-1-i}.  A key never equals
 * the empty marker below: k <= 31 leaves the top two bits clear.
 * Table.  dev_table: caller device memory, 16-byte aligned, `slots` rows of two uint64 {key, count}; slots a
 * power of two, at least 64.  An empty row is {~0, 0}.  The home of a key is mix(key) >> (64 - log2 slots) with
 * the mix of "read dedup" above; probing is linear with wrap, so a consumer can probe the table itself.  Without
 * ACCUMULATE the call first makes the whole table empty; with it the call adds to what an earlier call with the
 * same k and CANONICAL bit left there (the caller guarantees that they match).  After a call that returns PPG_OK
 * every distinct key ever inserted has exactly one row, which holds the number of valid positions with that
 * key, and every other row is empty.  Which row holds a key is unspecified; the set of rows is a function of the
 * inputs alone.
 * Capacity.  PPG_OK requires that the occupied rows after the call are at most slots / 2.  Otherwise the call
 * returns PPG_BUF_ERROR; the table's contents are then unspecified, and nothing outside it is written (result
 * and spectrum included).  Nobody knows the distinct count in advance, so an undersized table is a normal call
 * and fails fast: a device counter of claimed rows stops the inserts once it passes slots / 2, and every probe
 * is bounded by `slots` steps.  A failing call costs about what a succeeding one costs; a caller sizes by
 * doubling.
 * Outputs, both optional and host memory.
 *   result    a ppg_kmer_count_result, declared below: sixteen int64_t.
 *   spectrum  int64, spectrum_cap >= PPG_KMER_SPECTRUM = 1024 entries, else PPG_BUF_ERROR before anything runs;
 *             the first 1024 are written.  spectrum[0] = 0; spectrum[c] = the rows with count c for 1 <= c <=
 *             1022; spectrum[1023] = the rows with count >= 1023.  It is made over the table after the call, so
 *             it sums to `distinct`.
 *  ppg_kmer_count_check  above.
 *  ppg_kmers_count    the count, the totals and the spectrum.
 *  ppg_kmers_select   the rows with count >= min_count (min_count >= 1, else PPG_ARG_ERROR) into dev_out: device
 *                     memory, 16-byte aligned, out_cap rows of 16 bytes, in unspecified order; *found (optional)
 *                     is their exact number.  When found > out_cap the call returns PPG_BUF_ERROR with *found
 *                     set, the first out_cap rows unspecified and nothing past them written.  dev_out NULL with
 *                     out_cap 0 only counts and returns PPG_OK.
 *  ppg_kmers_lookup   dev_counts[i] (device int64, 8-byte aligned) = the count of dev_keys[i] (device uint64,
 *                     8-byte aligned) as given -- a key is not canonicalised, that is the caller's job -- and
 *                     0 for a key the table does not hold, ~0 among them.
 * PPG_ARG_ERROR: a NULL ctx, view, view plane other than qual, or table; a negative count or cap; a misaligned
 * pointer; a mask_cap that is no multiple of 32; slots not a power of two or below 64; a flag without its buffer
 * or a buffer without its flag; a seq_off[records] that is negative or no multiple of 32.  PPG_BUF_ERROR: more
 * records than mask_cap or windows_cap, a spectrum_cap below 1024.  Nothing is written on either.  The calls run
 * on the ctx stream and block, like the other one-shot calls; the caller orders the producers of the planes, the
 * mask and the windows before them with ppg_ctx_wait_stream.
 * Not built: k > 31 (a key of more than one word); minimizer or super-k-mer partitioning; counts across ranks (a
 * rank's table sees its own share); a per-batch shard hook or a cursor (a multi-batch shard leaves its whole
 * packed set resident through ppg_shard_set_seqpack, which is what the Python layer counts); quality-aware
 * k-mers; writing the table to a Jellyfish or KMC file. */
enum { PPG_KMER_CANONICAL = 1, PPG_KMER_USE_WINDOWS = 2, PPG_KMER_USE_MASK = 4, PPG_KMER_ACCUMULATE = 8 };
enum { PPG_KMER_SPECTRUM = 1024 };
typedef struct {
    int64_t flags;           /* PPG_KMER_* */
    int64_t k;               /* 1 .. 31 */
    int64_t reserved[6];     /* 0 */
} ppg_kmer_count;
typedef struct {
    /* of this call */
    int64_t records;         /* the set's records */
    int64_t participating;
    int64_t short_reads;     /* participants with w < k */
    int64_t bases;           /* sum of w over the participants */
    int64_t positions;
    int64_t kmers;           /* the valid positions */
    int64_t invalid;         /* positions - kmers */
    /* of the table after the call */
    int64_t distinct;        /* occupied rows */
    int64_t singletons;      /* rows with count 1 */
    int64_t max_count;
    int64_t max_key;         /* the lowest key among the rows of max_count; -1 for an empty table */
    int64_t total_count;     /* the sum of all counts */
    int64_t overflow;        /* inserts given up; 0 on PPG_OK */
    int64_t reserved[3];
} ppg_kmer_count_result;
int ppg_kmer_count_check(const void *kmers);
int ppg_kmers_count(ppg_ctx *ctx, const void *kmers, const void *set, const uint32_t *dev_mask, int64_t mask_cap,
                    const void *dev_windows, int64_t windows_cap, void *dev_table, int64_t slots, void *result,
                    int64_t *spectrum, int64_t spectrum_cap);
int ppg_kmers_select(ppg_ctx *ctx, const void *dev_table, int64_t slots, int64_t min_count, void *dev_out,
                     int64_t out_cap, int64_t *found);
int ppg_kmers_lookup(ppg_ctx *ctx, const void *dev_table, int64_t slots, const void *dev_keys, int64_t nkeys,
                     int64_t *dev_counts);

/* Library build string (kernel ISA, version). */
const char *ppg_version(void);
/* "inflate-<16 hex>": a hash of the inflate kernels' object (all variants + launcher), fixed at
 * build time.  Measurements quoted from files (bench.py's roofline.traffic) carry it and are
 * refused when it differs from the library in use. */
const char *ppg_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* PPGPU_H */
