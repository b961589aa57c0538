// interop/PpGpu.cs — the P/Invoke class a maintainer adds next to the reference's LibZ
// (Interop/PlatformInterop.cs:6-35) to bind libppgpu.so.  One extern per entry point of
// include/ppgpu.h, same argument order and meaning; status codes keep ZResult's values
// (Interop/Conventions.cs:9-20) plus the library codes in PpgStatus.  (Source only: this image
// has no .NET SDK, so it is not compiled here; tests/test_interop_cs.py checks it covers the
// header exactly.)
using System.Runtime.InteropServices;

namespace ParallelParsing.Interop;

public static class PpgStatus
{
    public const int IndexOutOfRange = -50;   // C# IndexOutOfRangeException (SURVEY Q4, Core.cs:93)
    public const int IoError = -51;
    public const int ArgError = -52;
    public const int Unsupported = -53;
    public const int DeviceError = -100;
    public const int NoDevice = -101;
}

/// <summary>A libppgpu failure that is not a zlib result (PpgStatus codes other than
/// IndexOutOfRange): bad arguments, unreadable files, unsupported input, device errors.  zlib's
/// results keep the reference's ZException (Interop/Conventions.cs:33-41).</summary>
public class PpgException : Exception
{
    public int Code { get; }

    public PpgException(int code, string what) : base($"libppgpu: {what} ({code})")
    {
        Code = code;
    }
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgBatch          // ppg_batch
{
    public int FirstChunk;
    public int NChunks;
    public long RecordBase;
    public long NRecords;
    public byte* Text;                  // raw_k = offset_k ++ chunk_k at Text + RawOff[k]
    public long* RawOff;                // NChunks + 1
    public uint* Desc;                  // (n1, n2, n3, n4) per record, relative to raw_k
    public long* RecOff;                // NChunks + 1
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgPairResult     // ppg_pair_result
{
    public long Pairs;
    public fixed long Records[2];
    public fixed long Duplicates[2];
    public long Mismatches;
    public long FirstBad;
    public fixed long FirstKeys[2];
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgSeqQueryResult // ppg_seq_query_result
{
    public long Records;                // records scanned
    public long Hits;                   // records whose Sequence contains the pattern
    public long Bases;                  // sum of the Sequence lengths
    public fixed long Count[5];         // A, C, G, T, other
}

[StructLayout(LayoutKind.Sequential)]
public struct PpgReadFilter            // ppg_read_filter
{
    public const long Length = 1, Other = 2, Mean = 4, Low = 8, AndMask = 0x100;
    public long Criteria;               // the bits above
    public long MinLen;
    public long MaxLen;                 // -1: no upper bound
    public long MaxOther;               // Sequence bytes that are not A C G T
    public long QualBase;               // the Quality byte of quality 0 (33)
    public long MinMeanMilli;           // 1000 x the least mean quality
    public long LowQ;                   // a base is low when its quality is below this
    public long MaxLowMilli;            // 1000 x the largest fraction of low bases
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgReadFilterResult // ppg_read_filter_result
{
    public long Records;
    public long Passed;
    public fixed long Failed[4];        // length, other, mean quality, low quality
    public long Bases;
    public long Other;
    public long QualBytes;
    public fixed long QualCount[256];   // Quality bytes by value
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgReadTrim        // ppg_read_trim
{
    public const long Leading = 1, Trailing = 2, Window = 4, Adapter = 8, AndMask = 0x100;
    public long Ops;                    // the bits above
    public long Head;                   // bases cut from the 5' end
    public long Tail;                   // bases cut from the 3' end
    public long QualBase;               // the Quality byte of quality 0 (33)
    public long LeadQ;                  // the first base of at least this quality starts the read
    public long TrailQ;                 // the last base of at least this quality ends it
    public long WinSize;                // bases per sliding window, 1 .. 32
    public long WinQ;                   // ... whose mean quality must not fall below this
    public long MinOverlap;             // the least adapter overlap that counts
    public long MaxErrMilli;            // 1000 x the largest fraction of mismatches in it
    public long MinLen;                 // keep: the least trimmed length
    public long AdapterLen;
    public fixed byte AdapterBytes[64];
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgReadTrimResult  // ppg_read_trim_result
{
    public long Records;
    public long Kept;
    public long Trimmed;
    public fixed long Cut[5];           // fixed, leading, trailing, window, adapter
    public long Bases;
    public long BasesWindow;
    public long BasesKept;
}

[StructLayout(LayoutKind.Sequential)]
public struct PpgReadProfile            // ppg_read_profile
{
    public const long UseMask = 1, UseWindows = 2, MaxPositions = 1024;
    public long Flags;                  // the bits above
    public long QualBase;               // the Quality byte of quality 0 (33)
    public long MaxPos;                 // positions profiled, 1 .. MaxPositions
    public long Reserved;               // 0
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgReadProfileResult  // ppg_read_profile_result
{
    public long Records;
    public long Profiled;
    public long Longer;                 // window >= MaxPos
    public long Bases;
    public long BasesProfiled;
    public long QualBytes;
    public long NoQuality;
    public long Reserved;
    public fixed long GcHist[101];
    public fixed long MeanqHist[64];
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgReadDedup       // ppg_read_dedup
{
    public const long UseWindows = 2, AndMask = 0x100;
    public long Flags;                  // the bits above
    public long MaxBases;               // 0: the whole window; 50: FastQC's rule
    public fixed long Reserved[2];      // 0
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgReadDedupResult  // ppg_read_dedup_result
{
    public long Records;
    public long Participating;
    public long Unique;
    public long Bases;
    public long BasesUnique;
    public long Overflow;               // 0
    public long MaxCount;
    public long MaxFirst;               // -1: an empty table
    public fixed long LevelDistinct[16];  // rows with a count of 1 .. 9, 10-49, 50-99, 100-499, 500-999, 1000-4999, 5000-9999, >= 10000
    public fixed long LevelReads[16];
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgPackedView      // ppg_packed_view: device pointers of a packed read set
{
    public long* SeqOff;                // records + 1 entries
    public uint* SeqLen;
    public uint* Bases;
    public uint* Mask;
    public byte* Qual;                  // the overlap does not read it (may be null); the merge needs it
    public long Records;
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgPairOverlap     // ppg_pair_overlap
{
    public long Flags;                  // 0
    public long MinOverlap;             // fastp: 30
    public long MaxDiff;                // fastp: 5
    public long MaxErrMilli;            // fastp: 200
    public fixed long Reserved[4];      // 0
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgPairOverlapResult  // ppg_pair_overlap_result
{
    public const int MaxLen = 1024, HistBins = 2048;   // PPG_OVERLAP_MAX_LEN, PPG_OVERLAP_HIST
    public long Pairs;
    public long Unmapped;
    public long TooLong;
    public long Analysed;
    public long Found;
    public long Negative;               // found with d < 0
    public long Adapter;                // found with an insert shorter than a mate
    public long OverlapBases;
    public long Mismatches;
    public fixed long Clipped[2];       // bases cut from R1 / R2
    public fixed long Reserved[5];
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgPairMerge       // ppg_pair_merge
{
    public long Flags;                  // 0
    public long QualHi;                 // corrected: the taken base's quality byte is at least this (default 63) ...
    public long QualLo;                 // ... and the overruled one's at most this (default 47)
    public fixed long Reserved[5];      // 0
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct PpgPairMergeResult // ppg_pair_merge_result
{
    public long Pairs;
    public long Unmapped;
    public long TooLong;
    public long Unmerged;               // no overlap row
    public long Stale;                  // a row that does not fit its pair
    public long Merged;
    public long MergedBases;
    public long PaddedBases;            // seq_off[merged]
    public long OverlapBases;           // positions both mates cover
    public long Disagree;               // both bases, different
    public long From2;                  // ... decided for read 2
    public long Ties;                   // ... at equal quality (read 1 is taken)
    public long NFilled;                // exactly one side N
    public long NBoth;
    public fixed long Corrected[2];     // read 1 / read 2 overruled across the thresholds
}

internal static unsafe class PpGpu
{
    const string Lib = "ppgpu";   // libppgpu.so from parallelparsing_amd/

    // ---- Index: Common/Index.cs, Common/IndexIO.cs, Core.BuildDeflateIndex (Core.cs:14-131) ----
    [DllImport(Lib)] public static extern int ppg_index_build_file(string gzPath, uint chunksize, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_build_mem(byte* gz, long gzLen, uint chunksize, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_build_gpu(nint ctx, byte* gz, long gzLen, int gzOnDevice,
        uint chunksize, long pieceBytes, long outCapacity, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_build_gpu_side(nint ctx, byte* gz, long gzLen, int gzOnDevice,
        uint chunksize, long pieceBytes, long outCapacity, long sideBytes, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_side_count(nint ix);
    [DllImport(Lib)] public static extern int ppg_index_side_points(nint ix, long* bit, long* output, byte* windows);
    [DllImport(Lib)] public static extern int ppg_index_set_side_points(nint ix, int n, long* bit, long* output,
        byte* windows);
    [DllImport(Lib)] public static extern int ppg_index_build_gpu_file(nint ctx, string gzPath, uint chunksize,
        long pieceBytes, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_build_gpu_stats(nint ctx, double* vals, int n);
    [DllImport(Lib)] public static extern int ppg_index_serialize(nint ix, string path);
    [DllImport(Lib)] public static extern int ppg_index_deserialize(string path, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_from_points(int count, long* output, long* input, int* bits,
        byte* windows, int* offsetLen, byte* offsets, int chunkMaxBytes, out nint ix);
    [DllImport(Lib)] public static extern int ppg_index_count(nint ix);
    [DllImport(Lib)] public static extern int ppg_index_chunk_max_bytes(nint ix);
    [DllImport(Lib)] public static extern int ppg_index_point(nint ix, int i, out long output, out long input,
        out int bits, out int offsetLen);
    [DllImport(Lib)] public static extern byte* ppg_index_window(nint ix, int i);
    [DllImport(Lib)] public static extern byte* ppg_index_offset(nint ix, int i);
    [DllImport(Lib)] public static extern void ppg_index_free(nint ix);
    [DllImport(Lib)] public static extern int ppg_index_validate(nint ix, int first, int n);

    // ---- device context: one per GPU ----
    [DllImport(Lib)] public static extern int ppg_device_count(out int n);
    [DllImport(Lib)] public static extern int ppg_open(int device, out nint ctx);
    [DllImport(Lib)] public static extern void ppg_close(nint ctx);
    [DllImport(Lib)] public static extern nint ppg_ctx_stream(nint ctx);
    [DllImport(Lib)] public static extern int ppg_ctx_wait_stream(nint ctx, nint stream);
    [DllImport(Lib)] public static extern int ppg_stream_wait_ctx(nint ctx, nint stream);

    // ---- README "Decompress": Core.ExtractDeflateIndex (Core.cs:133-192) + Parsing.Parse ----
    [DllImport(Lib)] public static extern int ppg_decompress_chunk(nint ctx, nint ix, int k, byte* slice,
        long sliceLen, byte* output, long outCap, out long produced, uint* recs, long recCap, out long nrec);
    // asynchronous Decompress: many chunks in flight from one caller (ppg_decompress_chunk_submit / _wait)
    [DllImport(Lib)] public static extern int ppg_decompress_chunk_submit(nint ctx, nint ix, int k, byte* slice,
        long sliceLen, byte* outp, long outCap, uint* recs, long recCap, out nint req);
    [DllImport(Lib)] public static extern int ppg_decompress_chunk_wait(nint ctx, nint req, out long produced,
        out long nrec);
    [DllImport(Lib)] public static extern int ppg_decompress_chunk_stats(nint ctx, out long calls, out long launches,
        out long maxBatch);
    [DllImport(Lib)] public static extern int ppg_decompress_chunk_split_stats(nint ctx, out long chunks,
        out long sidePoints);

    // ---- README "DecompressAll": a shard of chunks resident on one GPU ----
    [DllImport(Lib)] public static extern int ppg_shard_create(nint ctx, nint ix, int first, int n, byte* comp,
        long compLen, int compOnDevice, long outCapacity, out nint shard);
    [DllImport(Lib)] public static extern void ppg_shard_free(nint shard);
    [DllImport(Lib)] public static extern int ppg_shard_run(nint shard);
    [DllImport(Lib)] public static extern int ppg_shard_set_split(nint shard, int nsub, long* bit, long* output,
        byte* windows);
    [DllImport(Lib)] public static extern int ppg_shard_results(nint shard, long* records, long* produced,
        int* status, int* flags, long* endBit);
    [DllImport(Lib)] public static extern long ppg_shard_total_records(nint shard);
    [DllImport(Lib)] public static extern int ppg_shard_batches(nint shard);
    [DllImport(Lib)] public static extern int ppg_shard_copy_chunk(nint shard, int k, byte* dst, long cap, out long len);
    [DllImport(Lib)] public static extern int ppg_shard_copy_records(nint shard, int k, uint* dst, long cap,
        out long nrec);
    [DllImport(Lib)] public static extern int ppg_shard_record_base(nint shard, long* b);
    [DllImport(Lib)] public static extern int ppg_shard_copy_output(nint shard, long off, long len, void* dst,
        int dstOnDevice);
    [DllImport(Lib)] public static extern int ppg_shard_keys(nint shard, long* devKeys, long cap);
    [DllImport(Lib)] public static extern int ppg_shard_set_keys(nint shard, long* devKeys, long cap);
    [DllImport(Lib)] public static extern int ppg_shard_keys_ready(nint shard);
    // packed reads: 2-bit bases, N mask, qualities (device planes; the format is in ppgpu.h)
    [DllImport(Lib)] public static extern int ppg_shard_seq_bases(nint shard, out long totalBases, out long records);
    [DllImport(Lib)] public static extern int ppg_shard_pack_seq(nint shard, long* devSeqOff, uint* devSeqLen, long recCap,
        uint* devBases, uint* devMask, byte* devQual, long baseCap, out long totalBases);
    [DllImport(Lib)] public static extern int ppg_shard_set_seqpack(nint shard, long* devSeqOff, uint* devSeqLen,
        long recCap, uint* devBases, uint* devMask, byte* devQual, long baseCap);
    [DllImport(Lib)] public static extern int ppg_shard_seqpack_ready(nint shard, out long totalBases);
    // sequence queries: Sequence.Contains(pattern) per record and the base census (result: a PpgSeqQueryResult*)
    [DllImport(Lib)] public static extern int ppg_shard_query_seq(nint shard, byte* pattern, int patternLen,
        uint* devHitMask, long recCap, long* chunkHits, void* result);
    [DllImport(Lib)] public static extern int ppg_shard_set_seqquery(nint shard, byte* pattern, int patternLen,
        uint* devHitMask, long recCap);
    [DllImport(Lib)] public static extern int ppg_shard_seqquery_ready(nint shard, long* chunkHits, void* result);
    // read filters: length, N content and quality per record and the pass bits they give (filter: a
    // PpgReadFilter*, result: a PpgReadFilterResult*; mask and metrics are device pointers)
    [DllImport(Lib)] public static extern int ppg_read_filter_check(void* filter);
    [DllImport(Lib)] public static extern int ppg_shard_filter_reads(nint shard, void* filter, uint* devPassMask,
        long recCap, void* devMetrics, long metricsCap, long* chunkPassed, void* result);
    [DllImport(Lib)] public static extern int ppg_shard_set_readfilter(nint shard, void* filter, uint* devPassMask,
        long recCap, void* devMetrics, long metricsCap);
    [DllImport(Lib)] public static extern int ppg_shard_readfilter_ready(nint shard, long* chunkPassed, void* result);
    // read trimming: the window (start, len) of every record and the keep bits (trim: a PpgReadTrim*,
    // result: a PpgReadTrimResult*; mask and rows are device pointers)
    [DllImport(Lib)] public static extern int ppg_read_trim_check(void* trim);
    [DllImport(Lib)] public static extern int ppg_shard_trim_reads(nint shard, void* trim, uint* devKeepMask,
        long recCap, void* devTrim, long trimCap, long* chunkKept, void* result);
    [DllImport(Lib)] public static extern int ppg_shard_set_readtrim(nint shard, void* trim, uint* devKeepMask,
        long recCap, void* devTrim, long trimCap);
    [DllImport(Lib)] public static extern int ppg_shard_readtrim_ready(nint shard, long* chunkKept, void* result);
    // read profile: bases and qualities per read position, lengths, GC and mean quality per read (profile: a
    // PpgReadProfile*, result: a PpgReadProfileResult*, table: host rows of 72 longs; mask and rows are device
    // pointers and only read)
    [DllImport(Lib)] public static extern int ppg_read_profile_check(void* profile);
    [DllImport(Lib)] public static extern int ppg_shard_profile_reads(nint shard, void* profile, uint* devMask,
        long maskCap, void* devWindows, long windowsCap, long* chunkProfiled, void* result, long* table, long tableCap);
    [DllImport(Lib)] public static extern int ppg_shard_set_readprofile(nint shard, void* profile, uint* devMask,
        long maskCap, void* devWindows, long windowsCap);
    [DllImport(Lib)] public static extern int ppg_shard_readprofile_ready(nint shard, long* chunkProfiled, void* result,
        long* table, long tableCap);
    // read dedup: first occurrences by a 64-bit fingerprint and the duplication levels (dedup: a PpgReadDedup*,
    // result: a PpgReadDedupResult*; mask, rows, first and the table of slots x 3 ulongs are device pointers)
    [DllImport(Lib)] public static extern int ppg_read_dedup_check(void* dedup);
    [DllImport(Lib)] public static extern int ppg_shard_dedup_reads(nint shard, void* dedup, uint* devUniqueMask,
        long maskCap, void* devWindows, long windowsCap, long* devFirst, long firstCap, void* devTable, long slots,
        long* chunkUnique, void* result);
    [DllImport(Lib)] public static extern int ppg_shard_set_readdedup(nint shard, void* dedup, uint* devUniqueMask,
        long maskCap, void* devWindows, long windowsCap, long* devFirst, long firstCap, void* devTable, long slots);
    [DllImport(Lib)] public static extern int ppg_shard_readdedup_ready(nint shard, long* chunkUnique, void* result);
    // record selection: the records a mask selects, compacted on the GPU (device pointers; a null mask
    // with maskCap 0 selects every record)
    [DllImport(Lib)] public static extern int ppg_shard_select_size(nint shard, uint* devMask, long maskCap,
        out long records, out long bytes);
    [DllImport(Lib)] public static extern int ppg_shard_select_records(nint shard, uint* devMask, long maskCap,
        long* devRecno, long* devSelOff, uint* devDesc, long selCap, byte* devBytes, long byteCap, out long records,
        out long bytes);
    [DllImport(Lib)] public static extern int ppg_shard_set_select(nint shard, uint* devMask, long maskCap,
        long* devRecno, long* devSelOff, uint* devDesc, long selCap, byte* devBytes, long byteCap);
    [DllImport(Lib)] public static extern int ppg_shard_select_ready(nint shard, out long records, out long bytes);
    [DllImport(Lib)] public static extern int ppg_shard_counts_to_device(nint shard, long* devDst);
    [DllImport(Lib)] public static extern int ppg_shard_timing(nint shard, out float inflateMs, out float parseMs,
        out float totalMs);

    // ---- LazyFileReader (LazyFileReader.cs:10-98): DecompressAll straight from the file ----
    [DllImport(Lib)] public static extern int ppg_file_decompress_all(nint ctx, nint ix, string gzPath, int first,
        int n, long pieceBytes, int threads, long* records, out long totalRecords, out double seconds);
    [DllImport(Lib)] public static extern int ppg_file_release(nint ctx);

    // ---- BatchedFASTQ's enumerator (BatchedFASTQ.cs:29-101): streamed record batches ----
    [DllImport(Lib)] public static extern int ppg_cursor_open(nint ctx, nint ix, string gzPath, int first, int n,
        long batchBytes, int threads, out nint cursor);
    [DllImport(Lib)] public static extern int ppg_cursor_next(nint cursor, out PpgBatch batch);
    [DllImport(Lib)] public static extern int ppg_cursor_batches(nint cursor);
    [DllImport(Lib)] public static extern void ppg_cursor_close(nint cursor);
    // the packed enumerator: batches of packed reads in pinned host memory (planes bit 0 = qualities)
    [DllImport(Lib)] public static extern int ppg_cursor_open_packed(nint ctx, nint ix, string gzPath, int first, int n,
        long batchBytes, int threads, int planes, out nint cursor);
    [DllImport(Lib)] public static extern int ppg_cursor_packed(nint cursor, uint** bases, uint** mask, byte** qual,
        uint** seqLen, out long totalBases);
    [DllImport(Lib)] public static extern int ppg_cursor_packed_offsets(nint cursor, long* seqOff, long cap);
    // the filtered enumerator: batches of the records whose Sequence contains the pattern, selected on
    // the GPU, in pinned host memory (descriptors relative to each record's first byte)
    [DllImport(Lib)] public static extern int ppg_cursor_open_select(nint ctx, nint ix, string gzPath, int first, int n,
        long batchBytes, int threads, byte* pattern, int patternLen, out nint cursor);
    [DllImport(Lib)] public static extern int ppg_cursor_selected(nint cursor, byte** bytes, uint** desc,
        out long records, out long nbytes);
    [DllImport(Lib)] public static extern int ppg_cursor_selected_index(nint cursor, long* selOff, long* recno, long cap);
    // ... narrowed to the hits that pass a read filter (a null filter: ppg_cursor_open_select)
    [DllImport(Lib)] public static extern int ppg_cursor_open_filter(nint ctx, nint ix, string gzPath, int first, int n,
        long batchBytes, int threads, byte* pattern, int patternLen, void* filter, out nint cursor);
    [DllImport(Lib)] public static extern int ppg_cursor_filter_result(nint cursor, void* result);
    // ... and trimmed: "hit, pass and keep", every selected record with its window (null filter / trim: none)
    [DllImport(Lib)] public static extern int ppg_cursor_open_trim(nint ctx, nint ix, string gzPath, int first, int n,
        long batchBytes, int threads, byte* pattern, int patternLen, void* filter, void* trim, out nint cursor);
    [DllImport(Lib)] public static extern int ppg_cursor_selected_trim(nint cursor, uint** trim);
    [DllImport(Lib)] public static extern int ppg_cursor_trim_result(nint cursor, void* result);

    // ---- multi-GPU DecompressAll: partition + count all-gather over RCCL inside the library ----
    [DllImport(Lib)] public static extern int ppg_comm_unique_id(byte* id /* 128 bytes */);
    [DllImport(Lib)] public static extern int ppg_comm_init(nint ctx, int nranks, int rank, byte* id, out nint comm);
    [DllImport(Lib)] public static extern int ppg_comm_from_rccl(nint ctx, nint ncclComm, int nranks, int rank,
        out nint comm);
    [DllImport(Lib)] public static extern int ppg_comm_init_host(int nranks, int rank, string name, out nint comm);
    [DllImport(Lib)] public static extern int ppg_comm_rank(nint comm, out int rank, out int nranks);
    [DllImport(Lib)] public static extern void ppg_comm_free(nint comm);
    [DllImport(Lib)] public static extern int ppg_rccl_version(out int version);
    [DllImport(Lib)] public static extern int ppg_comm_alltoallv(nint comm, long* send, long* recv, long* counts,
        int onDevice);
    [DllImport(Lib)] public static extern int ppg_partition(nint ix, int first, int n, int nranks, int* bounds);
    [DllImport(Lib)] public static extern int ppg_shard_gather_counts(nint shard, nint comm, int* bounds,
        long* counts, long* bases, out long totalRecords);
    [DllImport(Lib)] public static extern int ppg_dist_decompress_all(nint ctx, nint comm, nint ix, string gzPath,
        long outCapacity, long* counts, long* bases, out long totalRecords);

    // ---- paired reads (SURVEY §8f #3, README.md:9): R1 / R2 shards checked on the device ----
    [DllImport(Lib)] public static extern int ppg_pairs_create(out nint pairs);
    [DllImport(Lib)] public static extern int ppg_pairs_check(nint pairs, nint r1, nint r2, nint comm,
        out PpgPairResult result);
    [DllImport(Lib)] public static extern int ppg_pairs_records(nint pairs, int file, long lo, long hi,
        long* shardRecord);
    [DllImport(Lib)] public static extern void ppg_pairs_free(nint pairs);
    // record-aligned pair chunks, packed on the device (ppg_pairs_emit_*)
    [DllImport(Lib)] public static extern int ppg_pairs_emit_begin(nint pairs, nint r1, nint r2, nint comm,
        long pairChunk, long windowBytes);
    [DllImport(Lib)] public static extern int ppg_pairs_emit_run(nint pairs, nint r1, nint r2, long pairChunk,
        long windowBytes);
    [DllImport(Lib)] public static extern int ppg_pairs_emit_next(nint pairs, out long j0, out long j1);
    [DllImport(Lib)] public static extern int ppg_pairs_chunk(nint pairs, long j, int file, out nint bytes, out long len,
        out nint desc, out long nrec);
    [DllImport(Lib)] public static extern int ppg_pairs_copy_chunk(nint pairs, long j, int file, byte* dst, long cap,
        out long len, uint* desc, long descCap, out long nrec);
    [DllImport(Lib)] public static extern int ppg_pairs_emit_stats(nint pairs, double* vals, int n);

    // pair overlap: insert sizes and the 3' cut of both mates (overlap: a PpgPairOverlap*, set1 / set2: a
    // PpgPackedView*, result: a PpgPairOverlapResult*; the maps, rows, mask and windows are device pointers,
    // hist is host memory of PpgPairOverlapResult.HistBins longs)
    [DllImport(Lib)] public static extern int ppg_pair_overlap_check(void* overlap);
    [DllImport(Lib)] public static extern int ppg_pairs_overlap(nint ctx, void* overlap, void* set1, void* set2,
        long* devRec1, long* devRec2, long npairs, void* devRows, long rowCap, uint* devFoundMask, long maskCap,
        void* devWindows1, long winCap1, void* devWindows2, long winCap2, void* result, long* hist, long histCap);

    // pair merge: one consensus read per overlapping pair as a third packed read set (merge: a PpgPairMerge*,
    // set1 / set2: a PpgPackedView* with Qual, result: a PpgPairMergeResult*; the maps, rows and output planes are
    // device pointers)
    [DllImport(Lib)] public static extern int ppg_pair_merge_check(void* merge);
    [DllImport(Lib)] public static extern int ppg_pairs_merge_size(nint ctx, void* set1, void* set2, long* devRec1,
        long* devRec2, long npairs, void* devRows, long rowCap, out long merged, out long paddedBases);
    [DllImport(Lib)] public static extern int ppg_pairs_merge(nint ctx, void* merge, void* set1, void* set2,
        long* devRec1, long* devRec2, long npairs, void* devRows, long rowCap, long* devSeqOff, uint* devSeqLen,
        long recCap, uint* devBases, uint* devMask, byte* devQual, long baseCap, long* devPairOf, void* result);

    // k-mer counts: the spectrum and the most frequent k-mers of a packed read set (kmers: eight longs -- flags
    // (1 canonical, 2 use windows, 4 use mask, 8 accumulate), k, six zeros; set: a PpgPackedView*; the mask, windows,
    // table (slots rows of two ulongs {key, count}, an empty row {~0, 0}), out rows, keys and counts are device
    // pointers; result: sixteen longs and spectrum: 1024 longs of host memory)
    [DllImport(Lib)] public static extern int ppg_kmer_count_check(void* kmers);
    [DllImport(Lib)] public static extern int ppg_kmers_count(nint ctx, void* kmers, void* set, uint* devMask,
        long maskCap, void* devWindows, long windowsCap, void* devTable, long slots, void* result, long* spectrum,
        long spectrumCap);
    [DllImport(Lib)] public static extern int ppg_kmers_select(nint ctx, void* devTable, long slots, long minCount,
        void* devOut, long outCap, out long found);
    [DllImport(Lib)] public static extern int ppg_kmers_lookup(nint ctx, void* devTable, long slots, void* devKeys,
        long nkeys, long* devCounts);

    [DllImport(Lib)] public static extern nint ppg_version();
    [DllImport(Lib)] public static extern nint ppg_build_id();

    // Status -> exception, as the reference's callers do (Core.cs:31-34, :68-74, :178-179): zlib's
    // ZResult codes (Conventions.cs:9-20) become ZException; the IndexOutOfRange that CreateIndex's
    // offset buffer throws in the reference (Core.cs:93, SURVEY Q4) stays IndexOutOfRangeException;
    // every library code becomes a PpgException carrying it.  Every PPG_* status of ppgpu.h has a
    // case here (tests/test_interop_cs.py); an unknown code is a PpgException too, never a ZResult
    // cast of a value the enum does not define.
    public static void Check(int rc)
    {
        switch (rc)
        {
            case 0: return;                                                       // PPG_OK
            case 1: throw new ZException(ZResult.STREAM_END);                     // PPG_STREAM_END
            case 2: throw new ZException(ZResult.NEED_DICT);                      // PPG_NEED_DICT
            case -1: throw new ZException(ZResult.ERRNO);                         // PPG_ERRNO
            case -2: throw new ZException(ZResult.STREAM_ERROR);                  // PPG_STREAM_ERROR
            case -3: throw new ZException(ZResult.DATA_ERROR);                    // PPG_DATA_ERROR
            case -4: throw new ZException(ZResult.MEM_ERROR);                     // PPG_MEM_ERROR
            case -5: throw new ZException(ZResult.BUF_ERROR);                     // PPG_BUF_ERROR
            case -6: throw new ZException(ZResult.VERSION_ERROR);                 // PPG_VERSION_ERROR
            case -50: throw new IndexOutOfRangeException();                       // PPG_INDEX_OUT_OF_RANGE
            case -51: throw new PpgException(rc, "I/O error");                    // PPG_IO_ERROR
            case -52: throw new PpgException(rc, "invalid argument");             // PPG_ARG_ERROR
            case -53: throw new PpgException(rc, "unsupported input");            // PPG_UNSUPPORTED
            case -100: throw new PpgException(rc, "device error");                // PPG_DEVICE_ERROR
            case -101: throw new PpgException(rc, "no gfx950 device");            // PPG_NO_DEVICE
            default: throw new PpgException(rc, "unknown status");
        }
    }
}
