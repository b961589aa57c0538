"""ctypes binding of libppgpu.so (include/ppgpu.h) and libppgsynth.so.

The HIP library is required: there is no CPU fallback for the decode path.  Importing this
module without a built libppgpu.so raises ImportError; opening a context without an MI355X
(gfx950) raises PpgError(PPG_NO_DEVICE).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPG_LIB_PATH") or os.path.join(_HERE, "libppgpu.so")
SYNTH_PATH = os.path.join(_HERE, "libppgsynth.so")

PPG_OK = 0
PPG_STREAM_END = 1
PPG_DATA_ERROR = -3
PPG_BUF_ERROR = -5
PPG_INDEX_OUT_OF_RANGE = -50
PPG_IO_ERROR = -51
PPG_ARG_ERROR = -52
PPG_UNSUPPORTED = -53
PPG_DEVICE_ERROR = -100
PPG_NO_DEVICE = -101

# ZResult names (Interop/Conventions.cs:9-20) for messages
_NAMES = {0: "OK", 1: "STREAM_END", 2: "NEED_DICT", -1: "ERRNO", -2: "STREAM_ERROR", -3: "DATA_ERROR",
          -4: "MEM_ERROR", -5: "BUF_ERROR", -6: "VERSION_ERROR", -50: "INDEX_OUT_OF_RANGE", -51: "IO_ERROR",
          -52: "ARG_ERROR", -53: "UNSUPPORTED", -100: "DEVICE_ERROR", -101: "NO_DEVICE"}


class PpgError(RuntimeError):
    """A non-zero status from libppgpu — the ZException of Interop/Conventions.cs:33-41."""

    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"{what}: {_NAMES.get(code, code)} ({code})")


def check(code, what):
    if code != PPG_OK:
        raise PpgError(code, what)
    return code


def _load(path, what):
    if not os.path.exists(path):
        raise ImportError(f"{what} not built at {path}: run `make -C parallelparsing_amd/csrc` "
                          f"(or __graft_entry__.build()); there is no fallback implementation")
    return C.CDLL(path)


# One HIP runtime per process: torch (when present) bundles its own libamdhip64 with the same soname
# as /opt/rocm's.  Whichever loads first serves both, and torch fails to initialise the GPU on the
# other's.  Importing torch first makes libppgpu bind to torch's runtime, as in bench.py.
try:
    import torch  # noqa: F401
except ImportError:
    pass

lib = _load(LIB_PATH, "libppgpu.so")

vp = C.c_void_p
i32, i64, u32 = C.c_int32, C.c_int64, C.c_uint32
P = C.POINTER

_SIGS = {
    "ppg_index_build_file": (C.c_int, [C.c_char_p, u32, P(vp)]),
    "ppg_index_build_mem": (C.c_int, [vp, i64, u32, P(vp)]),
    "ppg_index_build_gpu": (C.c_int, [vp, vp, i64, C.c_int, u32, i64, i64, P(vp)]),
    "ppg_index_build_gpu_side": (C.c_int, [vp, vp, i64, C.c_int, u32, i64, i64, i64, P(vp)]),
    "ppg_index_side_count": (C.c_int, [vp]),
    "ppg_index_set_side_points": (C.c_int, [vp, i32, vp, vp, vp]),
    "ppg_index_side_points": (C.c_int, [vp, vp, vp, vp]),
    "ppg_index_build_gpu_file": (C.c_int, [vp, C.c_char_p, u32, i64, P(vp)]),
    "ppg_index_build_gpu_stats": (C.c_int, [vp, P(C.c_double), i32]),
    "ppg_index_serialize": (C.c_int, [vp, C.c_char_p]),
    "ppg_index_deserialize": (C.c_int, [C.c_char_p, P(vp)]),
    "ppg_index_from_points": (C.c_int, [i32, vp, vp, vp, vp, vp, vp, i32, P(vp)]),
    "ppg_index_count": (i32, [vp]),
    "ppg_index_chunk_max_bytes": (i32, [vp]),
    "ppg_index_point": (C.c_int, [vp, i32, P(i64), P(i64), P(i32), P(i32)]),
    "ppg_index_window": (vp, [vp, i32]),
    "ppg_index_offset": (vp, [vp, i32]),
    "ppg_index_free": (None, [vp]),
    "ppg_index_validate": (C.c_int, [vp, i32, i32]),
    "ppg_device_count": (C.c_int, [P(C.c_int)]),
    "ppg_open": (C.c_int, [C.c_int, P(vp)]),
    "ppg_close": (None, [vp]),
    "ppg_ctx_stream": (vp, [vp]),
    "ppg_ctx_wait_stream": (C.c_int, [vp, vp]),
    "ppg_stream_wait_ctx": (C.c_int, [vp, vp]),
    "ppg_decompress_chunk": (C.c_int, [vp, vp, i32, vp, i64, vp, i64, P(i64), vp, i64, P(i64)]),
    "ppg_decompress_chunk_stats": (C.c_int, [vp, P(i64), P(i64), P(i64)]),
    "ppg_decompress_chunk_submit": (C.c_int, [vp, vp, i32, vp, i64, vp, i64, vp, i64, P(vp)]),
    "ppg_decompress_chunk_wait": (C.c_int, [vp, vp, P(i64), P(i64)]),
    "ppg_decompress_chunk_split_stats": (C.c_int, [vp, P(i64), P(i64)]),
    "ppg_shard_create": (C.c_int, [vp, vp, i32, i32, vp, i64, C.c_int, i64, P(vp)]),
    "ppg_shard_free": (None, [vp]),
    "ppg_shard_run": (C.c_int, [vp]),
    "ppg_shard_results": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "ppg_shard_total_records": (i64, [vp]),
    "ppg_shard_batches": (i32, [vp]),
    "ppg_shard_set_split": (C.c_int, [vp, i32, vp, vp, vp]),
    "ppg_shard_copy_chunk": (C.c_int, [vp, i32, vp, i64, P(i64)]),
    "ppg_shard_copy_records": (C.c_int, [vp, i32, vp, i64, P(i64)]),
    "ppg_shard_record_base": (C.c_int, [vp, vp]),
    "ppg_shard_copy_output": (C.c_int, [vp, i64, i64, vp, C.c_int]),
    "ppg_shard_keys": (C.c_int, [vp, vp, i64]),
    "ppg_shard_set_keys": (C.c_int, [vp, vp, i64]),
    "ppg_shard_counts_to_device": (C.c_int, [vp, vp]),
    "ppg_shard_timing": (C.c_int, [vp, P(C.c_float), P(C.c_float), P(C.c_float)]),
    "ppg_file_decompress_all": (C.c_int, [vp, vp, C.c_char_p, i32, i32, i64, C.c_int, vp, P(i64), P(C.c_double)]),
    "ppg_file_release": (C.c_int, [vp]),
    "ppg_version": (C.c_char_p, []),
    "ppg_build_id": (C.c_char_p, []),
    "ppg_cursor_open": (C.c_int, [vp, vp, C.c_char_p, i32, i32, i64, C.c_int, P(vp)]),
    "ppg_cursor_next": (C.c_int, [vp, vp]),
    "ppg_cursor_batches": (i32, [vp]),
    "ppg_cursor_close": (None, [vp]),
    "ppg_shard_seq_bases": (C.c_int, [vp, P(i64), P(i64)]),
    "ppg_shard_pack_seq": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, i64, P(i64)]),
    "ppg_shard_set_seqpack": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, i64]),
    "ppg_shard_seqpack_ready": (C.c_int, [vp, P(i64)]),
    "ppg_shard_query_seq": (C.c_int, [vp, vp, i32, vp, i64, vp, vp]),
    "ppg_shard_set_seqquery": (C.c_int, [vp, vp, i32, vp, i64]),
    "ppg_shard_seqquery_ready": (C.c_int, [vp, vp, vp]),
    "ppg_read_filter_check": (C.c_int, [vp]),
    "ppg_shard_filter_reads": (C.c_int, [vp, vp, vp, i64, vp, i64, vp, vp]),
    "ppg_shard_set_readfilter": (C.c_int, [vp, vp, vp, i64, vp, i64]),
    "ppg_shard_readfilter_ready": (C.c_int, [vp, vp, vp]),
    "ppg_cursor_open_filter": (C.c_int, [vp, vp, C.c_char_p, i32, i32, i64, C.c_int, vp, i32, vp, P(vp)]),
    "ppg_cursor_filter_result": (C.c_int, [vp, vp]),
    "ppg_read_trim_check": (C.c_int, [vp]),
    "ppg_shard_trim_reads": (C.c_int, [vp, vp, vp, i64, vp, i64, vp, vp]),
    "ppg_shard_set_readtrim": (C.c_int, [vp, vp, vp, i64, vp, i64]),
    "ppg_shard_readtrim_ready": (C.c_int, [vp, vp, vp]),
    "ppg_cursor_open_trim": (C.c_int, [vp, vp, C.c_char_p, i32, i32, i64, C.c_int, vp, i32, vp, vp, P(vp)]),
    "ppg_cursor_selected_trim": (C.c_int, [vp, P(vp)]),
    "ppg_cursor_trim_result": (C.c_int, [vp, vp]),
    "ppg_read_profile_check": (C.c_int, [vp]),
    "ppg_shard_profile_reads": (C.c_int, [vp, vp, vp, i64, vp, i64, vp, vp, vp, i64]),
    "ppg_shard_set_readprofile": (C.c_int, [vp, vp, vp, i64, vp, i64]),
    "ppg_shard_readprofile_ready": (C.c_int, [vp, vp, vp, vp, i64]),
    "ppg_read_dedup_check": (C.c_int, [vp]),
    "ppg_shard_dedup_reads": (C.c_int, [vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]),
    "ppg_shard_set_readdedup": (C.c_int, [vp, vp, vp, i64, vp, i64, vp, i64, vp, i64]),
    "ppg_shard_readdedup_ready": (C.c_int, [vp, vp, vp]),
    "ppg_shard_select_size": (C.c_int, [vp, vp, i64, P(i64), P(i64)]),
    "ppg_shard_select_records": (C.c_int, [vp, vp, i64, vp, vp, vp, i64, vp, i64, P(i64), P(i64)]),
    "ppg_shard_set_select": (C.c_int, [vp, vp, i64, vp, vp, vp, i64, vp, i64]),
    "ppg_shard_select_ready": (C.c_int, [vp, P(i64), P(i64)]),
    "ppg_cursor_open_select": (C.c_int, [vp, vp, C.c_char_p, i32, i32, i64, C.c_int, vp, i32, P(vp)]),
    "ppg_cursor_selected": (C.c_int, [vp, P(vp), P(vp), P(i64), P(i64)]),
    "ppg_cursor_selected_index": (C.c_int, [vp, vp, vp, i64]),
    "ppg_cursor_open_packed": (C.c_int, [vp, vp, C.c_char_p, i32, i32, i64, C.c_int, i32, P(vp)]),
    "ppg_cursor_packed": (C.c_int, [vp, P(vp), P(vp), P(vp), P(vp), P(i64)]),
    "ppg_cursor_packed_offsets": (C.c_int, [vp, vp, i64]),
    "ppg_comm_unique_id": (C.c_int, [vp]),
    "ppg_comm_init": (C.c_int, [vp, i32, i32, vp, P(vp)]),
    "ppg_comm_from_rccl": (C.c_int, [vp, vp, i32, i32, P(vp)]),
    "ppg_comm_init_host": (C.c_int, [i32, i32, C.c_char_p, P(vp)]),
    "ppg_comm_rank": (C.c_int, [vp, P(i32), P(i32)]),
    "ppg_comm_free": (None, [vp]),
    "ppg_rccl_version": (C.c_int, [P(C.c_int)]),
    "ppg_partition": (C.c_int, [vp, i32, i32, i32, vp]),
    "ppg_shard_gather_counts": (C.c_int, [vp, vp, vp, vp, vp, P(i64)]),
    "ppg_dist_decompress_all": (C.c_int, [vp, vp, vp, C.c_char_p, i64, vp, vp, P(i64)]),
    "ppg_shard_keys_ready": (C.c_int, [vp]),
    "ppg_comm_alltoallv": (C.c_int, [vp, vp, vp, vp, C.c_int]),
    "ppg_pairs_create": (C.c_int, [P(vp)]),
    "ppg_pairs_check": (C.c_int, [vp, vp, vp, vp, vp]),
    "ppg_pairs_records": (C.c_int, [vp, i32, i64, i64, vp]),
    "ppg_pairs_free": (None, [vp]),
    "ppg_pairs_emit_begin": (C.c_int, [vp, vp, vp, vp, i64, i64]),
    "ppg_pairs_emit_run": (C.c_int, [vp, vp, vp, i64, i64]),
    "ppg_pairs_emit_next": (C.c_int, [vp, P(i64), P(i64)]),
    "ppg_pairs_chunk": (C.c_int, [vp, i64, i32, P(vp), P(i64), P(vp), P(i64)]),
    "ppg_pairs_copy_chunk": (C.c_int, [vp, i64, i32, vp, i64, P(i64), vp, i64, P(i64)]),
    "ppg_pairs_emit_stats": (C.c_int, [vp, P(C.c_double), i32]),
    "ppg_pair_overlap_check": (C.c_int, [vp]),
    "ppg_pairs_overlap": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i64]),
    "ppg_pair_merge_check": (C.c_int, [vp]),
    "ppg_pairs_merge_size": (C.c_int, [vp, vp, vp, vp, vp, i64, vp, i64, P(i64), P(i64)]),
    "ppg_pairs_merge": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp, vp]),
    "ppg_kmer_count_check": (C.c_int, [vp]),
    "ppg_kmers_count": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, i64]),
    "ppg_kmers_select": (C.c_int, [vp, vp, i64, i64, vp, i64, P(i64)]),
    "ppg_kmers_lookup": (C.c_int, [vp, vp, i64, vp, i64, vp]),
}


class PpgBatch(C.Structure):
    """ppg_batch (include/ppgpu.h)."""
    _fields_ = [("first_chunk", C.c_int32), ("nchunks", C.c_int32), ("record_base", C.c_int64),
                ("nrecords", C.c_int64), ("text", C.c_void_p), ("raw_off", C.POINTER(C.c_int64)),
                ("desc", C.POINTER(C.c_uint32)), ("rec_off", C.POINTER(C.c_int64))]


class PpgPairResult(C.Structure):
    """ppg_pair_result (include/ppgpu.h)."""
    _fields_ = [("pairs", C.c_int64), ("records", C.c_int64 * 2), ("duplicates", C.c_int64 * 2),
                ("mismatches", C.c_int64), ("first_bad", C.c_int64), ("first_keys", C.c_int64 * 2)]


class PpgSeqQueryResult(C.Structure):
    """ppg_seq_query_result (include/ppgpu.h)."""
    _fields_ = [("records", C.c_int64), ("hits", C.c_int64), ("bases", C.c_int64), ("count", C.c_int64 * 5)]


class PpgReadFilter(C.Structure):
    """ppg_read_filter (include/ppgpu.h)."""
    _fields_ = [("criteria", C.c_int64), ("min_len", C.c_int64), ("max_len", C.c_int64), ("max_other", C.c_int64),
                ("qual_base", C.c_int64), ("min_mean_milli", C.c_int64), ("low_q", C.c_int64),
                ("max_low_milli", C.c_int64)]


class PpgReadFilterResult(C.Structure):
    """ppg_read_filter_result (include/ppgpu.h)."""
    _fields_ = [("records", C.c_int64), ("passed", C.c_int64), ("failed", C.c_int64 * 4), ("bases", C.c_int64),
                ("other", C.c_int64), ("qual_bytes", C.c_int64), ("qual_count", C.c_int64 * 256)]


PPG_FILTER_LENGTH, PPG_FILTER_OTHER, PPG_FILTER_MEAN, PPG_FILTER_LOW, PPG_FILTER_AND_MASK = 1, 2, 4, 8, 0x100


class PpgReadTrim(C.Structure):
    """ppg_read_trim (include/ppgpu.h)."""
    _fields_ = [("ops", C.c_int64), ("head", C.c_int64), ("tail", C.c_int64), ("qual_base", C.c_int64),
                ("lead_q", C.c_int64), ("trail_q", C.c_int64), ("win_size", C.c_int64), ("win_q", C.c_int64),
                ("min_overlap", C.c_int64), ("max_err_milli", C.c_int64), ("min_len", C.c_int64),
                ("adapter_len", C.c_int64), ("adapter", C.c_uint8 * 64)]


class PpgReadTrimResult(C.Structure):
    """ppg_read_trim_result (include/ppgpu.h)."""
    _fields_ = [("records", C.c_int64), ("kept", C.c_int64), ("trimmed", C.c_int64), ("cut", C.c_int64 * 5),
                ("bases", C.c_int64), ("bases_window", C.c_int64), ("bases_kept", C.c_int64)]


PPG_TRIM_LEADING, PPG_TRIM_TRAILING, PPG_TRIM_WINDOW, PPG_TRIM_ADAPTER, PPG_TRIM_AND_MASK = 1, 2, 4, 8, 0x100


class PpgReadProfile(C.Structure):
    """ppg_read_profile (include/ppgpu.h)."""
    _fields_ = [("flags", C.c_int64), ("qual_base", C.c_int64), ("max_pos", C.c_int64), ("reserved", C.c_int64)]


class PpgReadProfileResult(C.Structure):
    """ppg_read_profile_result (include/ppgpu.h)."""
    _fields_ = [("records", C.c_int64), ("profiled", C.c_int64), ("longer", C.c_int64), ("bases", C.c_int64),
                ("bases_profiled", C.c_int64), ("qual_bytes", C.c_int64), ("no_quality", C.c_int64),
                ("reserved", C.c_int64), ("gc_hist", C.c_int64 * 101), ("meanq_hist", C.c_int64 * 64)]


PPG_PROFILE_USE_MASK, PPG_PROFILE_USE_WINDOWS, PPG_PROFILE_MAX_POS = 1, 2, 1024


class PpgReadDedup(C.Structure):
    """ppg_read_dedup (include/ppgpu.h)."""
    _fields_ = [("flags", C.c_int64), ("max_bases", C.c_int64), ("reserved", C.c_int64 * 2)]


class PpgReadDedupResult(C.Structure):
    """ppg_read_dedup_result (include/ppgpu.h)."""
    _fields_ = [("records", C.c_int64), ("participating", C.c_int64), ("unique", C.c_int64), ("bases", C.c_int64),
                ("bases_unique", C.c_int64), ("overflow", C.c_int64), ("max_count", C.c_int64), ("max_first", C.c_int64),
                ("level_distinct", C.c_int64 * 16), ("level_reads", C.c_int64 * 16)]


PPG_DEDUP_USE_WINDOWS, PPG_DEDUP_AND_MASK = 2, 0x100


class PpgPackedView(C.Structure):
    """ppg_packed_view (include/ppgpu.h): device pointers of a packed read set."""
    _fields_ = [("seq_off", C.c_void_p), ("seq_len", C.c_void_p), ("bases", C.c_void_p), ("mask", C.c_void_p),
                ("qual", C.c_void_p), ("records", C.c_int64)]


class PpgPairOverlap(C.Structure):
    """ppg_pair_overlap (include/ppgpu.h)."""
    _fields_ = [("flags", C.c_int64), ("min_overlap", C.c_int64), ("max_diff", C.c_int64), ("max_err_milli", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class PpgPairOverlapResult(C.Structure):
    """ppg_pair_overlap_result (include/ppgpu.h)."""
    _fields_ = [("pairs", C.c_int64), ("unmapped", C.c_int64), ("too_long", C.c_int64), ("analysed", C.c_int64),
                ("found", C.c_int64), ("negative", C.c_int64), ("adapter", C.c_int64), ("overlap_bases", C.c_int64),
                ("mismatches", C.c_int64), ("clipped", C.c_int64 * 2), ("reserved", C.c_int64 * 5)]


PPG_OVERLAP_MAX_LEN, PPG_OVERLAP_HIST = 1024, 2048


class PpgPairMerge(C.Structure):
    """ppg_pair_merge (include/ppgpu.h)."""
    _fields_ = [("flags", C.c_int64), ("qual_hi", C.c_int64), ("qual_lo", C.c_int64), ("reserved", C.c_int64 * 5)]


class PpgPairMergeResult(C.Structure):
    """ppg_pair_merge_result (include/ppgpu.h)."""
    _fields_ = [("pairs", C.c_int64), ("unmapped", C.c_int64), ("too_long", C.c_int64), ("unmerged", C.c_int64),
                ("stale", C.c_int64), ("merged", C.c_int64), ("merged_bases", C.c_int64), ("padded_bases", C.c_int64),
                ("overlap_bases", C.c_int64), ("disagree", C.c_int64), ("from2", C.c_int64), ("ties", C.c_int64),
                ("n_filled", C.c_int64), ("n_both", C.c_int64), ("corrected", C.c_int64 * 2)]


class PpgKmerCount(C.Structure):
    """ppg_kmer_count (include/ppgpu.h)."""
    _fields_ = [("flags", C.c_int64), ("k", C.c_int64), ("reserved", C.c_int64 * 6)]


class PpgKmerCountResult(C.Structure):
    """ppg_kmer_count_result (include/ppgpu.h)."""
    _fields_ = [("records", C.c_int64), ("participating", C.c_int64), ("short_reads", C.c_int64), ("bases", C.c_int64),
                ("positions", C.c_int64), ("kmers", C.c_int64), ("invalid", C.c_int64), ("distinct", C.c_int64),
                ("singletons", C.c_int64), ("max_count", C.c_int64), ("max_key", C.c_int64), ("total_count", C.c_int64),
                ("overflow", C.c_int64), ("reserved", C.c_int64 * 3)]


PPG_KMER_CANONICAL, PPG_KMER_USE_WINDOWS, PPG_KMER_USE_MASK, PPG_KMER_ACCUMULATE, PPG_KMER_SPECTRUM = 1, 2, 4, 8, 1024


for _name, (_res, _args) in _SIGS.items():
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args

EXPORTED = sorted(_SIGS)

_synth = None


def synth():
    """libppgsynth.so: synthetic Generator-shape FASTQ and gzip (tests / bench input only)."""
    global _synth
    if _synth is None:
        s = _load(SYNTH_PATH, "libppgsynth.so")
        s.ppg_synth_fastq_size.restype = i64
        s.ppg_synth_fastq_size.argtypes = [i64, i64, C.c_int]
        s.ppg_synth_fastq.restype = i64
        s.ppg_synth_fastq.argtypes = [C.c_uint64, i64, i64, C.c_int, vp, i64, C.c_int]
        s.ppg_synth_fastq_size_mate.restype = i64
        s.ppg_synth_fastq_size_mate.argtypes = [i64, i64, C.c_int, C.c_int]
        s.ppg_synth_fastq_mate.restype = i64
        s.ppg_synth_fastq_mate.argtypes = [C.c_uint64, C.c_int, i64, i64, C.c_int, vp, i64, C.c_int]
        s.ppg_synth_illumina_size.restype = i64
        s.ppg_synth_illumina_size.argtypes = [C.c_uint64, i64, i64]
        s.ppg_synth_illumina.restype = i64
        s.ppg_synth_illumina.argtypes = [C.c_uint64, i64, i64, vp, i64, C.c_int]
        s.ppg_synth_gzip.restype = i64
        s.ppg_synth_gzip.argtypes = [vp, i64, C.c_int, i64, C.c_int, vp, i64]
        s.ppg_synth_segment.restype = i64
        s.ppg_synth_segment.argtypes = [vp, i64, C.c_int, i64, C.c_int, vp, i64, P(C.c_uint32)]
        s.ppg_synth_segment_pieces.restype = i64
        s.ppg_synth_segment_pieces.argtypes = [vp, i64, C.c_int, i64, C.c_int, vp, i64, P(C.c_uint32), vp, i64]
        s.ppg_synth_segment_blocks_pieces.restype = i64
        s.ppg_synth_segment_blocks_pieces.argtypes = [vp, vp, i64, vp, i64, i64, C.c_int, vp, vp, i64]
        s.ppg_synth_tiled_frame.restype = None
        s.ppg_synth_tiled_frame.argtypes = [C.c_uint32, i64, i64, vp, vp]
        s.ppg_synth_segment_blocks.restype = i64
        s.ppg_synth_segment_blocks.argtypes = [vp, i64, i64, vp, vp, i64]
        s.ppg_synth_tiled_points.restype = i64
        s.ppg_synth_tiled_points.argtypes = [vp, i64, i64, i64, vp, vp, i64, u32, vp, vp, vp, vp, vp, i64]
        s.ppg_synth_tiled_fill.restype = None
        s.ppg_synth_tiled_fill.argtypes = [vp, i64, vp, vp, vp, i64, i64, vp, vp]
        _synth = s
    return _synth
