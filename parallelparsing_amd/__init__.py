"""parallelparsing_amd — MI355X-native chunked-gzip FASTQ DecompressAll.

Host-side mirror of the reference's API surface (names, argument meaning, error behaviour) over
the C ABI of libppgpu.so (include/ppgpu.h):

  Core.BuildDeflateIndex(path_or_bytes, chunksize)        Decompressor/Core.cs:14-131 (CreateIndex)
  Core.ExtractDeflateIndex(file_buffer, index, k, buf)     Decompressor/Core.cs:133-192 (Decompress)
  Parsing.Parse(chunk)                                     Decompressor/Parsing.cs:11-51
  IndexIO.Serialize(index, path) / IndexIO.Deserialize    Common/IndexIO.cs:7-53
  BatchedFASTQ(index_or_path, gzip_path, ssd)              Decompressor/BatchedFASTQ.cs:10-101 (DecompressAll)
  FastqRecord / Index / Point                              Common/FastqRecord.cs, Common/Index.cs

Errors raise PpgError (the ZException of Interop/Conventions.cs:33-41) carrying the ZResult code.
The decode runs only on the GPU; there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from ._lib import lib, check, PpgError, PPG_NO_DEVICE, PPG_STREAM_END, PpgBatch, synth  # noqa: F401
from . import _lib

WINSIZE = 32768
CHUNK = 16384


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class Point:
    """Common/Index.cs:51-82 (read-only view)."""

    __slots__ = ("Output", "Input", "Bits", "Window", "offset")

    def __init__(self, output, inp, bits, window, offset):
        self.Output, self.Input, self.Bits, self.Window, self.offset = output, inp, bits, window, offset

    def __repr__(self):
        return f"Point(Output={self.Output}, Input={self.Input}, Bits={self.Bits}, |offset|={len(self.offset)})"


class Index:
    """Common/Index.cs: the checkpoint list, owned by libppgpu (ppg_index)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:   # (lib is None at interpreter exit)
            lib.ppg_index_free(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def Count(self):
        return lib.ppg_index_count(self._h)

    def __len__(self):
        return self.Count

    @property
    def ChunkMaxBytes(self):
        return lib.ppg_index_chunk_max_bytes(self._h)

    def point_fields(self, i):
        o, n, b, ol = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(lib.ppg_index_point(self._h, i, C.byref(o), C.byref(n), C.byref(b), C.byref(ol)), "Index[i]")
        return o.value, n.value, b.value, ol.value

    def __getitem__(self, i):
        if i < 0:
            i += self.Count
        o, n, b, ol = self.point_fields(i)
        w = C.string_at(lib.ppg_index_window(self._h, i), WINSIZE)
        off = C.string_at(lib.ppg_index_offset(self._h, i), ol) if ol else b""
        return Point(o, n, b, w, off)

    def validate(self, first=0, n=None):
        """ppg_index_validate: raises PpgError(PPG_UNSUPPORTED) if a chunk of [first, first+n) is
        too large for the decode kernels (output >= 2^31 bytes, or >= 2^32 - 2^12 compressed bits)."""
        if n is None:
            n = self.Count - 1 - first
        check(lib.ppg_index_validate(self._h, int(first), int(n)), "Index.validate")
        return self

    def arrays(self):
        """(output, input, bits) int64 numpy arrays over all points."""
        n = self.Count
        out = np.empty(n, np.int64)
        inp = np.empty(n, np.int64)
        bits = np.empty(n, np.int64)
        for i in range(n):
            out[i], inp[i], bits[i], _ = self.point_fields(i)
        return out, inp, bits

    def windows_array(self):
        """All Point windows as one uint8 array (Count * 32768; the index stores them contiguously)."""
        n = self.Count
        if n == 0:
            return np.zeros(0, np.uint8)
        return np.frombuffer(C.string_at(lib.ppg_index_window(self._h, 0), n * WINSIZE), np.uint8)

    def set_side_points(self, bits, outputs, windows):
        """Attach side points (inner deflate block starts: absolute bit, output offset, the 32 KiB
        before each) found by the host, as BuildDeflateIndexGpu(side_bytes=...) records them
        (ppg_index_set_side_points)."""
        b, o = np.ascontiguousarray(bits, np.int64), np.ascontiguousarray(outputs, np.int64)
        w = np.ascontiguousarray(windows, np.uint8)
        assert w.size == 32768 * b.size and o.size == b.size
        check(lib.ppg_index_set_side_points(self._h, b.size, _ptr(b), _ptr(o), _ptr(w)), "ppg_index_set_side_points")
        return self

    def side_points(self, first=0, n=None):
        """(bits, outputs, windows) of the side points BuildDeflateIndexGpu(side_bytes=...) recorded,
        those inside chunks [first, first+n) (a Shard's range) -- Shard.set_split's arguments."""
        m = lib.ppg_index_side_count(self._h)
        bits, outs = np.zeros(max(1, m), np.int64), np.zeros(max(1, m), np.int64)
        win = np.zeros(max(1, m) * 32768, np.uint8)
        check(lib.ppg_index_side_points(self._h, _ptr(bits), _ptr(outs), _ptr(win)), "side_points")
        if n is None:
            n = self.Count - 1 - first
        lo, hi = self.point_fields(first)[0], self.point_fields(first + n)[0]
        keep = np.nonzero((outs[:m] > lo) & (outs[:m] < hi))[0]
        return bits[keep], outs[keep], win.reshape(-1, 32768)[keep].ravel()

    @staticmethod
    def from_points(output, inp, bits, windows, offset_len, offsets, chunk_max_bytes=0):
        """Index from arrays (ppg_index_from_points): windows is count*32768 bytes."""
        output = np.ascontiguousarray(output, np.int64)
        inp = np.ascontiguousarray(inp, np.int64)
        bits = np.ascontiguousarray(bits, np.int32)
        windows = np.ascontiguousarray(windows, np.uint8)
        offset_len = np.ascontiguousarray(offset_len, np.int32)
        offsets = np.ascontiguousarray(offsets, np.uint8) if len(offsets) else np.zeros(1, np.uint8)
        h = C.c_void_p()
        check(lib.ppg_index_from_points(len(output), _ptr(output), _ptr(inp), _ptr(bits), _ptr(windows),
                                        _ptr(offset_len), _ptr(offsets), int(chunk_max_bytes), C.byref(h)),
              "Index.from_points")
        return Index(h.value)


class IndexIO:
    """Common/IndexIO.cs."""

    @staticmethod
    def Serialize(index, path):
        check(lib.ppg_index_serialize(index.handle, os.fsencode(path)), "IndexIO.Serialize")

    @staticmethod
    def Deserialize(path):
        h = C.c_void_p()
        check(lib.ppg_index_deserialize(os.fsencode(path), C.byref(h)), "IndexIO.Deserialize")
        return Index(h.value)


class Device:
    """One GPU context (ppg_ctx): a HIP stream on an MI355X."""

    _default = {}

    def __init__(self, device=0):
        h = C.c_void_p()
        check(lib.ppg_open(int(device), C.byref(h)), f"ppg_open({device})")
        self._h = h
        self.device = device
        self._users = 0          # live Shards / Cursors: their ppg_*_free reads this ctx
        self._dropped = False

    def __del__(self):
        # The cyclic collector finalises a Device and the Shards that refer to it in any order (a
        # traceback that holds them is such a cycle), and ppg_shard_free / ppg_cursor_close read the
        # ctx: the ctx is closed by whichever goes last.
        self._dropped = True
        if getattr(self, "_users", 0) == 0:
            self._close()

    def _close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:   # (lib is None at interpreter exit)
            lib.ppg_close(h)
            self._h = None

    def _retain(self):
        self._users += 1

    def _release(self):
        self._users -= 1
        if self._users == 0 and self._dropped:
            self._close()

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return lib.ppg_ctx_stream(self._h)

    def wait_stream(self, stream):
        """Order this ctx's later work after everything queued on `stream` (a hipStream_t handle, or
        a torch.cuda.Stream) so far -- ppg_ctx_wait_stream, no host drain."""
        check(lib.ppg_ctx_wait_stream(self._h, C.c_void_p(_stream_handle(stream))), "ppg_ctx_wait_stream")

    def stream_wait(self, stream):
        """Order `stream`'s later work after everything queued on this ctx so far (ppg_stream_wait_ctx)."""
        check(lib.ppg_stream_wait_ctx(self._h, C.c_void_p(_stream_handle(stream))), "ppg_stream_wait_ctx")

    def release_file_buffers(self):
        """Free what decompress_file keeps in this ctx between calls (ppg_file_release): its device
        pieces and their shards' outputs, the pinned staging; the next call allocates them again."""
        check(lib.ppg_file_release(self._h), "ppg_file_release")

    def decompress_chunk_stats(self):
        """{calls, launches, max_batch, split_chunks, side_points} of ppg_decompress_chunk on this
        ctx: how the thread-safe per-chunk Decompress combined concurrent calls into launches, and
        how many chunks it split at inner block starts it found on the GPU."""
        v = [C.c_int64() for _ in range(5)]
        check(lib.ppg_decompress_chunk_stats(self._h, *[C.byref(x) for x in v[:3]]), "ppg_decompress_chunk_stats")
        check(lib.ppg_decompress_chunk_split_stats(self._h, *[C.byref(x) for x in v[3:]]),
              "ppg_decompress_chunk_split_stats")
        return dict(zip(("calls", "launches", "max_batch", "split_chunks", "side_points"), (x.value for x in v)))

    def after_torch(self):
        """wait_stream(torch's current stream on this device): call before a ppg call reads device
        memory torch's stream writes, or writes memory it may still read."""
        import torch
        self.wait_stream(torch.cuda.current_stream(torch.device("cuda", self.device)))

    @classmethod
    def default(cls, device=None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        if device not in cls._default:
            cls._default[device] = cls(device)
        return cls._default[device]


def _stream_handle(stream):
    if stream is None:
        return 0
    return int(getattr(stream, "cuda_stream", stream))


def device_count():
    n = C.c_int(0)
    lib.ppg_device_count(C.byref(n))
    return n.value


class FastqRecord:
    """Common/FastqRecord.cs: Identifier, Sequence, Other, Quality (bytes fields, lazy str)."""

    __slots__ = ("raw", "start", "n1", "n2", "n3", "n4")

    def __init__(self, raw, start, n1, n2, n3, n4):
        self.raw, self.start, self.n1, self.n2, self.n3, self.n4 = raw, start, n1, n2, n3, n4

    # field slices exactly as Parsing.cs:37-40
    @property
    def identifier(self):
        return bytes(self.raw[self.start + 1:self.n1])

    @property
    def sequence(self):
        return bytes(self.raw[self.n1 + 1:self.n2])

    @property
    def other(self):
        return bytes(self.raw[self.n2 + 2:self.n3])

    @property
    def quality(self):
        return bytes(self.raw[self.n3 + 1:self.n4])

    Identifier = property(lambda s: s.identifier.decode("ascii", "replace"))
    Sequence = property(lambda s: s.sequence.decode("ascii", "replace"))
    Other = property(lambda s: s.other.decode("ascii", "replace"))
    Quality = property(lambda s: s.quality.decode("ascii", "replace"))

    def __repr__(self):
        return f"FastqRecord({self.identifier!r})"


class TrimmedRecord(FastqRecord):
    """A FastqRecord with the window a read trim left of it (include/ppgpu.h "read trimming"):
    trimmed_sequence = Sequence[start, start + len), trimmed_quality = Quality[start, start + len)."""

    __slots__ = ("trim_start", "trim_len")

    def __init__(self, raw, start, n1, n2, n3, n4, trim_start, trim_len):
        super().__init__(raw, start, n1, n2, n3, n4)
        self.trim_start, self.trim_len = trim_start, trim_len

    @property
    def trimmed_sequence(self):
        a = self.n1 + 1 + self.trim_start
        return bytes(self.raw[a:a + self.trim_len])

    @property
    def trimmed_quality(self):
        a = self.n3 + 1 + self.trim_start
        return bytes(self.raw[a:min(a + self.trim_len, self.n4)])


def records_from_descriptors(raw, desc):
    """FastqRecords of one chunk from its (n,4) uint32 descriptors over raw = offset ++ chunk."""
    recs = []
    start = 0
    for n1, n2, n3, n4 in np.asarray(desc).reshape(-1, 4).tolist():
        recs.append(FastqRecord(raw, start, n1, n2, n3, n4))
        start = n4 + 1
    return recs


class Parsing:
    """Decompressor/Parsing.cs — the GPU record scan runs inside Core/Shard; this helper rebuilds
    FastqRecord objects from its descriptors."""

    @staticmethod
    def Parse(offset, chunk, desc):
        raw = bytes(offset or b"") + bytes(chunk)
        return records_from_descriptors(raw, desc)


def _as_u8(buf):
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf, np.uint8)
    return np.frombuffer(bytes(buf), np.uint8)


class Core:
    """Decompressor/Core.cs."""

    @staticmethod
    def BuildDeflateIndex(gz, chunksize):
        """CreateIndex over a path or in-memory .gz bytes (Core.cs:14-131)."""
        h = C.c_void_p()
        if isinstance(gz, (str, os.PathLike)):
            check(lib.ppg_index_build_file(os.fsencode(gz), int(chunksize) & 0xFFFFFFFF, C.byref(h)),
                  "Core.BuildDeflateIndex")
        else:
            a = _as_u8(gz)
            check(lib.ppg_index_build_mem(_ptr(a), a.size, int(chunksize) & 0xFFFFFFFF, C.byref(h)),
                  "Core.BuildDeflateIndex")
        return Index(h.value)

    @staticmethod
    def BuildDeflateIndexGpu(gz, chunksize, device=None, piece_bytes=0, out_capacity=0, side_bytes=0):
        """CreateIndex on the GPU (ppg_index_gpu.cpp): the same Points as BuildDeflateIndex for a
        single-member gzip, from a block-parallel decode.  gz: a path, bytes / uint8 array (host),
        or a uint8 torch tensor on the device.  Raises PpgError(PPG_UNSUPPORTED) for zlib-wrapped
        or multi-member input (BuildDeflateIndex handles those).  side_bytes > 0 (in-memory input)
        also records side points every >= side_bytes of output inside chunks (Index.side_points,
        for Shard.set_split)."""
        dev = device or Device.default()
        h = C.c_void_p()
        cs = int(chunksize) & 0xFFFFFFFF
        if isinstance(gz, (str, os.PathLike)):
            if side_bytes:
                raise ValueError("side_bytes needs the member in memory (host or device)")
            rc = lib.ppg_index_build_gpu_file(dev.handle, os.fsencode(gz), cs, int(piece_bytes), C.byref(h))
        elif hasattr(gz, "data_ptr"):
            import torch
            if not (gz.is_cuda and gz.dtype == torch.uint8 and gz.is_contiguous() and gz.dim() == 1):
                raise ValueError("BuildDeflateIndexGpu: a device tensor must be a contiguous 1-D uint8 CUDA tensor")
            if gz.data_ptr() % 4:
                raise ValueError("BuildDeflateIndexGpu: a device tensor must be 4-byte aligned")
            # the block finder and the inflate reader fetch whole 4-byte words and read ahead: bytes
            # past gz_len may be read (never used), so they must be mapped -- torch's caching
            # allocator rounds every block up to 512 B; ppgpu.h documents the requirement
            dev.wait_stream(torch.cuda.current_stream(gz.device))   # our stream reads what torch's wrote
            rc = lib.ppg_index_build_gpu_side(dev.handle, C.c_void_p(gz.data_ptr()), gz.numel(), 1, cs,
                                              int(piece_bytes), int(out_capacity), int(side_bytes), C.byref(h))
        else:
            a = _as_u8(gz)
            rc = lib.ppg_index_build_gpu_side(dev.handle, _ptr(a), a.size, 0, cs, int(piece_bytes),
                                              int(out_capacity), int(side_bytes), C.byref(h))
        check(rc, "Core.BuildDeflateIndexGpu")
        return Index(h.value)

    GPU_INDEX_STATS = ("finder_ms", "pass1_ms", "chain_ms", "pass2_ms", "census_ms", "total_ms", "pieces",
                       "real_pieces", "redo1", "resolve_ms", "batches", "blocks", "points", "output_bytes",
                       "upload_ms", "pass2_alloc_ms", "spec_redos", "serial_redos")

    @staticmethod
    def gpu_index_stats(device=None):
        """Timings and counts of the last BuildDeflateIndexGpu on a device (ppg_index_build_gpu_stats)."""
        dev = device or Device.default()
        v = (C.c_double * len(Core.GPU_INDEX_STATS))()
        check(lib.ppg_index_build_gpu_stats(dev.handle, v, len(v)), "ppg_index_build_gpu_stats")
        return dict(zip(Core.GPU_INDEX_STATS, list(v)))

    @staticmethod
    def ExtractDeflateIndex(file_buffer, index, k, buf=None, device=None, with_records=False):
        """Decompress checkpoint k (Core.cs:133-192) on the GPU.  file_buffer = file bytes
        [Index[k].Input-1, Index[k+1].Input-1].  Returns the produced byte count written into buf
        (allocated if None) — and the (n,4) record descriptors if with_records.  Thread safe, as
        README.md:38-50 requires: concurrent calls on one Device share launches
        (ppg_decompress_chunk; ctypes releases the GIL for the call)."""
        dev = device or Device.default()
        src = _as_u8(file_buffer)
        o0, _, _, _ = index.point_fields(k)
        o1, _, _, _ = index.point_fields(k + 1)
        need = max(0, o1 - o0)
        if buf is None:
            buf = np.empty(need, np.uint8)   # every produced byte is written
        produced = C.c_int64()
        nrec = C.c_int64()
        # descriptor rows for >= 64-B records (a FASTQ record is hundreds); a chunk of smaller ones
        # reports its record count with PPG_BUF_ERROR and is decoded again into an exact table
        # (r05: rows for 4-B records made every call zero 4x its output bytes in the allocator)
        recs = np.empty((_rec_rows(need), 4), np.uint32) if with_records else None
        rc = lib.ppg_decompress_chunk(dev.handle, index.handle, int(k), _ptr(src), src.size, _ptr(buf), buf.size,
                                      C.byref(produced), _ptr(recs), recs.shape[0] if with_records else 0,
                                      C.byref(nrec))
        if with_records and rc == _lib.PPG_BUF_ERROR and nrec.value > recs.shape[0]:
            recs = np.empty((nrec.value, 4), np.uint32)
            rc = lib.ppg_decompress_chunk(dev.handle, index.handle, int(k), _ptr(src), src.size, _ptr(buf), buf.size,
                                          C.byref(produced), _ptr(recs), recs.shape[0], C.byref(nrec))
        check(rc, "Core.ExtractDeflateIndex")
        if with_records:
            return produced.value, buf, recs[:nrec.value]
        return produced.value, buf

    @staticmethod
    def ExtractDeflateIndexAsync(file_buffer, index, k, buf=None, device=None):
        """ExtractDeflateIndex queued without blocking (ppg_decompress_chunk_submit): returns a
        ChunkFuture whose result() is (produced, buf, records).  Many queued chunks share launches
        of up to 256 chunks; every future's result() must be taken (it frees the ticket)."""
        dev = device or Device.default()
        src = _as_u8(file_buffer)
        o0, _, _, _ = index.point_fields(k)
        o1, _, _, _ = index.point_fields(k + 1)
        need = max(0, o1 - o0)
        if buf is None:
            buf = np.empty(need, np.uint8)
        recs = np.empty((_rec_rows(need), 4), np.uint32)   # (too few: result() decodes it again)
        t = C.c_void_p()
        check(lib.ppg_decompress_chunk_submit(dev.handle, index.handle, int(k), _ptr(src), src.size, _ptr(buf), buf.size,
                                              _ptr(recs), recs.shape[0], C.byref(t)), "ppg_decompress_chunk_submit")
        return ChunkFuture(dev, t, (src, buf, recs, index, k))


def _rec_rows(nbytes):
    """Descriptor rows to offer for a chunk of nbytes of text: enough for records of >= 64 bytes."""
    return int(nbytes) // 64 + 256


class ChunkFuture:
    """A queued ExtractDeflateIndexAsync: result() waits (ppg_decompress_chunk_wait) -- once."""

    def __init__(self, dev, ticket, keep):
        self._dev, self._t, self._keep, self._res = dev, ticket, keep, None

    def result(self):
        if self._res is None:
            produced, nrec = C.c_int64(), C.c_int64()
            t, self._t = self._t, None
            if t is None:
                raise RuntimeError("ChunkFuture waited twice")
            rc = lib.ppg_decompress_chunk_wait(self._dev.handle, t, C.byref(produced), C.byref(nrec))
            src, buf, recs, index, k = self._keep
            self._keep = None
            if rc == _lib.PPG_BUF_ERROR and nrec.value > recs.shape[0]:   # records under 64 B: once more, exactly
                self._res = Core.ExtractDeflateIndex(src, index, k, buf=buf, device=self._dev, with_records=True)
                return self._res
            check(rc, "Core.ExtractDeflateIndexAsync")
            self._res = (produced.value, buf, recs[:nrec.value])
        return self._res

    def __del__(self):
        if getattr(self, "_t", None) is not None:   # never waited: wait now (the buffers must outlive it)
            try:
                self.result()
            except Exception:   # noqa: BLE001 - a finaliser must not raise
                pass


class PackedReads:
    """A packed read set (include/ppgpu.h "packed reads"): seq_off (int64, records + 1, in bases),
    seq_len (records), bases (2 bits per base, 16 per word), mask (1 bit per base: not ACGT) and
    qual (one byte per base, or None); every record starts on a 32-base unit.  The arrays are
    either CUDA tensors on one device (int64; int32 views of the uint32 words; uint8) or numpy
    arrays (int64, uint32, uint8).  sequence(j) / quality(j) read host arrays."""

    _CODES = np.frombuffer(b"ACGT", np.uint8)

    def __init__(self, seq_off, seq_len, bases, mask, qual=None, records=None, total_bases=None):
        self.seq_off, self.seq_len, self.bases, self.mask, self.qual = seq_off, seq_len, bases, mask, qual
        self.records = int(records) if records is not None else int(seq_len.shape[0])
        self.total_bases = None if total_bases is None else int(total_bases)

    @classmethod
    def empty(cls, rec_cap, base_cap, quality=True, device=None):
        """Planes for rec_cap records and base_cap bases (rounded up to a multiple of 32): CUDA
        tensors on `device` (an int or torch.device), numpy arrays when device is None."""
        rec_cap, base_cap = int(rec_cap), (int(base_cap) + 31) // 32 * 32
        if device is None:
            return cls(np.zeros(rec_cap + 1, np.int64), np.zeros(rec_cap, np.uint32), np.zeros(base_cap // 16, np.uint32),
                       np.zeros(base_cap // 32, np.uint32), np.zeros(base_cap, np.uint8) if quality else None)
        import torch
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        mk = lambda n, dt: torch.zeros(max(int(n), 1), dtype=dt, device=dev)[:int(n)]   # noqa: E731
        return cls(mk(rec_cap + 1, torch.int64), mk(rec_cap, torch.int32), mk(base_cap // 16, torch.int32),
                   mk(base_cap // 32, torch.int32), mk(base_cap, torch.uint8) if quality else None)

    @property
    def on_device(self):
        return hasattr(self.seq_off, "data_ptr")

    @property
    def rec_cap(self):
        return int(self.seq_len.shape[0])

    @property
    def base_cap(self):
        return 32 * int(self.mask.shape[0])

    def _check_device(self, what):
        import torch
        planes = [self.seq_off, self.seq_len, self.bases, self.mask] + ([self.qual] if self.qual is not None else [])
        dts = [torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8]
        for t, dt in zip(planes, dts):
            if not (hasattr(t, "data_ptr") and t.is_cuda and t.dtype == dt and t.is_contiguous()):
                raise ValueError(f"{what}: the planes must be contiguous CUDA tensors (int64, int32 words, uint8)")
        if self.seq_off.numel() != self.rec_cap + 1 or self.bases.numel() != 2 * self.mask.numel() or \
                (self.qual is not None and self.qual.numel() != self.base_cap):
            raise ValueError(f"{what}: plane sizes do not agree (PackedReads.empty makes them)")

    def _ptrs(self):
        return (C.c_void_p(self.seq_off.data_ptr()), C.c_void_p(self.seq_len.data_ptr()), self.rec_cap,
                C.c_void_p(self.bases.data_ptr()), C.c_void_p(self.mask.data_ptr()),
                C.c_void_p(self.qual.data_ptr()) if self.qual is not None else None, self.base_cap)

    def to_host(self):
        """The same read set as numpy arrays (a copy; uint32 words), cut to its records and bases
        when they are known."""
        if not self.on_device:
            return self
        off = self.seq_off.cpu().numpy()
        nb = self.total_bases if self.total_bases is not None else self.base_cap
        nr = self.records
        w = lambda t, n: t.cpu().numpy().view(np.uint32)[:n].copy()   # noqa: E731
        return PackedReads(off[:nr + 1].copy(), w(self.seq_len, nr), w(self.bases, nb // 16), w(self.mask, nb // 32),
                           self.qual.cpu().numpy()[:nb].copy() if self.qual is not None else None, nr, nb)

    def _span(self, j):
        if self.on_device:
            raise ValueError("PackedReads: sequence / quality read host arrays (to_host() first)")
        return int(self.seq_off[j]), int(self.seq_len[j])

    def sequence(self, j):
        """Record j's Sequence as bytes, every masked position as 'N'."""
        b, L = self._span(j)
        if L == 0:
            return b""
        P = (L + 31) // 32 * 32
        words = np.asarray(self.bases[b >> 4:(b + P) >> 4], np.uint32)
        codes = ((words[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)[:L]
        mw = np.asarray(self.mask[b >> 5:(b + P) >> 5], np.uint32)
        m = ((mw[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:L]
        s = self._CODES[codes]
        s[m != 0] = ord("N")
        return s.tobytes()

    def quality(self, j):
        """Record j's quality bytes (the Quality string cut or zero-filled to the sequence's length)."""
        if self.qual is None:
            raise ValueError("PackedReads: no quality plane")
        b, L = self._span(j)
        return np.asarray(self.qual[b:b + L], np.uint8).tobytes()


def _pattern_arg(pattern):
    """(pointer argument, length) of a query pattern: bytes, str (ASCII) or None / empty for none."""
    if pattern is None:
        return None, 0
    b = pattern.encode("ascii") if isinstance(pattern, str) else bytes(pattern)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0"), len(b)


class SeqQuery:
    """The result of a sequence query (include/ppgpu.h "sequence queries"): `records` scanned, `hits`
    (records whose Sequence contains the pattern; all of them without a pattern), `bases` (the sum of
    the Sequence lengths), `counts` (bytes 'A' 'C' 'G' 'T' and every other byte over all Sequences),
    `chunk_hits` (numpy int64, hits per chunk of the shard) and `hit_mask`: a uint32 CUDA tensor with
    bit j & 31 of word j >> 5 set iff shard record j is a hit, or None when no mask was asked for."""

    CLASSES = ("A", "C", "G", "T", "other")

    def __init__(self, result, chunk_hits, hit_mask=None):
        self.records, self.hits, self.bases = int(result.records), int(result.hits), int(result.bases)
        self.counts = {c: int(v) for c, v in zip(self.CLASSES, result.count)}
        self.chunk_hits = chunk_hits
        self.hit_mask = hit_mask

    def hit_records(self):
        """The shard record numbers of the hits, ascending: an int64 tensor on the mask's device."""
        if self.hit_mask is None:
            raise ValueError("SeqQuery.hit_records: the query was made without a mask")
        import torch
        w = self.hit_mask.view(torch.int32)[:(self.records + 31) // 32]
        bit = torch.arange(32, dtype=torch.int32, device=w.device)
        return ((w[:, None] >> bit) & 1).reshape(-1).nonzero().reshape(-1)

    def __repr__(self):
        return f"SeqQuery(records={self.records}, hits={self.hits}, bases={self.bases}, counts={self.counts})"


class ReadFilter:
    """A quality-control filter over records (include/ppgpu.h "read filters"); a criterion left at None
    is not applied.  min_length / max_length bound the Sequence length; max_n the Sequence bytes that are
    not A C G T; min_mean_quality the mean of the Quality bytes above quality_base; low_quality and
    max_low_fraction go together: at most that fraction of the Quality bytes may lie below low_quality.
    The two real-valued thresholds are held as round(1000 * x), the comparisons are exact integers."""

    def __init__(self, min_length=0, max_length=None, max_n=None, min_mean_quality=None, low_quality=None,
                 max_low_fraction=None, quality_base=33):
        if (low_quality is None) != (max_low_fraction is None):
            raise ValueError("ReadFilter: low_quality and max_low_fraction go together")
        self.min_length, self.max_length, self.max_n = min_length, max_length, max_n
        self.min_mean_quality, self.low_quality, self.max_low_fraction = min_mean_quality, low_quality, max_low_fraction
        self.quality_base = quality_base

    def struct(self, and_mask=False):
        """The ppg_read_filter of this filter (and_mask: with the AND_MASK bit); ValueError when
        ppg_read_filter_check refuses it."""
        crit = 0
        if self.min_length or self.max_length is not None:
            crit |= _lib.PPG_FILTER_LENGTH
        if self.max_n is not None:
            crit |= _lib.PPG_FILTER_OTHER
        if self.min_mean_quality is not None:
            crit |= _lib.PPG_FILTER_MEAN
        if self.low_quality is not None:
            crit |= _lib.PPG_FILTER_LOW
        if and_mask:
            crit |= _lib.PPG_FILTER_AND_MASK
        f = _lib.PpgReadFilter(
            crit, int(self.min_length), -1 if self.max_length is None else int(self.max_length),
            0 if self.max_n is None else int(self.max_n), int(self.quality_base),
            0 if self.min_mean_quality is None else int(round(1000 * self.min_mean_quality)),
            0 if self.low_quality is None else int(self.low_quality),
            0 if self.max_low_fraction is None else int(round(1000 * self.max_low_fraction)))
        if lib.ppg_read_filter_check(C.byref(f)) != 0:
            raise ValueError(f"ReadFilter: not a valid filter: {self!r}")
        return f

    def __repr__(self):
        return (f"ReadFilter(min_length={self.min_length}, max_length={self.max_length}, max_n={self.max_n}, "
                f"min_mean_quality={self.min_mean_quality}, low_quality={self.low_quality}, "
                f"max_low_fraction={self.max_low_fraction}, quality_base={self.quality_base})")


def _filter_struct(flt, and_mask=False):
    """The ppg_read_filter of a ReadFilter, or a _lib.PpgReadFilter as it is (its AND_MASK bit set on demand)."""
    if isinstance(flt, ReadFilter):
        return flt.struct(and_mask)
    if not isinstance(flt, _lib.PpgReadFilter):
        raise ValueError("expected a ReadFilter")
    f = _lib.PpgReadFilter.from_buffer_copy(flt)
    if and_mask:
        f.criteria |= _lib.PPG_FILTER_AND_MASK
    return f


class ReadFilterResult:
    """The result of a read filter (include/ppgpu.h "read filters"): `records` measured, `passed`,
    `failed` (records failing each criterion on its own, by 'length', 'n', 'mean_quality',
    'low_quality'), `bases`, `other` (Sequence bytes that are not A C G T), `qual_bytes`, `qual_count`
    (numpy int64[256]: the Quality bytes by value), `chunk_passed` (numpy int64, passes per chunk) and,
    when asked for, `pass_mask` (a uint32 CUDA tensor in the hit-mask format) and `metrics` (a uint8
    CUDA tensor of 24-byte rows, see metrics_host)."""

    CRITERIA = ("length", "n", "mean_quality", "low_quality")
    METRICS_DTYPE = np.dtype([("length", "<u4"), ("other", "<u4"), ("qual_length", "<u4"), ("low", "<u4"),
                              ("qual_sum", "<u8")])

    def __init__(self, result, chunk_passed=None, pass_mask=None, metrics=None):
        self.records, self.passed = int(result.records), int(result.passed)
        self.failed = {c: int(v) for c, v in zip(self.CRITERIA, result.failed)}
        self.bases, self.other, self.qual_bytes = int(result.bases), int(result.other), int(result.qual_bytes)
        self.qual_count = np.array(result.qual_count, np.int64)
        self.chunk_passed = chunk_passed
        self.pass_mask = pass_mask
        self.metrics = metrics

    def pass_records(self):
        """The shard record numbers of the set mask bits, ascending: an int64 tensor on the mask's device."""
        if self.pass_mask is None:
            raise ValueError("ReadFilterResult.pass_records: the filter was run without a mask")
        import torch
        w = self.pass_mask.view(torch.int32)[:(self.records + 31) // 32]
        bit = torch.arange(32, dtype=torch.int32, device=w.device)
        return ((w[:, None] >> bit) & 1).reshape(-1).nonzero().reshape(-1)

    def metrics_host(self):
        """The metrics rows of the records as a numpy structured array (length, other, qual_length, low, qual_sum)."""
        if self.metrics is None:
            raise ValueError("ReadFilterResult.metrics_host: the filter was run without metrics")
        import torch
        raw = self.metrics.view(torch.uint8).reshape(-1)[:24 * self.records].cpu().numpy()
        return raw.view(self.METRICS_DTYPE)

    def __repr__(self):
        return (f"ReadFilterResult(records={self.records}, passed={self.passed}, failed={self.failed}, "
                f"bases={self.bases}, other={self.other}, qual_bytes={self.qual_bytes})")


class ReadTrim:
    """A read trim (include/ppgpu.h "read trimming"); a cut left at None is not applied.  head / tail
    bases are cut from the ends in any case; leading_quality / trailing_quality cut the bases below that
    quality from the 5' / 3' end; window=(size, quality) cuts from the first full window whose mean quality
    is below `quality`; adapter (bytes) cuts from the leftmost 3' adapter site of at least min_overlap
    bases with at most max_error_rate mismatches (held as round(1000 * x), compared as exact integers).
    Every cut is decided on the read after head / tail alone, not on the others' results.  A read is
    kept when min_length bases are left."""

    def __init__(self, head=0, tail=0, leading_quality=None, trailing_quality=None, window=None, adapter=None,
                 min_overlap=3, max_error_rate=0.1, min_length=0, quality_base=33):
        if window is not None and len(tuple(window)) != 2:
            raise ValueError("ReadTrim: window is (size, quality)")
        self.head, self.tail = head, tail
        self.leading_quality, self.trailing_quality = leading_quality, trailing_quality
        self.window = None if window is None else tuple(window)
        self.adapter = None if adapter is None else (adapter.encode("ascii") if isinstance(adapter, str) else bytes(adapter))
        self.min_overlap, self.max_error_rate = min_overlap, max_error_rate
        self.min_length, self.quality_base = min_length, quality_base

    def struct(self, and_mask=False):
        """The ppg_read_trim of this trim (and_mask: with the AND_MASK bit); ValueError when
        ppg_read_trim_check refuses it."""
        ops = 0
        if self.leading_quality is not None:
            ops |= _lib.PPG_TRIM_LEADING
        if self.trailing_quality is not None:
            ops |= _lib.PPG_TRIM_TRAILING
        if self.window is not None:
            ops |= _lib.PPG_TRIM_WINDOW
        if self.adapter is not None:
            ops |= _lib.PPG_TRIM_ADAPTER
        if and_mask:
            ops |= _lib.PPG_TRIM_AND_MASK
        ad = self.adapter or b""
        if len(ad) > 64:
            raise ValueError("ReadTrim: an adapter has at most 64 bytes")
        t = _lib.PpgReadTrim(
            ops, int(self.head), int(self.tail), int(self.quality_base),
            0 if self.leading_quality is None else int(self.leading_quality),
            0 if self.trailing_quality is None else int(self.trailing_quality),
            0 if self.window is None else int(self.window[0]), 0 if self.window is None else int(self.window[1]),
            int(self.min_overlap) if self.adapter is not None else 0,
            int(round(1000 * self.max_error_rate)) if self.adapter is not None else 0,
            int(self.min_length), len(ad), (C.c_uint8 * 64)(*ad))
        if lib.ppg_read_trim_check(C.byref(t)) != 0:
            raise ValueError(f"ReadTrim: not a valid trim: {self!r}")
        return t

    def __repr__(self):
        return (f"ReadTrim(head={self.head}, tail={self.tail}, leading_quality={self.leading_quality}, "
                f"trailing_quality={self.trailing_quality}, window={self.window}, adapter={self.adapter!r}, "
                f"min_overlap={self.min_overlap}, max_error_rate={self.max_error_rate}, min_length={self.min_length}, "
                f"quality_base={self.quality_base})")


def _trim_struct(trim, and_mask=False):
    """The ppg_read_trim of a ReadTrim, or a _lib.PpgReadTrim as it is (its AND_MASK bit set on demand)."""
    if isinstance(trim, ReadTrim):
        return trim.struct(and_mask)
    if not isinstance(trim, _lib.PpgReadTrim):
        raise ValueError("expected a ReadTrim")
    t = _lib.PpgReadTrim.from_buffer_copy(trim)
    if and_mask:
        t.ops |= _lib.PPG_TRIM_AND_MASK
    return t


class ReadTrimResult:
    """The result of a read trim (include/ppgpu.h "read trimming"): `records`, `kept`, `trimmed` (records
    whose window is not the whole read), `cut` (records each cut moved on its own, by 'fixed', 'leading',
    'trailing', 'window', 'adapter'), `bases`, `bases_window`, `bases_kept`, `chunk_kept` (numpy int64,
    keeps per chunk) and, when asked for, `windows` (an int32 CUDA tensor [records, 2] of (start, len)
    rows) and `keep_mask` (a uint32 CUDA tensor in the hit-mask format)."""

    CUTS = ("fixed", "leading", "trailing", "window", "adapter")

    def __init__(self, result, chunk_kept=None, keep_mask=None, windows=None):
        self.records, self.kept, self.trimmed = int(result.records), int(result.kept), int(result.trimmed)
        self.cut = {c: int(v) for c, v in zip(self.CUTS, result.cut)}
        self.bases, self.bases_window, self.bases_kept = int(result.bases), int(result.bases_window), int(result.bases_kept)
        self.chunk_kept = chunk_kept
        self.keep_mask = keep_mask
        self.windows = windows

    def keep_records(self):
        """The shard record numbers of the set mask bits, ascending: an int64 tensor on the mask's device."""
        if self.keep_mask is None:
            raise ValueError("ReadTrimResult.keep_records: the trim was run without a mask")
        import torch
        w = self.keep_mask.view(torch.int32)[:(self.records + 31) // 32]
        bit = torch.arange(32, dtype=torch.int32, device=w.device)
        return ((w[:, None] >> bit) & 1).reshape(-1).nonzero().reshape(-1)

    def windows_host(self):
        """The (start, len) rows of the records as a numpy uint32[records, 2] array."""
        if self.windows is None:
            raise ValueError("ReadTrimResult.windows_host: the trim was run without windows")
        return self.windows.reshape(-1, 2)[:self.records].cpu().numpy().view(np.uint32).reshape(-1, 2)

    def __repr__(self):
        return (f"ReadTrimResult(records={self.records}, kept={self.kept}, trimmed={self.trimmed}, cut={self.cut}, "
                f"bases={self.bases}, bases_window={self.bases_window}, bases_kept={self.bases_kept})")


class ReadProfile:
    """A read profile (include/ppgpu.h "read profile"): bases and qualities of the first max_positions read
    positions (1 .. 1024), read lengths, GC content and mean quality per read.  quality_base is the Quality
    byte of quality 0; the quality histograms have 64 bins above it."""

    def __init__(self, max_positions=256, qual_base=33):
        self.max_positions, self.qual_base = max_positions, qual_base

    def struct(self, use_mask=False, use_windows=False):
        """The ppg_read_profile of this profile (with the USE_MASK / USE_WINDOWS bits); ValueError when
        ppg_read_profile_check refuses it."""
        flags = (_lib.PPG_PROFILE_USE_MASK if use_mask else 0) | (_lib.PPG_PROFILE_USE_WINDOWS if use_windows else 0)
        p = _lib.PpgReadProfile(flags, int(self.qual_base), int(self.max_positions), 0)
        if lib.ppg_read_profile_check(C.byref(p)) != 0:
            raise ValueError(f"ReadProfile: not a valid profile: {self!r}")
        return p

    def __repr__(self):
        return f"ReadProfile(max_positions={self.max_positions}, qual_base={self.qual_base})"


def _profile_struct(profile, use_mask=False, use_windows=False):
    """The ppg_read_profile of a ReadProfile, or of a _lib.PpgReadProfile with its flags set for the buffers."""
    if isinstance(profile, ReadProfile):
        return profile.struct(use_mask, use_windows)
    if not isinstance(profile, _lib.PpgReadProfile):
        raise ValueError("expected a ReadProfile")
    return ReadProfile(profile.max_pos, profile.qual_base).struct(use_mask, use_windows)


class ReadProfileResult:
    """The result of a read profile (include/ppgpu.h "read profile"): the totals `records`, `profiled`,
    `longer` (windows of at least max_positions bases, which length_hist does not count), `bases`,
    `bases_profiled`, `qual_bytes`, `no_quality`; `gc_hist` (numpy int64[101]: reads by GC percent),
    `meanq_hist` (int64[64]: reads by mean quality), `chunk_profiled` (int64, profiled records per chunk)
    and `table`, a numpy structured array of one row per position (base[5], qual_n, qual_sum, len_here,
    qhist[64]).  base_counts, mean_quality and length_hist are views / derivations of the table."""

    CLASSES = ("A", "C", "G", "T", "other")
    ROW_DTYPE = np.dtype([("base", "<i8", (5,)), ("qual_n", "<i8"), ("qual_sum", "<i8"), ("len_here", "<i8"),
                          ("qhist", "<i8", (64,))])

    def __init__(self, result, table, chunk_profiled=None, qual_base=33):
        for name in ("records", "profiled", "longer", "bases", "bases_profiled", "qual_bytes", "no_quality"):
            setattr(self, name, int(getattr(result, name)))
        self.gc_hist = np.array(result.gc_hist, np.int64)
        self.meanq_hist = np.array(result.meanq_hist, np.int64)
        self.table = np.ascontiguousarray(table, np.int64).reshape(-1, 72).view(self.ROW_DTYPE).reshape(-1)
        self.chunk_profiled = chunk_profiled
        self.qual_base = qual_base

    @property
    def base_counts(self):
        """int64[positions, 5]: the bases A, C, G, T and other at every position."""
        return self.table["base"]

    @property
    def length_hist(self):
        """int64[positions]: the profiled reads by the length of their window (`longer` holds the rest)."""
        return self.table["len_here"]

    @property
    def mean_quality(self):
        """float64[positions]: the mean quality above qual_base at every position, nan where no Quality
        byte was counted.  Derived on the host from qual_sum and qual_n."""
        n = self.table["qual_n"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, self.table["qual_sum"] / n - self.qual_base, np.nan)

    def __repr__(self):
        return (f"ReadProfileResult(records={self.records}, profiled={self.profiled}, longer={self.longer}, "
                f"bases={self.bases}, bases_profiled={self.bases_profiled}, qual_bytes={self.qual_bytes}, "
                f"no_quality={self.no_quality}, positions={self.table.shape[0]})")


class ReadDedup:
    """A read dedup (include/ppgpu.h "read dedup"): reads are duplicates of each other when the 64-bit
    fingerprints of their key bytes are equal.  The key is the read, or its trim window, cut to its first
    max_bases bases (0: all of it; 50 is FastQC's rule)."""

    def __init__(self, max_bases=0):
        self.max_bases = max_bases

    def struct(self, and_mask=False, use_windows=False):
        """The ppg_read_dedup of this dedup (with the AND_MASK / USE_WINDOWS bits); ValueError when
        ppg_read_dedup_check refuses it."""
        flags = (_lib.PPG_DEDUP_AND_MASK if and_mask else 0) | (_lib.PPG_DEDUP_USE_WINDOWS if use_windows else 0)
        d = _lib.PpgReadDedup(flags, int(self.max_bases), (C.c_int64 * 2)(0, 0))
        if lib.ppg_read_dedup_check(C.byref(d)) != 0:
            raise ValueError(f"ReadDedup: not a valid dedup: {self!r}")
        return d

    @staticmethod
    def min_slots(records):
        """The smallest legal table for a run of `records` records: a power of two, at least 64 and 2 x records."""
        return max(64, 1 << max(2 * int(records) - 1, 0).bit_length())

    def __repr__(self):
        return f"ReadDedup(max_bases={self.max_bases})"


def _dedup_struct(dedup, and_mask=False, use_windows=False):
    """The ppg_read_dedup of a ReadDedup, or of a _lib.PpgReadDedup with its flags set for the buffers."""
    if isinstance(dedup, ReadDedup):
        return dedup.struct(and_mask, use_windows)
    if not isinstance(dedup, _lib.PpgReadDedup):
        raise ValueError("expected a ReadDedup")
    return ReadDedup(dedup.max_bases).struct(and_mask, use_windows)


class ReadDedupResult:
    """The result of a read dedup (include/ppgpu.h "read dedup"): the totals `records`, `participating`,
    `unique`, `bases`, `bases_unique`, `overflow`, `max_count`, `max_first`; `level_distinct` and `level_reads`
    (numpy int64[16]: the table's rows and their reads by FastQC's duplication level, LEVELS names the bins);
    `chunk_unique` (int64, unique records per chunk); `duplication_rate` = 1 - unique / participating; and the
    device tensors of the call: `unique_mask` (uint32 hit-mask words), `first` (int64 per record: the first
    occurrence's record number, -1 when the record does not participate) and `table` (int64 [slots, 3]: key,
    first, count; an empty row is 0, -1, 0), each None when not asked for."""

    TOTALS = ("records", "participating", "unique", "bases", "bases_unique", "overflow", "max_count", "max_first")
    LEVELS = ("1", "2", "3", "4", "5", "6", "7", "8", "9", ">10", ">50", ">100", ">500", ">1k", ">5k", ">10k")

    def __init__(self, result, chunk_unique=None, unique_mask=None, first=None, table=None):
        for name in self.TOTALS:
            setattr(self, name, int(getattr(result, name)))
        self.level_distinct = np.array(result.level_distinct, np.int64)
        self.level_reads = np.array(result.level_reads, np.int64)
        self.chunk_unique = chunk_unique
        self.unique_mask, self.first, self.table = unique_mask, first, table

    @property
    def duplication_rate(self):
        return 1.0 - self.unique / self.participating if self.participating else 0.0

    def top(self, k):
        """[(count, first)] of the k rows with the greatest counts (fewer when the table holds fewer), found by
        torch.topk on the device table; ties go to the lower first."""
        if self.table is None:
            raise ValueError("ReadDedupResult.top: the dedup was run without a table tensor")
        import torch
        t = self.table.reshape(-1, 3)
        k = min(int(k), t.shape[0])
        if k <= 0:
            return []
        # one score per row: the count first, then the lower record number (first < records)
        m = self.records + 1
        score = torch.where(t[:, 0] != 0, t[:, 2] * m + (m - 1 - t[:, 1]), torch.full_like(t[:, 2], -1))
        rows = t[torch.topk(score, k).indices].cpu().numpy()
        return [(int(c), int(f)) for key, f, c in rows if key != 0]

    def __repr__(self):
        return (f"ReadDedupResult(records={self.records}, participating={self.participating}, unique={self.unique}, "
                f"bases={self.bases}, bases_unique={self.bases_unique}, max_count={self.max_count}, "
                f"max_first={self.max_first}, duplication_rate={self.duplication_rate:.4f})")


class PairOverlap:
    """A pair overlap (include/ppgpu.h "pair overlap"): read 1 against the reverse complement of read 2, an
    offset accepted with at least min_overlap bases of overlap, at most max_diff mismatches and at most
    max_err_milli / 1000 of the overlap mismatching.  The defaults are fastp's."""

    def __init__(self, min_overlap=30, max_diff=5, max_err_milli=200):
        self.min_overlap, self.max_diff, self.max_err_milli = min_overlap, max_diff, max_err_milli

    def struct(self):
        """The ppg_pair_overlap of this overlap; ValueError when ppg_pair_overlap_check refuses it."""
        o = _lib.PpgPairOverlap(0, int(self.min_overlap), int(self.max_diff), int(self.max_err_milli), (C.c_int64 * 4)())
        if lib.ppg_pair_overlap_check(C.byref(o)) != 0:
            raise ValueError(f"PairOverlap: not a valid overlap: {self!r}")
        return o

    def __repr__(self):
        return f"PairOverlap(min_overlap={self.min_overlap}, max_diff={self.max_diff}, max_err_milli={self.max_err_milli})"


class PairOverlapResult:
    """The result of a pair overlap (include/ppgpu.h "pair overlap"): the totals `pairs`, `unmapped`, `too_long`,
    `analysed`, `found`, `negative`, `adapter`, `overlap_bases`, `mismatches`; `clipped` (bases cut from R1, R2);
    `insert_hist` (numpy int64[2048]: found pairs by insert size) and `median_insert` (the lower median of the
    found pairs' insert sizes, None when none was found); and the device tensors of the call: `rows` (int32
    [pairs, 4]: d, overlap, mismatches, insert size; zeros when not found), `found_mask` (uint32 hit-mask words
    by pair), `windows1` / `windows2` (int32 / uint32 [records, 2] (start, len) rows by record of their set),
    each None when not asked for."""

    TOTALS = ("pairs", "unmapped", "too_long", "analysed", "found", "negative", "adapter", "overlap_bases", "mismatches")

    def __init__(self, result, insert_hist, rows=None, found_mask=None, windows1=None, windows2=None):
        for name in self.TOTALS:
            setattr(self, name, int(getattr(result, name)))
        self.clipped = tuple(int(x) for x in result.clipped)
        self.insert_hist = np.asarray(insert_hist, np.int64)
        self.rows, self.found_mask, self.windows1, self.windows2 = rows, found_mask, windows1, windows2

    @property
    def median_insert(self):
        n = int(self.insert_hist.sum())
        if n == 0:
            return None
        return int(np.searchsorted(np.cumsum(self.insert_hist), (n + 1) // 2))

    def __repr__(self):
        return (f"PairOverlapResult(pairs={self.pairs}, analysed={self.analysed}, found={self.found}, "
                f"adapter={self.adapter}, clipped={self.clipped}, median_insert={self.median_insert})")


def _int_tensor_arg(t, dtypes, what, name):
    if not (hasattr(t, "data_ptr") and t.is_cuda and t.dtype in dtypes and t.is_contiguous()):
        raise ValueError(f"{what}: {name} must be a contiguous CUDA tensor of {' / '.join(str(d) for d in dtypes)}")
    return t


def pair_overlap(packed1, packed2, overlap, rec1=None, rec2=None, windows1=None, windows2=None, rows=True,
                 found_mask=True, device=None):
    """The pair overlap `overlap` (a PairOverlap) of two packed read sets on one GPU (ppg_pairs_overlap), as a
    PairOverlapResult.  packed1 / packed2: PackedReads of CUDA tensors (qualities not needed).  rec1 / rec2: int64
    CUDA tensors, pair i = record rec1[i] of set 1 and rec2[i] of set 2 (None: record i; an entry outside the set
    leaves the pair out).  windows1 / windows2: int32 / uint32 CUDA tensors of (start, len) rows by record of that
    set (a trim's), clipped in place to the insert size for found pairs; True starts from whole reads, None: no
    windows.  rows / found_mask: True allocates, a tensor is written, False / None leaves the output out.
    Ordered after torch's stream, complete on return."""
    import torch
    what = "pair_overlap"
    for p in (packed1, packed2):
        if not isinstance(p, PackedReads) or not p.on_device:
            raise ValueError(f"{what}: expected two PackedReads of CUDA tensors")
        p._check_device(what)
    tdev = packed1.seq_off.device
    if packed2.seq_off.device != tdev:
        raise ValueError(f"{what}: both read sets must be on one device")
    dev = device or Device.default(tdev.index if tdev.index is not None else torch.cuda.current_device())
    o = overlap.struct() if isinstance(overlap, PairOverlap) else PairOverlap().struct() if overlap is None else overlap
    if not isinstance(o, _lib.PpgPairOverlap):
        raise ValueError(f"{what}: expected a PairOverlap")
    sets = (packed1, packed2)
    maps = [None if r is None else _int_tensor_arg(r, (torch.int64,), what, "rec1 / rec2") for r in (rec1, rec2)]
    if maps[0] is not None and maps[1] is not None and maps[0].numel() != maps[1].numel():
        raise ValueError(f"{what}: rec1 and rec2 differ in length")
    given = [m.numel() for m in maps if m is not None]
    npairs = given[0] if given else min(packed1.records, packed2.records)
    if rows is True:
        rows = torch.zeros((npairs, 4), dtype=torch.int32, device=tdev)
    elif rows is False:
        rows = None
    if rows is not None:
        _int_tensor_arg(rows, (torch.int32,), what, "rows")
    if found_mask is True:
        found_mask = torch.zeros((npairs + 31) // 32, dtype=torch.int32, device=tdev)
    elif found_mask is False:
        found_mask = None
    if found_mask is not None:
        _int_tensor_arg(found_mask, (torch.int32, torch.uint32), what, "found_mask")
    wins = []
    for p, w in zip(sets, (windows1, windows2)):
        if w is True:
            w = torch.stack([torch.zeros_like(p.seq_len[:p.records]), p.seq_len[:p.records]], dim=1).contiguous()
        if w is not None:
            _int_tensor_arg(w, (torch.int32, torch.uint32), what, "windows")
        wins.append(w)
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                p.qual.data_ptr() if p.qual is not None else None, p.records) for p in sets]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None   # noqa: E731
    res, hist = _lib.PpgPairOverlapResult(), np.zeros(_lib.PPG_OVERLAP_HIST, np.int64)
    dev.after_torch()
    check(lib.ppg_pairs_overlap(dev.handle, C.byref(o), C.byref(views[0]), C.byref(views[1]), ptr(maps[0]), ptr(maps[1]),
                                npairs, ptr(rows), rows.numel() // 4 if rows is not None else 0, ptr(found_mask),
                                32 * found_mask.numel() if found_mask is not None else 0,
                                ptr(wins[0]), wins[0].numel() // 2 if wins[0] is not None else 0,
                                ptr(wins[1]), wins[1].numel() // 2 if wins[1] is not None else 0,
                                C.byref(res), _ptr(hist), hist.size), what)
    return PairOverlapResult(res, hist, rows, None if found_mask is None else found_mask.view(torch.uint32), wins[0], wins[1])


class PairMerge:
    """A pair merge (include/ppgpu.h "pair merge"): one consensus read per overlapping pair.  qual_hi / qual_lo are
    quality bytes as they stand in the file; a disagreement counts as corrected when the base taken has at least
    qual_hi and the one overruled at most qual_lo.  The defaults are '?' and '/': phred 30 and 14 at offset 33."""

    def __init__(self, qual_hi=63, qual_lo=47):
        self.qual_hi, self.qual_lo = qual_hi, qual_lo

    def struct(self):
        """The ppg_pair_merge of this merge; ValueError when ppg_pair_merge_check refuses it."""
        m = _lib.PpgPairMerge(0, int(self.qual_hi), int(self.qual_lo), (C.c_int64 * 5)())
        if lib.ppg_pair_merge_check(C.byref(m)) != 0:
            raise ValueError(f"PairMerge: not a valid merge: {self!r}")
        return m

    def __repr__(self):
        return f"PairMerge(qual_hi={self.qual_hi}, qual_lo={self.qual_lo})"


class PairMergeResult:
    """The result of a pair merge (include/ppgpu.h "pair merge"): the totals `pairs`, `unmapped`, `too_long`,
    `unmerged`, `stale`, `merged`, `merged_bases`, `padded_bases`, `overlap_bases`, `disagree`, `from2`, `ties`,
    `n_filled`, `n_both` and `agree` (the overlap's other positions); `corrected` (read 1 overruled, read 2
    overruled); `reads`, the merged set as a PackedReads of CUDA tensors whose `records` and `total_bases` are the
    merged ones, so that to_host() cuts exactly; `pair_of` (int64 CUDA tensor: the pair of each merged record, or
    None); `overlap`, the PairOverlapResult when PairedFASTQ.Merge ran the overlap."""

    TOTALS = ("pairs", "unmapped", "too_long", "unmerged", "stale", "merged", "merged_bases", "padded_bases",
              "overlap_bases", "disagree", "from2", "ties", "n_filled", "n_both")

    def __init__(self, result, reads, pair_of=None, overlap=None):
        for name in self.TOTALS:
            setattr(self, name, int(getattr(result, name)))
        self.corrected = tuple(int(x) for x in result.corrected)
        self.reads, self.pair_of, self.overlap = reads, pair_of, overlap

    @property
    def agree(self):
        return self.overlap_bases - self.disagree - self.n_filled - self.n_both

    def __repr__(self):
        return (f"PairMergeResult(pairs={self.pairs}, merged={self.merged}, merged_bases={self.merged_bases}, "
                f"disagree={self.disagree}, corrected={self.corrected})")


def pair_merge(packed1, packed2, rows, merge=None, rec1=None, rec2=None, out=None, quality=True, pair_of=True, device=None):
    """The pair merge of two packed read sets with qualities on one GPU (ppg_pairs_merge), as a PairMergeResult.
    rows: the int32 CUDA tensor [pairs, 4] a pair_overlap of the same sets and maps wrote (a zeroed row leaves its
    pair out).  merge: a PairMerge (None: the defaults).  rec1 / rec2: as in pair_overlap.  out: a PackedReads of
    CUDA tensors to write (None: sized with ppg_pairs_merge_size and allocated, with a quality plane iff
    `quality`).  pair_of: True allocates, an int64 CUDA tensor is written, False / None leaves it out.  Ordered
    after torch's stream, complete on return."""
    import torch
    what = "pair_merge"
    for p in (packed1, packed2):
        if not isinstance(p, PackedReads) or not p.on_device:
            raise ValueError(f"{what}: expected two PackedReads of CUDA tensors")
        p._check_device(what)
        if p.qual is None:
            raise ValueError(f"{what}: both read sets need their quality plane")
    tdev = packed1.seq_off.device
    if packed2.seq_off.device != tdev:
        raise ValueError(f"{what}: both read sets must be on one device")
    dev = device or Device.default(tdev.index if tdev.index is not None else torch.cuda.current_device())
    m = merge.struct() if isinstance(merge, PairMerge) else PairMerge().struct() if merge is None else merge
    if not isinstance(m, _lib.PpgPairMerge):
        raise ValueError(f"{what}: expected a PairMerge")
    maps = [None if r is None else _int_tensor_arg(r, (torch.int64,), what, "rec1 / rec2") for r in (rec1, rec2)]
    if maps[0] is not None and maps[1] is not None and maps[0].numel() != maps[1].numel():
        raise ValueError(f"{what}: rec1 and rec2 differ in length")
    given = [r.numel() for r in maps if r is not None]
    npairs = given[0] if given else min(packed1.records, packed2.records)
    _int_tensor_arg(rows, (torch.int32,), what, "rows")
    if rows.numel() % 4:
        raise ValueError(f"{what}: rows must hold four int32 per pair")
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                p.qual.data_ptr(), p.records) for p in (packed1, packed2)]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None   # noqa: E731
    inputs = (C.byref(views[0]), C.byref(views[1]), ptr(maps[0]), ptr(maps[1]), npairs, ptr(rows), rows.numel() // 4)
    dev.after_torch()
    if out is None:
        nrec, nbases = C.c_int64(), C.c_int64()
        check(lib.ppg_pairs_merge_size(dev.handle, *inputs, C.byref(nrec), C.byref(nbases)), what)
        out = PackedReads.empty(nrec.value, nbases.value, quality, tdev)
        dev.after_torch()   # (the planes' zeroing)
    elif not isinstance(out, PackedReads) or not out.on_device:
        raise ValueError(f"{what}: out must be a PackedReads of CUDA tensors")
    else:
        out._check_device(what)
    if pair_of is True:
        pair_of = torch.zeros(out.rec_cap, dtype=torch.int64, device=tdev)
        dev.after_torch()
    elif pair_of is False:
        pair_of = None
    if pair_of is not None:
        _int_tensor_arg(pair_of, (torch.int64,), what, "pair_of")
        if pair_of.numel() < out.rec_cap:
            raise ValueError(f"{what}: pair_of is shorter than out's records")
    res = _lib.PpgPairMergeResult()
    check(lib.ppg_pairs_merge(dev.handle, C.byref(m), *inputs, *out._ptrs(),
                              C.c_void_p(pair_of.data_ptr()) if pair_of is not None else None, C.byref(res)), what)
    out.records, out.total_bases = int(res.merged), int(res.padded_bases)
    return PairMergeResult(res, out, None if pair_of is None else pair_of[:int(res.merged)])


class KmerCount:
    """A k-mer count (include/ppgpu.h "k-mer counts"): every k-mer of k bases, 1 <= k <= 31, as the key whose first
    base is most significant (A 0, C 1, G 2, T 3); canonical: a k-mer and its reverse complement count as one, under
    the smaller of their keys."""

    _BASES = "ACGT"

    def __init__(self, k=21, canonical=True):
        self.k, self.canonical = k, bool(canonical)

    def struct(self, use_windows=False, use_mask=False, accumulate=False):
        """The ppg_kmer_count of this count (with the USE_WINDOWS / USE_MASK / ACCUMULATE bits); ValueError when
        ppg_kmer_count_check refuses it."""
        flags = (_lib.PPG_KMER_CANONICAL if self.canonical else 0) | (_lib.PPG_KMER_USE_WINDOWS if use_windows else 0) | \
            (_lib.PPG_KMER_USE_MASK if use_mask else 0) | (_lib.PPG_KMER_ACCUMULATE if accumulate else 0)
        c = _lib.PpgKmerCount(flags, int(self.k), (C.c_int64 * 6)())
        if lib.ppg_kmer_count_check(C.byref(c)) != 0:
            raise ValueError(f"KmerCount: not a valid k-mer count: {self!r}")
        return c

    @staticmethod
    def min_slots(distinct):
        """The smallest legal table for `distinct` distinct keys: a power of two, at least 64 and 2 x distinct."""
        return max(64, 1 << max(2 * int(distinct) - 1, 0).bit_length())

    def key(self, word):
        """The key of a k-mer given as str or bytes of k upper-case ACGT (the canonical key when canonical)."""
        w = word.decode("ascii") if isinstance(word, (bytes, bytearray)) else str(word)
        if len(w) != self.k or any(c not in self._BASES for c in w):
            raise ValueError(f"KmerCount.key: expected {self.k} bases of ACGT, got {word!r}")
        key = 0
        for c in w:
            key = key * 4 + self._BASES.index(c)
        return self.canonical_key(key) if self.canonical else key

    def canonical_key(self, key):
        """min(key, the key of the reverse complement)."""
        key, rc = int(key), 0
        for i in range(self.k):
            rc = rc * 4 + (3 - ((key >> (2 * i)) & 3))
        return min(key, rc)

    def word(self, key):
        """The k-mer of a key as str (of the canonical key when canonical)."""
        key = int(key)
        if not 0 <= key < 4 ** self.k:
            raise ValueError(f"KmerCount.word: not a key of {self.k} bases: {key}")
        if self.canonical:
            key = self.canonical_key(key)
        return "".join(self._BASES[(key >> (2 * (self.k - 1 - i))) & 3] for i in range(self.k))

    def __repr__(self):
        return f"KmerCount(k={self.k}, canonical={self.canonical})"


class KmerCountResult:
    """The result of a k-mer count (include/ppgpu.h "k-mer counts"): the totals of the call `records`,
    `participating`, `short_reads`, `bases`, `positions`, `kmers`, `invalid`; those of the table after it `distinct`,
    `singletons`, `max_count`, `max_key`, `total_count`; `overflow`; `spectrum` (numpy int64[1024]: rows by count,
    the last bin >= 1023); `table` (the int64 CUDA tensor [slots, 2] of {key, count} rows, an empty row is -1, 0);
    `kmers_spec` (the KmerCount) and `retries` (how often a table sized by doubling was too small)."""

    TOTALS = ("records", "participating", "short_reads", "bases", "positions", "kmers", "invalid", "distinct",
              "singletons", "max_count", "max_key", "total_count", "overflow")

    def __init__(self, result, spectrum, table, kmers_spec, device, retries=0):
        for name in self.TOTALS:
            setattr(self, name, int(getattr(result, name)))
        self.spectrum = np.asarray(spectrum, np.int64)
        self.table, self.kmers_spec, self.device, self.retries = table, kmers_spec, device, int(retries)

    @property
    def slots(self):
        return self.table.numel() // 2

    def select(self, min_count):
        """numpy uint64 [n, 2]: the {key, count} rows with count >= min_count, in no order (two ppg_kmers_select:
        one to count, one to fill)."""
        found = C.c_int64()
        self.device.after_torch()
        check(lib.ppg_kmers_select(self.device.handle, C.c_void_p(self.table.data_ptr()), self.slots, int(min_count), None, 0,
                                   C.byref(found)), "kmers_select")
        return self._select(int(min_count), found.value)

    def _select(self, min_count, cap):
        import torch
        out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=self.table.device)
        found = C.c_int64()
        self.device.after_torch()
        check(lib.ppg_kmers_select(self.device.handle, C.c_void_p(self.table.data_ptr()), self.slots, min_count,
                                   C.c_void_p(out.data_ptr()), cap, C.byref(found)), "kmers_select")
        return out[:found.value].cpu().numpy().view(np.uint64)

    def top(self, n):
        """[(word, count)] of the n most frequent k-mers (fewer when the table holds fewer), ties by the lower key:
        the threshold comes from the spectrum, one ppg_kmers_select takes the rows at or above it, the host sorts."""
        n = min(int(n), self.distinct)
        if n <= 0:
            return []
        above = np.cumsum(self.spectrum[::-1])[::-1]          # above[c]: the rows with count >= c
        t = max(int(np.nonzero(above >= n)[0][-1]), 1)        # the greatest threshold that still gives n rows
        rows = self._select(t, int(above[t]))
        order = np.lexsort((rows[:, 0], -rows[:, 1].astype(np.int64)))[:n]
        return [(self.kmers_spec.word(int(k)), int(c)) for k, c in rows[order]]

    def lookup(self, words_or_keys):
        """numpy int64: the count of each k-mer (str / bytes, canonicalised when the count is canonical) or key
        (int, looked up as given); 0 for one the table does not hold (ppg_kmers_lookup)."""
        import torch
        keys = np.array([k if isinstance(k, (int, np.integer)) else self.kmers_spec.key(k) for k in words_or_keys], np.uint64)
        if keys.size == 0:
            return np.zeros(0, np.int64)
        dk = torch.from_numpy(keys.view(np.int64)).to(self.table.device)
        counts = torch.zeros(keys.size, dtype=torch.int64, device=self.table.device)
        self.device.after_torch()
        check(lib.ppg_kmers_lookup(self.device.handle, C.c_void_p(self.table.data_ptr()), self.slots,
                                   C.c_void_p(dk.data_ptr()), keys.size, C.c_void_p(counts.data_ptr())), "kmers_lookup")
        return counts.cpu().numpy()

    def __repr__(self):
        return (f"KmerCountResult(records={self.records}, kmers={self.kmers}, invalid={self.invalid}, "
                f"distinct={self.distinct}, singletons={self.singletons}, max_count={self.max_count}, slots={self.slots})")


def _kmer_slot_range(k, positions):
    """(first, last) table sizes of a count sized by doubling: the powers of two >= max(64, 2 d / 16) and >= 2 d with
    d = min(4^k, positions), the most distinct keys there can be; the last cannot fail."""
    d = min(4 ** int(k), max(int(positions), 0))
    return KmerCount.min_slots((d + 15) // 16), KmerCount.min_slots(d)


def count_kmers_sets(sets, kmers, masks=None, windows=None, table=None, slots=None, accumulate=False, device=None):
    """count_kmers over several packed read sets into one table: the first as count_kmers would, every further one
    with ACCUMULATE; masks / windows: one entry (or None) per set.  The KmerCountResult is the last call's: its
    totals "of the call" are the last set's, those "of the table" are all sets'.  Sized by doubling when neither
    table nor slots is given: a table that turns out too small starts all sets again in one twice as large."""
    import torch
    what = "count_kmers"
    sets = list(sets)
    if not sets:
        raise ValueError(f"{what}: no read set")
    for p in sets:
        if not isinstance(p, PackedReads) or not p.on_device:
            raise ValueError(f"{what}: expected PackedReads of CUDA tensors")
        p._check_device(what)
    tdev = sets[0].seq_off.device
    if any(p.seq_off.device != tdev for p in sets):
        raise ValueError(f"{what}: the read sets must be on one device")
    dev = device or Device.default(tdev.index if tdev.index is not None else torch.cuda.current_device())
    kmers = KmerCount() if kmers is None else kmers
    if not isinstance(kmers, KmerCount):
        raise ValueError(f"{what}: expected a KmerCount")
    masks = list(masks) if masks is not None else [None] * len(sets)
    windows = list(windows) if windows is not None else [None] * len(sets)
    if len(masks) != len(sets) or len(windows) != len(sets):
        raise ValueError(f"{what}: one mask and one windows entry per read set")
    margs = []
    for p, m, w in zip(sets, masks, windows):
        mp, mcap, _ = _mask_arg(m, what)
        if m is not None and mp is None and p.records:
            raise ValueError(f"{what}: the mask is empty")
        if w is not None:
            _int_tensor_arg(w, (torch.int32, torch.uint32), what, "windows")
            if w.numel() % 2:
                raise ValueError(f"{what}: windows must hold two values per record")
        margs.append((mp, mcap, C.c_void_p(w.data_ptr()) if w is not None else None, w.numel() // 2 if w is not None else 0))
    if accumulate and table is None:
        raise ValueError(f"{what}: accumulate needs the table of the earlier count")
    if table is not None:
        _int_tensor_arg(table, (torch.int64,), what, "table")
        if table.device != tdev or table.numel() % 2:
            raise ValueError(f"{what}: table must hold two int64 per row on the read sets' device")
        first = last = table.numel() // 2
    elif slots is not None:
        first = last = int(slots)
    else:
        first, last = _kmer_slot_range(kmers.k, sum(p.total_bases if p.total_bases is not None else p.base_cap for p in sets))
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                p.qual.data_ptr() if p.qual is not None else None, p.records) for p in sets]
    structs = [kmers.struct(use_windows=a[2] is not None, use_mask=a[0] is not None, accumulate=accumulate or i > 0)
               for i, a in enumerate(margs)]
    n, retries = first, 0
    while True:
        t = table if table is not None else torch.empty((n, 2), dtype=torch.int64, device=tdev)
        res, spectrum = _lib.PpgKmerCountResult(), np.zeros(_lib.PPG_KMER_SPECTRUM, np.int64)
        dev.after_torch()
        rc = 0
        for v, c, (mp, mcap, wp, wcap) in zip(views, structs, margs):
            rc = lib.ppg_kmers_count(dev.handle, C.byref(c), C.byref(v), mp, mcap, wp, wcap, C.c_void_p(t.data_ptr()), n,
                                     C.byref(res), _ptr(spectrum), spectrum.size)
            if rc != 0:
                break
        if rc == _lib.PPG_BUF_ERROR and n < last:
            del t
            n, retries = 2 * n, retries + 1
            continue
        check(rc, what)
        return KmerCountResult(res, spectrum, t, kmers, dev, retries)


def count_kmers(packed, kmers=None, mask=None, windows=None, table=None, slots=None, accumulate=False, device=None):
    """The k-mer count `kmers` (a KmerCount, None: k = 21 canonical) of a packed read set on one GPU
    (ppg_kmers_count), as a KmerCountResult.  packed: a PackedReads of CUDA tensors (qualities not needed).  mask: a
    SeqQuery with a mask or int32 / uint32 CUDA tensor of hit-mask words by record: only records with their bit set
    count (None: all).  windows: an int32 / uint32 CUDA tensor of (start, len) rows by record (a trim's): k-mers are
    taken inside them (None: whole reads).  table: an int64 CUDA tensor [slots, 2] to count into, slots a power of
    two >= 64; or slots: the size of a new one; or neither: sized by doubling, from a sixteenth of the largest table
    the input can need, again after every PPG_BUF_ERROR (the result's `retries`).  accumulate: add to what an
    earlier count with the same KmerCount left in `table`.  Ordered after torch's stream, complete on return."""
    return count_kmers_sets([packed], kmers, [mask], [windows], table, slots, accumulate, device)


class SelectedRecords:
    """The records a mask selects (include/ppgpu.h "record selection"): `bytes` (uint8, the selected
    records' text back to back), `sel_off` (int64, records + 1 offsets into it), `desc` (records x 4:
    the newline positions relative to the record's own first byte) and `recno` (int64, the records'
    numbers), with `records` and `nbytes` the counts in use.  The arrays are either CUDA tensors on
    one device (uint8, int64, int32 views of the uint32 descriptors) or numpy arrays (uint8, int64,
    uint32); record(i) and iteration read host arrays.  A trimming cursor's selection also has `trim`,
    a numpy uint32[records, 2] array of the records' (start, len) windows (else None), and trimmed(i)."""

    def __init__(self, bytes, sel_off, desc, recno, records=None, nbytes=None, trim=None):   # noqa: A002
        self.bytes, self.sel_off, self.desc, self.recno = bytes, sel_off, desc, recno
        self.trim = trim
        self.records = int(records) if records is not None else int(recno.shape[0])
        self.nbytes = int(nbytes) if nbytes is not None else int(bytes.shape[0])

    @classmethod
    def empty(cls, sel_cap, byte_cap, device=None):
        """Buffers for sel_cap records of byte_cap bytes in all: CUDA tensors on `device` (an int or
        torch.device), numpy arrays when device is None; no record in use."""
        sel_cap, byte_cap = int(sel_cap), int(byte_cap)
        if device is None:
            return cls(np.zeros(byte_cap, np.uint8), np.zeros(sel_cap + 1, np.int64), np.zeros((sel_cap, 4), np.uint32),
                       np.zeros(sel_cap, np.int64), 0, 0)
        import torch
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        # (an empty tensor has no address: a buffer of capacity 0 keeps one element behind it)
        back = [torch.zeros(max(int(n), 1), dtype=dt, device=dev)
                for n, dt in ((byte_cap, torch.uint8), (sel_cap + 1, torch.int64), (4 * sel_cap, torch.int32), (sel_cap, torch.int64))]
        out = cls(back[0][:byte_cap], back[1], back[2][:4 * sel_cap].view(-1, 4), back[3][:sel_cap], 0, 0)
        out._back = back
        return out

    @property
    def on_device(self):
        return hasattr(self.bytes, "data_ptr")

    @property
    def sel_cap(self):
        return int(self.recno.shape[0])

    @property
    def byte_cap(self):
        return int(self.bytes.shape[0])

    def _check_device(self, what):
        import torch
        for t, dt in ((self.bytes, torch.uint8), (self.sel_off, torch.int64), (self.desc, torch.int32),
                      (self.recno, torch.int64)):
            if not (hasattr(t, "data_ptr") and t.is_cuda and t.dtype == dt and t.is_contiguous()):
                raise ValueError(f"{what}: the buffers must be contiguous CUDA tensors (uint8, int64, int32 words)")
        if self.sel_off.numel() != self.sel_cap + 1 or self.desc.numel() != 4 * self.sel_cap:
            raise ValueError(f"{what}: buffer sizes do not agree (SelectedRecords.empty makes them)")

    def _ptrs(self):
        b, off, desc, recno = getattr(self, "_back", None) or (self.bytes, self.sel_off, self.desc, self.recno)
        return (C.c_void_p(recno.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(desc.data_ptr()),
                self.sel_cap, C.c_void_p(b.data_ptr()), self.byte_cap)

    def to_host(self):
        """The same selection as numpy arrays (a copy; uint32 descriptors), cut to its records and bytes."""
        nr, nb = self.records, self.nbytes
        if not self.on_device:
            return SelectedRecords(np.array(self.bytes[:nb]), np.array(self.sel_off[:nr + 1]),
                                   np.array(self.desc).reshape(-1, 4)[:nr].copy(), np.array(self.recno[:nr]), nr, nb)
        desc = self.desc.reshape(-1, 4)[:nr].cpu().numpy().view(np.uint32).reshape(-1, 4)
        return SelectedRecords(self.bytes[:nb].cpu().numpy(), self.sel_off[:nr + 1].cpu().numpy(), desc,
                               self.recno[:nr].cpu().numpy(), nr, nb)

    def record(self, i):
        """Selected record i as a FastqRecord over this selection's bytes (host arrays)."""
        if self.on_device:
            raise ValueError("SelectedRecords: record() reads host arrays (to_host() first)")
        if not 0 <= i < self.records:
            raise IndexError(i)
        a, e = int(self.sel_off[i]), int(self.sel_off[i + 1])
        n1, n2, n3, n4 = (int(v) for v in self.desc[i])
        return FastqRecord(self.bytes[a:e], 0, n1, n2, n3, n4)

    def trimmed(self, i):
        """(sequence, quality) of selected record i cut to its window: views of this selection's bytes,
        S[start, start + len) and Q[start, min(start + len, Lq)) (include/ppgpu.h "read trimming")."""
        if self.trim is None:
            raise ValueError("SelectedRecords: trimmed() needs a selection made with a trim")
        r = self.record(i)
        a, n = int(self.trim[i][0]), int(self.trim[i][1])
        return r.raw[r.n1 + 1 + a:r.n1 + 1 + a + n], r.raw[r.n3 + 1 + a:min(r.n3 + 1 + a + n, r.n4)]

    def __len__(self):
        return self.records

    def __iter__(self):
        for i in range(self.records):
            yield self.record(i)

    def __repr__(self):
        return f"SelectedRecords(records={self.records}, nbytes={self.nbytes})"


def _mask_arg(mask, what):
    """(pointer argument, mask_cap, the tensor to keep alive) of a record mask: None (every record), a
    SeqQuery made with a mask, or a contiguous int32 / uint32 CUDA tensor of hit-mask words."""
    if mask is None:
        return None, 0, None
    if isinstance(mask, SeqQuery):
        if mask.hit_mask is None:
            raise ValueError(f"{what}: the SeqQuery was made without a mask")
        mask = mask.hit_mask
    import torch
    if not (hasattr(mask, "data_ptr") and mask.is_cuda and mask.dtype in (torch.int32, torch.uint32) and mask.is_contiguous()):
        raise ValueError(f"{what}: mask must be a SeqQuery with a mask or a contiguous int32 / uint32 CUDA tensor")
    if mask.numel() == 0:
        return None, 0, None
    return C.c_void_p(mask.data_ptr()), 32 * mask.numel(), mask


class Shard:
    """DecompressAll over index chunks [first, first+n) resident on one GPU (ppg_shard)."""

    def __init__(self, index, comp, first=0, n=None, device=None, comp_on_device=False, comp_len=None,
                 out_capacity=0):
        self.index = index
        self.dev = device or Device.default()
        if n is None:
            n = index.Count - 1 - first
        self.first, self.n = first, n
        self._on_device = bool(comp_on_device)
        if comp_on_device:
            ptr, length = int(comp), int(comp_len)
            # the library reads comp on its own stream: order that after torch's producers of comp
            # (a caller on another stream calls self.dev.wait_stream(its stream) itself)
            self._torch_order()
        else:
            self._host = _as_u8(comp)
            ptr, length = self._host.ctypes.data, self._host.size
        h = C.c_void_p()
        check(lib.ppg_shard_create(self.dev.handle, index.handle, first, n, C.c_void_p(ptr), length,
                                   1 if comp_on_device else 0, int(out_capacity), C.byref(h)), "ppg_shard_create")
        self._h = h
        self.dev._retain()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:   # (lib is None at interpreter exit)
            lib.ppg_shard_free(h)
            self._h = None
            self.dev._release()

    @property
    def handle(self):
        return self._h

    def _torch_order(self):
        import sys
        if "torch" in sys.modules and sys.modules["torch"].cuda.is_initialized():
            self.dev.after_torch()

    def run(self):
        hooked = getattr(self, "_seqpack", None) is not None or getattr(self, "_sq_mask", None) is not None or \
            getattr(self, "_select", None) is not None or getattr(self, "_rf", None) is not None or \
            getattr(self, "_rt", None) is not None or getattr(self, "_dd", None) is not None
        if self._on_device or hooked:
            self._torch_order()   # the caller may have rewritten comp (or the hooks' tensors) since the last run
        check(lib.ppg_shard_run(self._h), "DecompressAll")
        return self

    def copy_output(self, off, length, dst=None):
        """Bytes [off, off+length) of the shard's decompressed output (relative to its first
        chunk's Output) into a new uint8 numpy array, or into `dst`: a numpy array (host) or a
        uint8 CUDA tensor on this device (device-to-device, stream-ordered after torch's stream)."""
        if dst is None:
            dst = np.empty(int(length), np.uint8)
        if hasattr(dst, "data_ptr"):
            if not (dst.is_cuda and dst.numel() >= length):
                raise ValueError("copy_output: dst tensor must be a CUDA tensor of >= length bytes")
            self.dev.after_torch()
            check(lib.ppg_shard_copy_output(self._h, int(off), int(length), C.c_void_p(dst.data_ptr()), 1),
                  "copy_output")
        else:
            if dst.nbytes < length:
                raise ValueError("copy_output: dst too small")
            check(lib.ppg_shard_copy_output(self._h, int(off), int(length), _ptr(dst), 0), "copy_output")
        return dst

    @property
    def batches(self):
        return lib.ppg_shard_batches(self._h)

    def set_split(self, bits, outputs, windows):
        """Decode chunks as several waves each, split at side points (deflate block starts inside
        the chunks: absolute bit, absolute output, 32 KiB window each; ppg_shard_set_split).
        Empty arrays restore one wave per chunk.  Results are identical either way."""
        bits = np.ascontiguousarray(bits, np.int64)
        outputs = np.ascontiguousarray(outputs, np.int64)
        windows = np.ascontiguousarray(windows, np.uint8)
        n = int(bits.size)
        if outputs.size != n or windows.size != n * 32768:
            raise ValueError("set_split: bits, outputs and windows (n * 32768 bytes) must agree")
        self._split = (bits, outputs, windows)
        check(lib.ppg_shard_set_split(self._h, n, _ptr(bits) if n else None, _ptr(outputs) if n else None,
                                      _ptr(windows) if n else None), "set_split")
        return self

    def set_keys(self, keys):
        """From the next run on, every output batch writes its records' spot keys (paired reads,
        ppg_record_keys) into `keys`, an int64 CUDA tensor on this device indexed by shard record
        number (ppg_shard_set_keys): works for shards of any number of batches.  None turns it off."""
        if keys is None:
            check(lib.ppg_shard_set_keys(self._h, None, 0), "set_keys")
            self._keys = None
            return self
        import torch
        if not (keys.is_cuda and keys.dtype == torch.int64 and keys.is_contiguous()):
            raise ValueError("set_keys: keys must be a contiguous int64 CUDA tensor")
        self._keys = keys   # kept alive while the library may write it
        check(lib.ppg_shard_set_keys(self._h, C.c_void_p(keys.data_ptr()), keys.numel()), "set_keys")
        return self

    def seq_bases(self):
        """(padded bases, records) of the last run, any number of batches (ppg_shard_seq_bases):
        the capacities a PackedReads of the whole shard needs."""
        tot, rec = C.c_int64(), C.c_int64()
        check(lib.ppg_shard_seq_bases(self._h, C.byref(tot), C.byref(rec)), "seq_bases")
        return tot.value, rec.value

    def pack_sequences(self, quality=True, packed=None):
        """The packed reads of a one-batch shard after its run (ppg_shard_pack_seq), as a
        PackedReads of CUDA tensors on this device: into `packed`, or into a new one sized by
        seq_bases().  Ordered after torch's stream, complete on return."""
        if packed is None:
            tot, rec = self.seq_bases()
            packed = PackedReads.empty(rec, tot, quality, self.dev.device)
        packed._check_device("pack_sequences")
        self.dev.after_torch()
        tot = C.c_int64()
        check(lib.ppg_shard_pack_seq(self._h, *packed._ptrs(), C.byref(tot)), "pack_sequences")
        packed.records, packed.total_bases = self.total_records, tot.value
        return packed

    def set_seqpack(self, packed):
        """From the next run on, every output batch packs its reads into `packed` (a PackedReads of
        CUDA tensors on this device, sized for the whole shard: seq_bases() of an earlier run) while
        its output is resident (ppg_shard_set_seqpack): works for shards of any number of batches.
        None turns it off."""
        if packed is None:
            check(lib.ppg_shard_set_seqpack(self._h, None, None, 0, None, None, None, 0), "set_seqpack")
            self._seqpack = None
            return self
        packed._check_device("set_seqpack")
        self._seqpack = packed   # kept alive while the library may write it
        self.dev.after_torch()
        check(lib.ppg_shard_set_seqpack(self._h, *packed._ptrs()), "set_seqpack")
        return self

    @property
    def seqpack_ready(self):
        """Whether the last run filled the set_seqpack planes (their records / total_bases are then set)."""
        tot = C.c_int64()
        ok = lib.ppg_shard_seqpack_ready(self._h, C.byref(tot)) == 1
        p = getattr(self, "_seqpack", None)
        if ok and p is not None:
            p.records, p.total_bases = self.total_records, tot.value
        return ok

    def query_sequences(self, pattern=None, mask=False):
        """Pattern search and base census over the Sequences of a one-batch shard after its run
        (ppg_shard_query_seq), as a SeqQuery.  pattern: up to 64 bytes without '\\n' (None or empty:
        the census alone, every record a hit); mask=True also returns the per-record hit bits as a
        uint32 CUDA tensor on this device.  Ordered after torch's stream, complete on return."""
        pat, m = _pattern_arg(pattern)
        hm, cap = None, 0
        if mask:
            import torch
            cap = (max(self.total_records, 0) + 31) // 32 * 32
            dev = torch.device("cuda", self.dev.device)
            hm = torch.zeros(cap // 32, dtype=torch.int32, device=dev).view(torch.uint32)
        self._torch_order()
        res, ch = _lib.PpgSeqQueryResult(), np.zeros(self.n, np.int64)
        check(lib.ppg_shard_query_seq(self._h, pat, m, C.c_void_p(hm.data_ptr()) if cap else None, cap, _ptr(ch),
                                      C.byref(res)), "query_sequences")
        return SeqQuery(res, ch, hm)

    def set_seqquery(self, pattern, mask=None):
        """From the next run on, every output batch is searched for `pattern` and its bases counted
        while its output is resident (ppg_shard_set_seqquery): works for shards of any number of
        batches; the result is `seqquery` after the run.  pattern as in query_sequences, b"" for
        the census alone; None turns the hook off.  mask: an int32 / uint32 CUDA tensor on this
        device of at least ceil(records / 32) words that receives the hit bits, or None."""
        if pattern is None:
            check(lib.ppg_shard_set_seqquery(self._h, None, -1, None, 0), "set_seqquery")
            self._sq_mask = None
            return self
        pat, m = _pattern_arg(pattern)
        ptr, cap = None, 0
        if mask is not None:
            import torch
            if not (mask.is_cuda and mask.dtype in (torch.int32, torch.uint32) and mask.is_contiguous()):
                raise ValueError("set_seqquery: mask must be a contiguous int32 / uint32 CUDA tensor")
            ptr, cap = C.c_void_p(mask.data_ptr()), 32 * mask.numel()
            mask = mask.view(torch.uint32)
        self._sq_mask = mask   # kept alive while the library may write it
        self._torch_order()
        check(lib.ppg_shard_set_seqquery(self._h, pat, m, ptr if cap else None, cap), "set_seqquery")
        return self

    @property
    def seqquery(self):
        """The SeqQuery of the last run's set_seqquery hook, or None when that run did not complete one."""
        res, ch = _lib.PpgSeqQueryResult(), np.zeros(self.n, np.int64)
        if lib.ppg_shard_seqquery_ready(self._h, _ptr(ch), C.byref(res)) != 1:
            return None
        return SeqQuery(res, ch, getattr(self, "_sq_mask", None))

    def filter_reads(self, flt, mask=False, metrics=False):
        """The read filter `flt` (a ReadFilter) over the records of a one-batch shard after its run
        (ppg_shard_filter_reads), as a ReadFilterResult.  mask=True also returns the per-record pass bits
        as a uint32 CUDA tensor on this device; a tensor of hit-mask words instead (a query's hit_mask)
        is ANDed in place with them.  metrics=True also returns the per-record metrics rows.  Ordered
        after torch's stream, complete on return."""
        import torch
        dev = torch.device("cuda", self.dev.device)
        nrec = max(self.total_records, 0)
        pm, cap, and_mask = None, 0, False
        if mask is True:
            cap = (nrec + 31) // 32 * 32
            pm = torch.zeros(cap // 32, dtype=torch.int32, device=dev).view(torch.uint32)
        elif mask is not False and mask is not None:
            _, cap, pm = _mask_arg(mask, "filter_reads")
            and_mask = True
        mt = torch.zeros((nrec, 24), dtype=torch.uint8, device=dev) if metrics else None
        f = _filter_struct(flt, and_mask)
        self._torch_order()
        res, ch = _lib.PpgReadFilterResult(), np.zeros(self.n, np.int64)
        check(lib.ppg_shard_filter_reads(self._h, C.byref(f), C.c_void_p(pm.data_ptr()) if cap else None, cap,
                                         C.c_void_p(mt.data_ptr()) if metrics and nrec else None, nrec if metrics else 0,
                                         _ptr(ch), C.byref(res)), "filter_reads")
        return ReadFilterResult(res, ch, pm, mt)

    def set_readfilter(self, flt, mask=None, metrics=None, and_mask=False):
        """From the next run on, every output batch is measured and filtered by `flt` while its output is
        resident (ppg_shard_set_readfilter): works for shards of any number of batches, and runs after a
        set_seqquery hook and before a set_select hook; the result is `readfilter` after the run.
        mask: an int32 / uint32 CUDA tensor of at least ceil(records / 32) words for the pass bits
        (and_mask=True: its bits are ANDed with them instead, e.g. the query hook's mask); metrics: a
        uint8 CUDA tensor of at least 24 * records bytes for the metrics rows.  flt=None turns it off."""
        if flt is None:
            check(lib.ppg_shard_set_readfilter(self._h, None, None, 0, None, 0), "set_readfilter")
            self._rf = None
            return self
        import torch
        ptr, cap = None, 0
        if mask is not None:
            ptr, cap, mask = _mask_arg(mask, "set_readfilter")
            if mask is not None:
                mask = mask.view(torch.uint32)
        mptr, mcap = None, 0
        if metrics is not None:
            if not (metrics.is_cuda and metrics.dtype == torch.uint8 and metrics.is_contiguous()):
                raise ValueError("set_readfilter: metrics must be a contiguous uint8 CUDA tensor")
            mcap = metrics.numel() // 24
            mptr = C.c_void_p(metrics.data_ptr()) if mcap else None
        f = _filter_struct(flt, and_mask)
        self._rf = (mask, metrics)   # kept alive while the library may write them
        self._torch_order()
        check(lib.ppg_shard_set_readfilter(self._h, C.byref(f), ptr, cap, mptr, mcap), "set_readfilter")
        return self

    @property
    def readfilter(self):
        """The ReadFilterResult of the last run's set_readfilter hook, or None when that run did not complete one."""
        res, ch = _lib.PpgReadFilterResult(), np.zeros(self.n, np.int64)
        if lib.ppg_shard_readfilter_ready(self._h, _ptr(ch), C.byref(res)) != 1:
            return None
        rf = getattr(self, "_rf", None) or (None, None)
        return ReadFilterResult(res, ch, rf[0], rf[1])

    def trim_reads(self, trim, mask=False, windows=True):
        """The read trim `trim` (a ReadTrim) over the records of a one-batch shard after its run
        (ppg_shard_trim_reads), as a ReadTrimResult.  windows=True also returns the per-record (start,
        len) rows as an int32 CUDA tensor [records, 2]; mask=True the keep bits as a uint32 CUDA tensor;
        a tensor of hit-mask words instead is ANDed in place with them.  Ordered after torch's stream,
        complete on return."""
        import torch
        dev = torch.device("cuda", self.dev.device)
        nrec = max(self.total_records, 0)
        km, cap, and_mask = None, 0, False
        if mask is True:
            cap = (nrec + 31) // 32 * 32
            km = torch.zeros(cap // 32, dtype=torch.int32, device=dev).view(torch.uint32)
        elif mask is not False and mask is not None:
            _, cap, km = _mask_arg(mask, "trim_reads")
            and_mask = True
        rows = torch.zeros((nrec, 2), dtype=torch.int32, device=dev) if windows else None
        t = _trim_struct(trim, and_mask)
        self._torch_order()
        res, ch = _lib.PpgReadTrimResult(), np.zeros(self.n, np.int64)
        check(lib.ppg_shard_trim_reads(self._h, C.byref(t), C.c_void_p(km.data_ptr()) if cap else None, cap,
                                       C.c_void_p(rows.data_ptr()) if windows and nrec else None, nrec if windows else 0,
                                       _ptr(ch), C.byref(res)), "trim_reads")
        return ReadTrimResult(res, ch, km, rows)

    def set_readtrim(self, trim, mask=None, windows=None, and_mask=False):
        """From the next run on, every output batch is trimmed by `trim` while its output is resident
        (ppg_shard_set_readtrim): works for shards of any number of batches, and runs after the
        set_seqquery and set_readfilter hooks and before a set_select hook; the result is `readtrim`
        after the run.  mask: an int32 / uint32 CUDA tensor of at least ceil(records / 32) words for the
        keep bits (and_mask=True: its bits are ANDed with them instead); windows: an int32 / uint32 CUDA
        tensor of at least 2 * records words for the (start, len) rows.  trim=None turns it off."""
        if trim is None:
            check(lib.ppg_shard_set_readtrim(self._h, None, None, 0, None, 0), "set_readtrim")
            self._rt = None
            return self
        import torch
        ptr, cap = None, 0
        if mask is not None:
            ptr, cap, mask = _mask_arg(mask, "set_readtrim")
            if mask is not None:
                mask = mask.view(torch.uint32)
        wptr, wcap = None, 0
        if windows is not None:
            if not (windows.is_cuda and windows.dtype in (torch.int32, torch.uint32) and windows.is_contiguous()):
                raise ValueError("set_readtrim: windows must be a contiguous int32 / uint32 CUDA tensor")
            wcap = windows.numel() // 2
            wptr = C.c_void_p(windows.data_ptr()) if wcap else None
        t = _trim_struct(trim, and_mask)
        self._rt = (mask, windows)   # kept alive while the library may write them
        self._torch_order()
        check(lib.ppg_shard_set_readtrim(self._h, C.byref(t), ptr, cap, wptr, wcap), "set_readtrim")
        return self

    @property
    def readtrim(self):
        """The ReadTrimResult of the last run's set_readtrim hook, or None when that run did not complete one."""
        res, ch = _lib.PpgReadTrimResult(), np.zeros(self.n, np.int64)
        if lib.ppg_shard_readtrim_ready(self._h, _ptr(ch), C.byref(res)) != 1:
            return None
        rt = getattr(self, "_rt", None) or (None, None)
        return ReadTrimResult(res, ch, rt[0], rt[1])

    def _profile_args(self, profile, mask, windows, what):
        """(struct, mask pointer, mask_cap, rows pointer, rows cap, tensors to keep alive) of a profile call"""
        ptr, cap, mask = _mask_arg(mask, what)
        wptr, wcap = None, 0
        if windows is not None:
            import torch
            if not (hasattr(windows, "data_ptr") and windows.is_cuda and windows.dtype in (torch.int32, torch.uint32)
                    and windows.is_contiguous()):
                raise ValueError(f"{what}: windows must be a contiguous int32 / uint32 CUDA tensor")
            wcap = windows.numel() // 2
            wptr = C.c_void_p(windows.data_ptr()) if wcap else None
        p = _profile_struct(profile, ptr is not None, wptr is not None)
        return p, ptr, cap, wptr, wcap if wptr is not None else 0, (mask, windows)

    def profile_reads(self, profile, mask=None, windows=None):
        """The read profile `profile` (a ReadProfile) over the records of a one-batch shard after its run
        (ppg_shard_profile_reads), as a ReadProfileResult.  mask: hit-mask words (a SeqQuery with a mask
        or an int32 / uint32 CUDA tensor): only the records whose bit is set are profiled; windows: an
        int32 / uint32 CUDA tensor of (start, len) rows (a trim's): each record is profiled inside its
        window.  Both are only read.  Ordered after torch's stream, complete on return."""
        p, ptr, cap, wptr, wcap, _ = self._profile_args(profile, mask, windows, "profile_reads")
        self._torch_order()
        res, ch = _lib.PpgReadProfileResult(), np.zeros(self.n, np.int64)
        table = np.zeros((int(p.max_pos), 72), np.int64)
        check(lib.ppg_shard_profile_reads(self._h, C.byref(p), ptr, cap, wptr, wcap, _ptr(ch), C.byref(res),
                                          _ptr(table), table.shape[0]), "profile_reads")
        return ReadProfileResult(res, table, ch, int(p.qual_base))

    def set_readprofile(self, profile, mask=None, windows=None):
        """From the next run on, every output batch is profiled by `profile` while its output is resident
        (ppg_shard_set_readprofile): works for shards of any number of batches, and runs after the
        set_seqquery, set_readfilter and set_readtrim hooks and before a set_select hook, so it reads the
        mask and the windows those have written; the result is `readprofile` after the run.  mask and
        windows as in profile_reads, sized for the whole shard.  profile=None turns it off."""
        if profile is None:
            check(lib.ppg_shard_set_readprofile(self._h, None, None, 0, None, 0), "set_readprofile")
            self._rp = None
            return self
        p, ptr, cap, wptr, wcap, keep = self._profile_args(profile, mask, windows, "set_readprofile")
        self._rp = (keep, int(p.max_pos), int(p.qual_base))   # kept alive while the library may read them
        self._torch_order()
        check(lib.ppg_shard_set_readprofile(self._h, C.byref(p), ptr, cap, wptr, wcap), "set_readprofile")
        return self

    @property
    def readprofile(self):
        """The ReadProfileResult of the last run's set_readprofile hook, or None when that run did not complete one."""
        rp = getattr(self, "_rp", None)
        if rp is None:
            return None
        res, ch = _lib.PpgReadProfileResult(), np.zeros(self.n, np.int64)
        table = np.zeros((rp[1], 72), np.int64)
        if lib.ppg_shard_readprofile_ready(self._h, _ptr(ch), C.byref(res), _ptr(table), table.shape[0]) != 1:
            return None
        return ReadProfileResult(res, table, ch, rp[2])

    def _dedup_args(self, dedup, mask, windows, first, table, and_mask, what, nrec=None):
        """(struct, the ctypes arguments after it up to slots, (mask, windows, first, table) tensors) of a dedup
        call.  mask / first: True allocates one for nrec records; table: None allocates the smallest legal one."""
        import torch
        dev = torch.device("cuda", self.dev.device)
        if mask is True:
            mask = torch.zeros((nrec + 31) // 32, dtype=torch.int32, device=dev)
        elif mask is False:
            mask = None
        ptr, cap, mask = _mask_arg(mask, what)
        if and_mask and ptr is None:
            raise ValueError(f"{what}: and_mask needs a mask tensor")
        wptr, wcap = None, 0
        if windows is not None:
            if not (hasattr(windows, "data_ptr") and windows.is_cuda and windows.dtype in (torch.int32, torch.uint32)
                    and windows.is_contiguous()):
                raise ValueError(f"{what}: windows must be a contiguous int32 / uint32 CUDA tensor")
            wcap = windows.numel() // 2
            wptr = C.c_void_p(windows.data_ptr()) if wcap else None
        if first is True:
            first = torch.zeros(nrec, dtype=torch.int64, device=dev)
        elif first is False:
            first = None
        fptr, fcap = None, 0
        if first is not None:
            if not (hasattr(first, "data_ptr") and first.is_cuda and first.dtype == torch.int64 and first.is_contiguous()):
                raise ValueError(f"{what}: first must be a contiguous int64 CUDA tensor")
            fcap = first.numel()
            fptr = C.c_void_p(first.data_ptr()) if fcap else None
        if table is None:
            table = torch.zeros((ReadDedup.min_slots(nrec), 3), dtype=torch.int64, device=dev)
        if not (hasattr(table, "data_ptr") and table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
                and table.numel() % 3 == 0):
            raise ValueError(f"{what}: table must be a contiguous int64 CUDA tensor of slots x 3 values")
        d = _dedup_struct(dedup, and_mask, wptr is not None)
        args = (ptr, cap, wptr, wcap if wptr is not None else 0, fptr, fcap if fptr is not None else 0,
                C.c_void_p(table.data_ptr()), table.numel() // 3)
        return d, args, (None if mask is None else mask.view(torch.uint32), windows, first, table)

    def dedup_reads(self, dedup, mask=False, windows=None, first=False, table=None, and_mask=False):
        """The read dedup `dedup` (a ReadDedup) over the records of a one-batch shard after its run
        (ppg_shard_dedup_reads), as a ReadDedupResult.  mask=True also returns the unique bits as a uint32 CUDA
        tensor; a tensor of hit-mask words is written instead, or with and_mask=True decides which records
        participate and is ANDed in place with the unique bits.  windows: an int32 / uint32 CUDA tensor of
        (start, len) rows (a trim's): the key bytes come from inside them.  first=True also returns the first
        occurrence's record number per record.  table: an int64 CUDA tensor [slots, 3], slots a power of two of
        at least 2 x records; None allocates the smallest legal one.  Ordered after torch's stream, complete on
        return."""
        nrec = max(self.total_records, 0)
        d, args, keep = self._dedup_args(dedup, mask, windows, first, table, and_mask, "dedup_reads", nrec)
        self._torch_order()
        res, ch = _lib.PpgReadDedupResult(), np.zeros(self.n, np.int64)
        check(lib.ppg_shard_dedup_reads(self._h, C.byref(d), *args, _ptr(ch), C.byref(res)), "dedup_reads")
        return ReadDedupResult(res, ch, keep[0], keep[2], keep[3])

    def set_readdedup(self, dedup, mask=None, windows=None, first=None, table=None, and_mask=False):
        """From the next run on, every output batch is deduplicated by `dedup` against `table` while its output
        is resident (ppg_shard_set_readdedup): works for shards of any number of batches, and runs after the
        set_seqquery, set_readfilter and set_readtrim hooks and before the set_readprofile and set_select
        hooks, so with and_mask=True on their mask tensor those see first occurrences only; the result is
        `readdedup` after the run.  mask, windows, first and table as in dedup_reads, tensors sized for the
        whole shard (table: required).  dedup=None turns it off."""
        if dedup is None:
            check(lib.ppg_shard_set_readdedup(self._h, None, None, 0, None, 0, None, 0, None, 0), "set_readdedup")
            self._dd = None
            return self
        if table is None:
            raise ValueError("set_readdedup: a table tensor is required (ReadDedup.min_slots(records) x 3 int64)")
        d, args, keep = self._dedup_args(dedup, False if mask is None else mask, windows, False if first is None else first,
                                         table, and_mask, "set_readdedup")
        self._dd = keep   # kept alive while the library may write them
        self._torch_order()
        check(lib.ppg_shard_set_readdedup(self._h, C.byref(d), *args), "set_readdedup")
        return self

    @property
    def readdedup(self):
        """The ReadDedupResult of the last run's set_readdedup hook, or None when that run did not complete one."""
        res, ch = _lib.PpgReadDedupResult(), np.zeros(self.n, np.int64)
        if lib.ppg_shard_readdedup_ready(self._h, _ptr(ch), C.byref(res)) != 1:
            return None
        dd = getattr(self, "_dd", None) or (None, None, None, None)
        return ReadDedupResult(res, ch, dd[0], dd[2], dd[3])

    def select_size(self, mask=None):
        """(records, bytes) a selection by `mask` holds, after a run of any number of batches
        (ppg_shard_select_size): the capacities its SelectedRecords needs.  mask: None (every record),
        a SeqQuery made with mask=True, or an int32 / uint32 CUDA tensor of hit-mask words."""
        ptr, cap, _ = _mask_arg(mask, "select_size")
        self._torch_order()
        rec, nb = C.c_int64(), C.c_int64()
        check(lib.ppg_shard_select_size(self._h, ptr, cap, C.byref(rec), C.byref(nb)), "select_size")
        return rec.value, nb.value

    def select_records(self, mask=None, out=None):
        """The records `mask` selects of a one-batch shard after its run (ppg_shard_select_records), as a
        SelectedRecords of CUDA tensors on this device: into `out`, or into a new one sized by
        select_size().  Ordered after torch's stream, complete on return."""
        ptr, cap, _ = _mask_arg(mask, "select_records")
        if out is None:
            rec, nb = self.select_size(mask)
            out = SelectedRecords.empty(rec, nb, self.dev.device)
        out._check_device("select_records")
        self.dev.after_torch()
        rec, nb = C.c_int64(), C.c_int64()
        check(lib.ppg_shard_select_records(self._h, ptr, cap, *out._ptrs(), C.byref(rec), C.byref(nb)), "select_records")
        out.records, out.nbytes = rec.value, nb.value
        return out

    def set_select(self, mask=None, out=None):
        """From the next run on, every output batch appends the records `mask` selects to `out` (a
        SelectedRecords of CUDA tensors on this device, sized for the whole shard) while its output is
        resident (ppg_shard_set_select): works for shards of any number of batches, and runs after a
        set_seqquery hook that fills the same mask tensor; the result is `selected` after the run.
        mask as in select_size; out=None turns the hook off."""
        if out is None:
            check(lib.ppg_shard_set_select(self._h, None, 0, None, None, None, 0, None, 0), "set_select")
            self._select = None
            return self
        ptr, cap, keep = _mask_arg(mask, "set_select")
        out._check_device("set_select")
        self._select = (keep, out)   # kept alive while the library may read / write them
        self.dev.after_torch()
        check(lib.ppg_shard_set_select(self._h, ptr, cap, *out._ptrs()), "set_select")
        return self

    @property
    def selected(self):
        """The SelectedRecords of the last run's set_select hook, or None when that run did not complete one."""
        rec, nb = C.c_int64(), C.c_int64()
        sel = getattr(self, "_select", None)
        if lib.ppg_shard_select_ready(self._h, C.byref(rec), C.byref(nb)) != 1 or sel is None:
            return None
        sel[1].records, sel[1].nbytes = rec.value, nb.value
        return sel[1]

    def results(self):
        n = self.n
        rec, prod, end = (np.zeros(n, np.int64) for _ in range(3))
        st, fl = np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(lib.ppg_shard_results(self._h, _ptr(rec), _ptr(prod), _ptr(st), _ptr(fl), _ptr(end)), "results")
        return {"records": rec, "produced": prod, "status": st, "flags": fl, "end_bit": end}

    @property
    def total_records(self):
        return lib.ppg_shard_total_records(self._h)

    def chunk_bytes(self, k):
        o0, _, _, _ = self.index.point_fields(self.first + k)
        o1, _, _, _ = self.index.point_fields(self.first + k + 1)
        dst = np.zeros(max(1, o1 - o0), np.uint8)
        ln = C.c_int64()
        check(lib.ppg_shard_copy_chunk(self._h, k, _ptr(dst), dst.size, C.byref(ln)), "copy_chunk")
        return dst[:ln.value]

    def chunk_records(self, k):
        nrec = C.c_int64()
        check(lib.ppg_shard_copy_records(self._h, k, None, 0, C.byref(nrec)), "copy_records")
        dst = np.zeros((max(1, nrec.value), 4), np.uint32)
        check(lib.ppg_shard_copy_records(self._h, k, _ptr(dst), dst.shape[0], C.byref(nrec)), "copy_records")
        return dst[:nrec.value]

    def record_base(self):
        b = np.zeros(self.n, np.int64)
        check(lib.ppg_shard_record_base(self._h, _ptr(b)), "record_base")
        return b

    def counts_to_device(self, dev_ptr):
        self._torch_order()
        check(lib.ppg_shard_counts_to_device(self._h, C.c_void_p(int(dev_ptr))), "counts_to_device")

    def timing(self):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib.ppg_shard_timing(self._h, C.byref(a), C.byref(b), C.byref(c)), "timing")
        return {"inflate_ms": a.value, "parse_ms": b.value, "total_ms": c.value}


class Comm:
    """ppg_comm: the communicator of multi-GPU DecompressAll's count all-gather (include/ppgpu.h).

    Comm.rccl(device, nranks, rank, uid)  RCCL, from a PPG_COMM_ID_BYTES id made by
                                          Comm.unique_id() on rank 0 and handed to every rank
    Comm.host(nranks, rank, name)         shared memory between processes of one machine (the
                                          one-GPU rehearsal: RCCL refuses two ranks on one GPU)"""

    def __init__(self, handle, device=None):
        self._h = C.c_void_p(handle)
        self.dev = device

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(lib.ppg_comm_unique_id(buf), "ppg_comm_unique_id")
        return bytes(buf)

    @classmethod
    def rccl(cls, device, nranks, rank, uid):
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        check(lib.ppg_comm_init(device.handle, int(nranks), int(rank), buf, C.byref(h)), "ppg_comm_init")
        return cls(h.value, device)

    @classmethod
    def host(cls, nranks, rank, name):
        h = C.c_void_p()
        check(lib.ppg_comm_init_host(int(nranks), int(rank), name.encode(), C.byref(h)), "ppg_comm_init_host")
        return cls(h.value)

    @property
    def handle(self):
        return self._h

    def alltoallv(self, send, counts):
        """ppg_comm_alltoallv over host memory (the host transport): counts[src, dst] int64 values go
        from rank src to rank dst; `send` holds this rank's by destination.  Returns what this rank
        receives, by source."""
        c = np.ascontiguousarray(counts, np.int64)
        r, n = self.rank_size()
        assert c.shape == (n, n)
        snd = np.ascontiguousarray(send, np.int64)
        assert snd.size == c[r].sum()
        rcv = np.zeros(max(1, int(c[:, r].sum())), np.int64)
        check(lib.ppg_comm_alltoallv(self._h, _ptr(snd if snd.size else np.zeros(1, np.int64)), _ptr(rcv), _ptr(c), 0),
              "ppg_comm_alltoallv")
        return rcv[:int(c[:, r].sum())]

    def rank_size(self):
        r, n = C.c_int32(), C.c_int32()
        check(lib.ppg_comm_rank(self._h, C.byref(r), C.byref(n)), "ppg_comm_rank")
        return r.value, n.value

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.ppg_comm_free(h)
            self._h = None

    def __del__(self):
        self.close()


def build_info():
    """The library in use: ppg_version() and ppg_build_id() (a hash of the inflate kernels' object)."""
    return {"ppg_version": lib.ppg_version().decode(), "build_id": lib.ppg_build_id().decode()}


def rccl_version():
    v = C.c_int()
    return v.value if lib.ppg_rccl_version(C.byref(v)) == 0 else None


def partition(index, nranks, first=0, n=None):
    """ppg_partition: contiguous chunk ranges balanced by compressed bytes -> bounds[nranks + 1]."""
    if n is None:
        n = index.Count - 1 - first
    b = np.zeros(nranks + 1, np.int32)
    check(lib.ppg_partition(index.handle, int(first), int(n), int(nranks), _ptr(b)), "ppg_partition")
    return b


def gather_counts(shard, comm, bounds):
    """ppg_shard_gather_counts: (counts, bases, total) of every chunk of [bounds[0], bounds[-1])."""
    bounds = np.ascontiguousarray(bounds, np.int32)
    m = int(bounds[-1] - bounds[0])
    counts, bases = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
    tot = C.c_int64()
    check(lib.ppg_shard_gather_counts(shard.handle, comm.handle, _ptr(bounds), _ptr(counts), _ptr(bases),
                                      C.byref(tot)), "ppg_shard_gather_counts")
    return counts[:m], bases[:m], tot.value


def dist_decompress_all(index, gzip_path, comm, device=None, out_capacity=0):
    """ppg_dist_decompress_all: this rank's share of the file decoded, counts gathered over comm.
    Returns (counts, bases, total) over every chunk of the index."""
    dev = device or Device.default()
    m = index.Count - 1
    counts, bases = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
    tot = C.c_int64()
    check(lib.ppg_dist_decompress_all(dev.handle, comm.handle, index.handle, os.fsencode(gzip_path),
                                      int(out_capacity), _ptr(counts), _ptr(bases), C.byref(tot)),
          "ppg_dist_decompress_all")
    return counts[:m], bases[:m], tot.value


def decompress_file(index, gzip_path, first=0, n=None, piece_bytes=8 << 30, threads=8, device=None):
    """DecompressAll of chunks [first, first+n) straight from a .gz file (ppg_file_decompress_all):
    reader threads pread ~piece_bytes pieces into pinned buffers, H2D overlaps the decode of the
    previous piece (the LazyFileReader path, Decompressor/LazyFileReader.cs:10-98).
    Returns (per-chunk record counts, total records, wall seconds)."""
    dev = device or Device.default()
    if n is None:
        n = index.Count - 1 - first
    rec = np.zeros(max(n, 1), np.int64)
    tot = C.c_int64(0)
    sec = C.c_double(0)
    check(lib.ppg_file_decompress_all(dev.handle, index.handle, os.fsencode(gzip_path), int(first), int(n),
                                      int(piece_bytes), int(threads), _ptr(rec), C.byref(tot), C.byref(sec)),
          "decompress_file")
    return rec[:n], tot.value, sec.value


class Cursor:
    """Bounded-memory record streaming (ppg_cursor): chunks [first, first+n) of a .gz file in
    batches of whole chunks of at most batch_bytes of text, read and decoded on the GPU while the
    previous batch is consumed.  Iterating yields Batch objects; a batch's arrays are views of the
    library's pinned buffers and stay valid only until the next batch is requested (as a
    FastqRecord is invalid after the next MoveNext, BatchedFASTQ.cs:56).

    packed=True opens the packed enumerator (ppg_cursor_open_packed): a batch then carries no text
    and no descriptors but Batch.packed, a host PackedReads over the pinned planes (with the quality
    plane when quality=True), so a fraction of the bytes crosses PCIe.

    pattern=b"..." opens the filtered enumerator (ppg_cursor_open_select; not with packed=True): every
    batch is searched for the pattern on the GPU and carries only Batch.selected, a host SelectedRecords
    of the records whose Sequence contains it (b"": every record); nrecords counts the records scanned.

    filter=ReadFilter(...) (ppg_cursor_open_filter; alone or with pattern=, not with packed=True) narrows
    that selection to the hits that pass the filter, decided on the GPU as well; Batch.filter_result is
    then the batch's ReadFilterResult, over all its records.

    trim=ReadTrim(...) (ppg_cursor_open_trim; alone or with pattern= / filter=, not with packed=True) trims
    every record on the GPU, narrows the selection to the records that are still min_length long, and
    hands out the windows: Batch.selected.trim and .trimmed(i); Batch.trim_result is the batch's
    ReadTrimResult, over all its records."""

    def __init__(self, index, gzip_path, first=0, n=None, batch_bytes=1 << 30, threads=8, device=None,
                 packed=False, quality=True, pattern=None, filter=None, trim=None):   # noqa: A002
        if packed and (pattern is not None or filter is not None or trim is not None):
            raise ValueError("Cursor: packed=True and pattern= / filter= / trim= exclude each other")
        if (filter is not None or trim is not None) and pattern is None:
            pattern = b""
        self.index = index
        self.dev = device or Device.default()
        if n is None:
            n = index.Count - 1 - first
        self.packed, self.quality = bool(packed), bool(quality)
        self.select = pattern is not None
        self.filtered = filter is not None
        self.trimming = trim is not None
        h = C.c_void_p()
        if self.trimming:
            pat, m = _pattern_arg(pattern)
            f = _filter_struct(filter) if self.filtered else None
            t = _trim_struct(trim)
            check(lib.ppg_cursor_open_trim(self.dev.handle, index.handle, os.fsencode(gzip_path), int(first), int(n),
                                           int(batch_bytes), int(threads), pat, m, C.byref(f) if self.filtered else None,
                                           C.byref(t), C.byref(h)), "ppg_cursor_open_trim")
        elif self.filtered:
            pat, m = _pattern_arg(pattern)
            f = _filter_struct(filter)
            check(lib.ppg_cursor_open_filter(self.dev.handle, index.handle, os.fsencode(gzip_path), int(first), int(n),
                                             int(batch_bytes), int(threads), pat, m, C.byref(f), C.byref(h)),
                  "ppg_cursor_open_filter")
        elif self.select:
            pat, m = _pattern_arg(pattern)
            check(lib.ppg_cursor_open_select(self.dev.handle, index.handle, os.fsencode(gzip_path), int(first), int(n),
                                             int(batch_bytes), int(threads), pat, m, C.byref(h)), "ppg_cursor_open_select")
        elif packed:
            check(lib.ppg_cursor_open_packed(self.dev.handle, index.handle, os.fsencode(gzip_path), int(first), int(n),
                                             int(batch_bytes), int(threads), 1 if quality else 0, C.byref(h)),
                  "ppg_cursor_open_packed")
        else:
            check(lib.ppg_cursor_open(self.dev.handle, index.handle, os.fsencode(gzip_path), int(first), int(n),
                                      int(batch_bytes), int(threads), C.byref(h)), "ppg_cursor_open")
        self._h = h
        self.dev._retain()

    def __del__(self):
        self.close()

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.ppg_cursor_close(h)
            self._h = None
            self.dev._release()

    @property
    def batches(self):
        return lib.ppg_cursor_batches(self._h)

    def next_batch(self):
        b = PpgBatch()
        rc = lib.ppg_cursor_next(self._h, C.byref(b))
        if rc == PPG_STREAM_END:
            return None
        check(rc, "ppg_cursor_next")
        return Batch(b, self.packed_reads(b.nrecords) if self.packed else None,
                     self.selected_records() if self.select else None, self.filter_result() if self.filtered else None,
                     self.trim_result() if self.trimming else None)

    def trim_result(self):
        """The current batch's ReadTrimResult (ppg_cursor_trim_result): totals alone."""
        res = _lib.PpgReadTrimResult()
        check(lib.ppg_cursor_trim_result(self._h, C.byref(res)), "ppg_cursor_trim_result")
        return ReadTrimResult(res)

    def filter_result(self):
        """The current batch's ReadFilterResult (ppg_cursor_filter_result): totals alone."""
        res = _lib.PpgReadFilterResult()
        check(lib.ppg_cursor_filter_result(self._h, C.byref(res)), "ppg_cursor_filter_result")
        return ReadFilterResult(res)

    def selected_records(self):
        """The current batch's selection (ppg_cursor_selected / ppg_cursor_selected_index) as a host
        SelectedRecords: bytes and desc are views of pinned memory, valid until the next batch; sel_off
        (batch-relative) and recno (among the records this cursor hands out) are copies; with a trim,
        trim is a view of pinned memory as well (ppg_cursor_selected_trim)."""
        pb, pd = C.c_void_p(), C.c_void_p()
        rec, nb = C.c_int64(), C.c_int64()
        check(lib.ppg_cursor_selected(self._h, C.byref(pb), C.byref(pd), C.byref(rec), C.byref(nb)), "ppg_cursor_selected")
        nr, nb = rec.value, nb.value
        off, recno = np.zeros(nr + 1, np.int64), np.zeros(max(nr, 1), np.int64)
        check(lib.ppg_cursor_selected_index(self._h, _ptr(off), _ptr(recno), nr), "ppg_cursor_selected_index")

        def view(p, ct, n):
            if not n or not p.value:
                return np.zeros(0, ct)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (n,))

        trim = None
        if self.trimming:
            pt = C.c_void_p()
            check(lib.ppg_cursor_selected_trim(self._h, C.byref(pt)), "ppg_cursor_selected_trim")
            trim = view(pt, C.c_uint32, 2 * nr).reshape(-1, 2)
        return SelectedRecords(view(pb, C.c_uint8, nb), off, view(pd, C.c_uint32, 4 * nr).reshape(-1, 4), recno[:nr], nr, nb,
                               trim)

    def packed_reads(self, nrecords):
        """The current batch's planes (ppg_cursor_packed / ppg_cursor_packed_offsets) as a host
        PackedReads: views of pinned memory, valid until the next batch; seq_off is a copy."""
        pb, pm, pq, pl = (C.c_void_p() for _ in range(4))
        tot = C.c_int64()
        check(lib.ppg_cursor_packed(self._h, C.byref(pb), C.byref(pm), C.byref(pq), C.byref(pl), C.byref(tot)),
              "ppg_cursor_packed")
        nr, nb = int(nrecords), tot.value
        off = np.zeros(nr + 1, np.int64)
        check(lib.ppg_cursor_packed_offsets(self._h, _ptr(off), off.size), "ppg_cursor_packed_offsets")

        def view(p, ct, n):
            if not n or not p.value:
                return np.zeros(0, ct)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (n,))

        qual = view(pq, C.c_uint8, nb) if pq.value else None
        return PackedReads(off, view(pl, C.c_uint32, nr), view(pb, C.c_uint32, nb // 16), view(pm, C.c_uint32, nb // 32),
                           qual, nr, nb)

    def __iter__(self):
        while True:
            b = self.next_batch()
            if b is None:
                return
            yield b


class Batch:
    """One ppg_batch: text (uint8), raw_off / rec_off (int64, nchunks + 1), desc (nrecords x 4).  A
    packed cursor's batch has text = desc = None and `packed`, a host PackedReads; a select cursor's
    has text = desc = None and `selected`, a host SelectedRecords, and with a filter `filter_result`, the
    batch's ReadFilterResult, with a trim `trim_result`, its ReadTrimResult."""

    def __init__(self, b, packed=None, selected=None, filter_result=None, trim_result=None):
        self.first_chunk, self.nchunks = b.first_chunk, b.nchunks
        self.record_base, self.nrecords = b.record_base, b.nrecords
        self.raw_off = np.ctypeslib.as_array(b.raw_off, (b.nchunks + 1,))
        self.rec_off = np.ctypeslib.as_array(b.rec_off, (b.nchunks + 1,))
        self.packed = packed
        self.selected = selected
        self.filter_result = filter_result
        self.trim_result = trim_result
        if packed is not None or selected is not None or not b.text:
            self.text = self.desc = None
            return
        nt = int(self.raw_off[-1])
        self.text = np.ctypeslib.as_array(C.cast(b.text, C.POINTER(C.c_uint8)), (max(nt, 1),))[:nt]
        nd = 4 * int(b.nrecords)
        self.desc = np.ctypeslib.as_array(b.desc, (max(nd, 1),))[:nd].reshape(-1, 4)

    def raw(self, k):
        """raw_k = offset_k ++ chunk_k of the batch's k-th chunk."""
        return self.text[self.raw_off[k]:self.raw_off[k + 1]]

    def records(self, k):
        """Descriptors (n, 4) of the batch's k-th chunk."""
        return self.desc[self.rec_off[k]:self.rec_off[k + 1]]


class BatchedFASTQ:
    """Decompressor/BatchedFASTQ.cs:10-101 — DecompressAll as an iterable of FastqRecord.

    The reference yields records in a nondeterministic interleaving; this yields the
    canonical order: chunk 0's records, then chunk 1's, ...  enable_ssd_optimization is accepted
    for signature parity (it selected 1 or 8 FileStreams, LazyFileReader.cs:27-33)."""

    def __init__(self, index, gzip_path, enable_ssd_optimization=False, device=None, rank=None, world=None,
                 comm=None):
        if isinstance(index, (str, os.PathLike)):
            index = IndexIO.Deserialize(index)
        self.index = index
        self.gzip_path = gzip_path
        self.enable_ssd_optimization = enable_ssd_optimization
        self.dev = device
        self._shard = None
        self._qshard = None   # CountPattern / CountBases: (out_capacity, Shard), kept until Dispose()
        # one rank of a multi-GPU job (the reference's Task.Run fan-out, BatchedFASTQ.cs:62-77, on
        # GPUs): iteration yields this rank's share -- the contiguous chunk range ppg_partition
        # gives it -- so the ranks' records, concatenated in rank order, are the file's
        # comm (a Comm of this job): Count() decodes only this rank's share and gathers every rank's
        # counts (ppg_dist_decompress_all), as the C# GpuBatchedFASTQ(..., GpuJob) does
        self.comm = comm
        if comm is not None and world is None:
            rank, world = comm.rank_size()
        self.rank, self.world = rank, world
        if (rank is None) != (world is None) or (world is not None and not 0 <= rank < world):
            raise ValueError("rank and world go together, 0 <= rank < world")

    def chunk_range(self):
        """(first, n): the chunks this enumerator streams (all of them, or this rank's share)."""
        m = self.index.Count - 1
        if self.world is None:
            return 0, m
        b = partition(self.index, self.world, 0, m)
        return int(b[self.rank]), int(b[self.rank + 1] - b[self.rank])

    def _run(self):
        if self._shard is None:
            n = self.index.Count - 1
            _, i0, _, _ = self.index.point_fields(0)
            _, i1, _, _ = self.index.point_fields(n)
            with open(self.gzip_path, "rb") as f:
                f.seek(i0 - 1)
                comp = f.read(i1 - i0 + 1)
            self._shard = Shard(self.index, comp, 0, n, device=self.dev).run()
        return self._shard

    def Count(self):
        """Number of records (Enumerable.Count over the enumerator, Decompressor/Program.cs:48-52):
        streamed from the file, nothing materialised on the host."""
        if self._shard is not None:
            return self._shard.total_records
        if self.world is not None:
            # one rank of a job: its own share decoded, the counts gathered -- every rank returns the
            # whole file's total (never each rank decoding the whole file)
            if self.comm is None:
                raise ValueError("Count() of a rank's BatchedFASTQ needs the job's comm (BatchedFASTQ(..., comm=))")
            _, _, total = dist_decompress_all(self.index, self.gzip_path, self.comm, device=self.dev)
            return total
        _, total, _ = decompress_file(self.index, self.gzip_path, device=self.dev,
                                      threads=16 if self.enable_ssd_optimization else 8)
        return total

    # text per streamed batch (ppg_cursor): up to five batches in flight, each ~1.13x this + its
    # compressed bytes of pinned host memory (ppg_cursor_open caps the slots by available memory)
    batch_bytes = 1 << 30

    def __iter__(self):
        """Records streamed through ppg_cursor in bounded memory, canonical chunk order; each
        batch's bytes are copied out before the next one is requested."""
        first, n = self.chunk_range()
        cur = Cursor(self.index, self.gzip_path, first=first, n=n, batch_bytes=self.batch_bytes,
                     threads=16 if self.enable_ssd_optimization else 8, device=self.dev)
        try:
            for b in cur:
                for k in range(b.nchunks):
                    yield from records_from_descriptors(b.raw(k).tobytes(), b.records(k))
        finally:
            cur.close()

    def Where(self, pattern=None, filter=None, trim=None):   # noqa: A002
        """The records whose Sequence contains `pattern` (the body of Benchmark/Naive.cs RunPattern's
        loop: foreach record, if record.Sequence.Contains(pattern)), in canonical order, through the
        select cursor (ppg_cursor_open_select) over chunk_range(): searched and compacted on the GPU,
        only the hits reach the host.  Each batch's bytes are copied out before the next one is
        requested.  pattern as in CountPattern (None or b"": every record).  filter: a ReadFilter the
        records must pass as well (ppg_cursor_open_filter), decided on the GPU too.  trim: a ReadTrim
        (ppg_cursor_open_trim): the records are trimmed on the GPU, those shorter than its min_length
        afterwards are dropped, and the rest come as TrimmedRecord with trimmed_sequence / trimmed_quality."""
        first, n = self.chunk_range()
        cur = Cursor(self.index, self.gzip_path, first=first, n=n, batch_bytes=self.batch_bytes,
                     threads=16 if self.enable_ssd_optimization else 8, device=self.dev,
                     pattern=b"" if pattern is None else pattern, filter=filter, trim=trim)
        try:
            for b in cur:
                sel = b.selected
                raw = sel.bytes.tobytes()
                off, desc = sel.sel_off.tolist(), sel.desc.tolist()
                win = sel.trim.tolist() if trim is not None else None
                for i in range(sel.records):
                    if win is None:
                        yield FastqRecord(raw[off[i]:off[i + 1]], 0, *desc[i])
                    else:
                        yield TrimmedRecord(raw[off[i]:off[i + 1]], 0, *desc[i], *win[i])
        finally:
            cur.close()

    # decompressed bytes resident per batch of CountPattern / CountBases: the shard runs the file in
    # batches of whole chunks no larger than this, so a file of any size is scanned in bounded memory
    query_out_capacity = 256 << 20

    def _query_shard(self):
        if self.world is not None:
            raise ValueError("CountPattern / CountBases / CountPassing run in a single process (no rank / world)")
        cap, sh = getattr(self, "_qshard", None) or (None, None)
        if sh is None or cap != self.query_out_capacity:
            # the file's compressed bytes go to the device once (from the page cache, no host copy) and
            # stay there with one batch of output until Dispose(): a second query only runs again
            n = self.index.Count - 1
            _, i0, _, _ = self.index.point_fields(0)
            _, i1, _, _ = self.index.point_fields(n)
            comp = np.memmap(self.gzip_path, np.uint8, "r", offset=i0 - 1, shape=(i1 - i0 + 1,))
            cap = self.query_out_capacity
            sh = Shard(self.index, comp, 0, n, device=self.dev, out_capacity=cap)
            self._qshard = (cap, sh)
        return sh

    def _stage_shard(self):
        """The query shard with every record-stage hook off: each Count* / Profile attaches its own."""
        sh = self._query_shard().set_seqquery(None).set_readfilter(None).set_readtrim(None).set_readprofile(None)
        return sh.set_readdedup(None)

    def _query(self, pattern):
        return self._stage_shard().set_seqquery(pattern).run().seqquery

    def CountPassing(self, filter):   # noqa: A002
        """The ReadFilterResult of `filter` (a ReadFilter) over the file: how many records pass, how many
        fail each criterion, and the totals, measured on the GPU batch by batch (Shard.set_readfilter):
        no record text reaches the host."""
        return self._stage_shard().set_readfilter(filter).run().readfilter

    def CountTrimmed(self, trim):
        """The ReadTrimResult of `trim` (a ReadTrim) over the file: how many records each cut moves, how
        many are kept and the bases left, measured on the GPU batch by batch (Shard.set_readtrim): totals
        alone, no record text and no window reaches the host."""
        return self._stage_shard().set_readtrim(trim).run().readtrim

    def _stage_records(self, sh):
        """The file's records: one run without hooks counts them, once per query shard (the tensors' sizes)."""
        nrec = getattr(sh, "_profile_records", None)
        if nrec is None:
            nrec = sh._profile_records = max(sh.run().total_records, 0)
        return nrec

    def _chain(self, sh, nrec, pattern, filter, trim, dedup):   # noqa: A002
        """Attaches the query / filter / trim / dedup hooks that are given to one mask tensor and one rows
        tensor; (mask, rows), each None when no stage needs it."""
        import torch
        dev = torch.device("cuda", sh.dev.device)
        masked = pattern is not None or filter is not None or trim is not None
        mask = torch.full(((nrec + 31) // 32 + 1,), -1, dtype=torch.int32, device=dev) if masked or dedup is not None else None
        rows = torch.zeros((nrec + 1, 2), dtype=torch.int32, device=dev) if trim is not None else None
        if pattern is not None:
            sh.set_seqquery(pattern, mask=mask)   # writes the words; the later stages AND into them
        if filter is not None:
            sh.set_readfilter(filter, mask=mask, and_mask=True)
        if trim is not None:
            sh.set_readtrim(trim, mask=mask, windows=rows, and_mask=True)
        if dedup is not None:
            table = torch.zeros((ReadDedup.min_slots(nrec), 3), dtype=torch.int64, device=dev)
            sh.set_readdedup(dedup, mask=mask, windows=rows, table=table, and_mask=True)
        return mask, rows

    def Duplication(self, dedup=None, pattern=None, filter=None, trim=None):   # noqa: A002
        """The ReadDedupResult of the file: how many reads are first occurrences, the duplication levels and the
        most frequent read (dedup: a ReadDedup, None for whole reads), made on the GPU batch by batch against
        one table in device memory (Shard.set_readdedup).  With pattern / filter / trim it is the duplication
        among the reads that contain the pattern, pass the filter and are kept by the trim, keyed inside the
        trim's windows.  One counting run gives the sizes; one mask, one rows tensor and one table are chained
        through the hooks, and nothing but the result leaves the device."""
        sh = self._stage_shard()
        nrec = self._stage_records(sh)
        try:
            self._chain(sh, nrec, pattern, filter, trim, ReadDedup() if dedup is None else dedup)
            return sh.run().readdedup
        finally:
            self._stage_shard()

    def CountUnique(self, dedup=None, pattern=None, filter=None, trim=None):   # noqa: A002
        """The number of first occurrences Duplication() finds."""
        return self.Duplication(dedup, pattern, filter, trim).unique

    def Profile(self, profile=None, pattern=None, filter=None, trim=None, dedup=None):   # noqa: A002
        """The ReadProfileResult of the file: bases and qualities per read position, read lengths, GC
        content and mean quality per read (profile: a ReadProfile, None for the default), made on the GPU
        batch by batch (Shard.set_readprofile).  With pattern / filter / trim it is the profile of the
        reads that contain the pattern, pass the filter and are kept by the trim, inside the trim's
        windows: one mask tensor and one rows tensor are chained through the hooks on the device, and
        nothing but the result leaves it.  dedup (a ReadDedup): of those, the first occurrences only."""
        sh = self._stage_shard()
        profile = ReadProfile() if profile is None else profile
        if pattern is None and filter is None and trim is None and dedup is None:
            return sh.set_readprofile(profile).run().readprofile
        nrec = self._stage_records(sh)
        try:
            mask, rows = self._chain(sh, nrec, pattern, filter, trim, dedup)
            return sh.set_readprofile(profile, mask=mask, windows=rows).run().readprofile
        finally:
            self._stage_shard()

    def CountKmers(self, kmers=None, pattern=None, filter=None, trim=None, dedup=None, slots=None):   # noqa: A002
        """The KmerCountResult of the file: the k-mer spectrum, the totals and the table of every k-mer's count
        (kmers: a KmerCount, None for k = 21 canonical), counted on the GPU (count_kmers).  The reads are packed
        without qualities while each batch is resident (Shard.set_seqpack), so a file of any number of batches leaves
        its whole packed set on the device; with pattern / filter / trim / dedup the same run chains their hooks onto
        one mask and one rows tensor as Profile does, and the k-mers are those of the reads that contain the pattern,
        pass the filter, are kept by the trim and (dedup) are first occurrences, inside the trim's windows.  A record
        the reference parses twice counts twice, as in the profile; with dedup the second is dropped.  slots: the
        table's size (None: sized by doubling)."""
        sh = self._stage_shard()
        nrec = self._stage_records(sh)
        tot, rec = sh.seq_bases()
        packed = PackedReads.empty(rec, tot, False, sh.dev.device)
        try:
            sh.set_seqpack(packed)
            mask, rows = self._chain(sh, nrec, pattern, filter, trim, dedup)
            sh.run()
            if not sh.seqpack_ready:
                raise ValueError("CountKmers: the shard's run did not fill the packed reads")
            return count_kmers(packed, kmers, mask=mask, windows=rows, slots=slots, device=sh.dev)
        finally:
            sh.set_seqpack(None)
            self._stage_shard()

    def QualityCounts(self):
        """numpy int64[256]: the bytes of every Quality line by value, counted on the GPU batch by batch."""
        return self.CountPassing(ReadFilter()).qual_count

    def CountPattern(self, pattern):
        """Number of records whose Sequence contains `pattern` (Benchmark/Naive.cs RunPattern:
        records.Count(r => r.Sequence.Contains(pattern))), searched on the GPU batch by batch
        (Shard.set_seqquery): no record text reaches the host."""
        return self._query(b"" if pattern is None else pattern).hits

    def CountBases(self):
        """{'A', 'C', 'G', 'T', 'other'}: the bytes of every Sequence by class (Decompressor/Program.cs:20-21
        counts the 'A's this way), counted on the GPU batch by batch."""
        return dict(self._query(b"").counts)

    def Dispose(self):
        self._shard = None
        self._qshard = None
