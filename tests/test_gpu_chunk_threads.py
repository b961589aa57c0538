"""README "Decompress" must be thread safe (/root/reference/README.md:38-50; the reference runs
Core.ExtractDeflateIndex from one ThreadPool task per chunk, BatchedFASTQ.cs:62-77).
ppg_decompress_chunk is called from 8 host threads on ONE ctx over every chunk of golden files and
of a 200k-record file; every call's bytes and record table must equal the oracle's (golden SHA-256 /
oracle.c's Extract + Parse), concurrent calls must have shared launches, and a bad request in a
launch must fail alone."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import parallelparsing_amd as pp
from conftest import load_case
from oracle import oracle as O
from parallelparsing_amd import _lib

pytestmark = pytest.mark.gpu
THREADS = 8


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def slice_of(gz, ix, k):
    _, i0, _, _ = ix.point_fields(k)
    _, i1, _, _ = ix.point_fields(k + 1)
    return np.frombuffer(gz[i0 - 1:i1], np.uint8)


def run_threads(work, nthreads=THREADS):
    """work(tid) in nthreads threads started together; re-raises the first failure."""
    errs = []
    bar = threading.Barrier(nthreads)

    def body(t):
        try:
            bar.wait()
            work(t)
        except BaseException as e:   # noqa: BLE001 - re-raised below
            errs.append(e)
    th = [threading.Thread(target=body, args=(t,)) for t in range(nthreads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise errs[0]


def chunk_calls(gz, ix, dev, jobs, check):
    """8 threads pull (k) from `jobs` and decode it with ppg_decompress_chunk on one ctx."""
    lock = threading.Lock()
    it = iter(jobs)

    def work(_):
        while True:
            with lock:
                k = next(it, None)
            if k is None:
                return
            got, buf, rec = pp.Core.ExtractDeflateIndex(slice_of(gz, ix, k), ix, k, device=dev, with_records=True)
            check(k, buf[:got], rec)
    run_threads(work)


@pytest.mark.parametrize("name", ["l6_c20", "memlevel1_c10", "huffonly_c20", "pigz_c100", "crlf_c100"])
def test_threads_golden(name):
    meta, gz = load_case(name)
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(gz, meta["chunksize"])
    n = ix.Count - 1

    def check(k, b, rec):
        c = meta["chunks"][k]
        assert len(b) == c["out_len"] and sha(b) == c["sha256"], (name, k)
        assert len(rec) == c["records"], (name, k)
        assert sha(np.ascontiguousarray(rec, "<u4").tobytes()) == c["rec_sha256"], (name, k)
    chunk_calls(gz, ix, dev, [k for _ in range(3) for k in range(n)], check)
    st = dev.decompress_chunk_stats()
    assert st["calls"] == 3 * n


def synth_gz(nrec, seed):
    S = pp.synth()
    sz = S.ppg_synth_fastq_size(0, nrec, 150)
    txt = np.zeros(sz, np.uint8)
    S.ppg_synth_fastq(seed, 0, nrec, 150, C.c_void_p(txt.ctypes.data), sz, 8)
    gzb = np.zeros(sz, np.uint8)
    L = S.ppg_synth_gzip(C.c_void_p(txt.ctypes.data), sz, 6, 4 << 20, 8, C.c_void_p(gzb.ctypes.data), gzb.size)
    return gzb[:L].tobytes()


@pytest.fixture(scope="module")
def file200k():
    gz = synth_gz(200_000, 5)
    oi = O.build_index(gz, 2000)
    exp = []
    for k in range(oi.count - 1):
        b = O.extract(gz, oi, k)
        exp.append((sha(b), O.parse(oi.point(k)[4], b)))
    return gz, exp


def test_threads_200k_records_vs_oracle(file200k):
    """~100 chunks of a 200k-record member, each decoded twice by 8 threads on one ctx: bytes and
    records equal the oracle's; the calls were combined into fewer launches."""
    gz, exp = file200k
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(gz, 2000)
    n = ix.Count - 1
    assert n == len(exp) and n > 80

    def check(k, b, rec):
        assert sha(b) == exp[k][0], k
        assert np.array_equal(rec, exp[k][1]), k
    chunk_calls(gz, ix, dev, list(range(n)) * 2, check)
    st = dev.decompress_chunk_stats()
    assert st["calls"] == 2 * n
    assert st["launches"] < st["calls"] and st["max_batch"] > 1, st
    # ~190 KB of gzip per chunk: the GPU search split (nearly) every chunk at its inner block starts
    assert st["split_chunks"] > n and st["side_points"] >= st["split_chunks"], st


@pytest.mark.parametrize("mat", [True, False])
def test_lone_chunks_found_side_points_vs_oracle(mat):
    """Chunks of 40,000 records (~4 MB of gzip) decoded one call at a time: each launch holds one
    chunk, whose inner block starts are found on the GPU (candidates, speculative symbolic decode,
    the verified chain from the chunk's Point, resolved histories) -- it is decoded as ~16 waves.
    Bytes and records equal the oracle's, and equal the one-wave decode (PPG_CHUNK_NO_FIND).
    mat: the materialise path (the default for plain indexes), or with PPG_CHUNK_NO_MAT the
    two-decode path (16 ranges of >= 48 KiB), which otherwise runs only in mixed launches."""
    import os
    gz = synth_gz(130_000, 11)
    oi = O.build_index(gz, 40_000)
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(gz, 40_000)
    n = ix.Count - 1
    assert n == oi.count - 1 and n >= 3
    before = dev.decompress_chunk_stats()
    for k in range(n):
        b = O.extract(gz, oi, k)
        if not mat:
            os.environ["PPG_CHUNK_NO_MAT"] = "1"
        try:
            got, buf, rec = pp.Core.ExtractDeflateIndex(slice_of(gz, ix, k), ix, k, device=dev, with_records=True)
        finally:
            os.environ.pop("PPG_CHUNK_NO_MAT", None)
        assert got == len(b) and sha(buf[:got]) == sha(b), k
        assert np.array_equal(rec, O.parse(oi.point(k)[4], b)), k
        os.environ["PPG_CHUNK_NO_FIND"] = "1"
        try:
            got2, buf2, rec2 = pp.Core.ExtractDeflateIndex(slice_of(gz, ix, k), ix, k, device=dev, with_records=True)
        finally:
            os.environ.pop("PPG_CHUNK_NO_FIND", None)
        assert got2 == got and sha(buf2[:got2]) == sha(b) and np.array_equal(rec2, rec), k
    st = dev.decompress_chunk_stats()
    split = st["split_chunks"] - before["split_chunks"]
    pts = st["side_points"] - before["side_points"]
    print(f"[found] {n} chunks split, {pts} side points")
    assert split == n and pts >= 2 * n, (split, pts)


def test_tiny_records_get_an_exact_table():
    """Records far under the wrappers' 64-B sizing ("@\nA\n+\n!\n": 8 bytes): the library reports
    the chunk's record count with PPG_BUF_ERROR and the wrapper decodes it again into an exact
    table -- synchronously and through the asynchronous entry point -- equal to the oracle's."""
    import zlib
    recs = [b"@%d\n%s\n+\n%s\n" % (i % 10, b"ACGT"[i % 4:i % 4 + 1], b"!?*"[i % 3:i % 3 + 1])
            for i in range(60_000)]
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    parts = []
    for g in range(0, len(recs), 5_000):   # a block end every 5,000 records: Points can fall there
        parts.append(co.compress(b"".join(recs[g:g + 5_000])))
        parts.append(co.flush(zlib.Z_FULL_FLUSH))
    parts.append(co.flush())
    gz = b"".join(parts)
    oi = O.build_index(gz, 20_000)
    ix = pp.Core.BuildDeflateIndex(gz, 20_000)
    dev = pp.Device(0)
    n = ix.Count - 1
    assert n >= 2
    futs = [pp.Core.ExtractDeflateIndexAsync(slice_of(gz, ix, k), ix, k, device=dev) for k in range(n)]
    for k in range(n):
        b = O.extract(gz, oi, k)
        exp = O.parse(oi.point(k)[4], b)
        if b:
            assert len(exp) > len(b) // 64 + 256   # more records than the first table holds
        got, buf, rec = pp.Core.ExtractDeflateIndex(slice_of(gz, ix, k), ix, k, device=dev, with_records=True)
        assert got == len(b) and sha(buf[:got]) == sha(b) and np.array_equal(rec, exp), k
        got, buf, rec = futs[k].result()
        assert got == len(b) and sha(buf[:got]) == sha(b) and np.array_equal(rec, exp), k


def test_threads_side_points_split_chunks(file200k):
    """An index with side points (GPU CreateIndex, side_bytes): each chunk is decoded as one wave
    per piece inside the combined launch -- results identical to the oracle's."""
    gz, exp = file200k
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndexGpu(gz, 2000, device=dev, side_bytes=64 << 10)
    assert len(ix.side_points()[0]) > ix.Count
    n = ix.Count - 1

    def check(k, b, rec):
        assert sha(b) == exp[k][0], k
        assert np.array_equal(rec, exp[k][1]), k
    chunk_calls(gz, ix, dev, list(range(n)), check)


def test_mixed_plain_and_side_point_indexes(file200k):
    """Two indexes of one member, one plain (no side points) and one with side points, their chunks
    0..15 queued interleaved on one device: a launch that holds both kinds takes the two-decode path
    (the index's side points for one, the GPU block search for the other).  Every result equals the
    oracle's, whichever launches the requests shared."""
    gz, exp = file200k
    dev = pp.Device(0)
    plain = pp.Core.BuildDeflateIndex(gz, 2000)
    side = pp.Core.BuildDeflateIndexGpu(gz, 2000, device=dev, side_bytes=64 << 10)
    assert len(plain.side_points()[0]) == 0 and len(side.side_points()[0]) > side.Count
    assert plain.Count == side.Count == len(exp) + 1
    futs = [(k, pp.Core.ExtractDeflateIndexAsync(slice_of(gz, ix, k), ix, k, device=dev))
            for k in range(16) for ix in (plain, side)]
    for k, f in futs:
        got, buf, rec = f.result()
        assert sha(buf[:got]) == exp[k][0], k
        assert np.array_equal(rec, exp[k][1]), k


def test_bad_requests_fail_alone(file200k):
    """In launches shared with good requests: a corrupted slice gets zlib's DATA_ERROR, a slice of
    the wrong length ARG_ERROR, a too-small output buffer BUF_ERROR -- each only its own call."""
    gz, exp = file200k
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(gz, 2000)
    n = ix.Count - 1
    outcomes = {}
    lock = threading.Lock()

    def work(t):
        for rep in range(4):
            k = (7 * t + 3 * rep) % n
            sl = slice_of(gz, ix, k).copy()
            kind = ("good", "corrupt", "short", "small")[(t + rep) % 4]
            try:
                if kind == "corrupt":
                    sl[len(sl) // 3: len(sl) // 3 + 64] ^= 0x5A
                    pp.Core.ExtractDeflateIndex(sl, ix, k, device=dev)
                elif kind == "short":
                    pp.Core.ExtractDeflateIndex(sl[:-1], ix, k, device=dev)
                elif kind == "small":
                    pp.Core.ExtractDeflateIndex(sl, ix, k, buf=np.zeros(10, np.uint8), device=dev)
                else:
                    got, buf, rec = pp.Core.ExtractDeflateIndex(sl, ix, k, device=dev, with_records=True)
                    assert sha(buf[:got]) == exp[k][0] and np.array_equal(rec, exp[k][1])
                code = 0
            except pp.PpgError as e:
                code = e.code
            with lock:
                outcomes.setdefault(kind, []).append(code)
    run_threads(work)
    assert set(outcomes["good"]) == {0}
    assert set(outcomes["short"]) == {_lib.PPG_ARG_ERROR}
    assert set(outcomes["small"]) == {_lib.PPG_BUF_ERROR}
    # a corrupted deflate stream: zlib's verdict for these bytes (DATA_ERROR, or garbage that
    # still decodes) -- never a device error, never another request's failure
    assert set(outcomes["corrupt"]) <= {0, _lib.PPG_DATA_ERROR, _lib.PPG_BUF_ERROR}


def test_async_submit_vs_oracle(file200k):
    """ppg_decompress_chunk_submit / _wait from ONE caller thread (the
    reference keeps 32 partitions queued, LazyFileReader.cs:14): every chunk of the 200k-record
    member queued twice before any wait, the launcher thread combines them into few launches, every
    result equals the oracle's; a bad request among them fails alone."""
    gz, exp = file200k
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(gz, 2000)
    n = ix.Count - 1
    before = dev.decompress_chunk_stats()
    futs = [(k, pp.Core.ExtractDeflateIndexAsync(slice_of(gz, ix, k), ix, k, device=dev)) for k in list(range(n)) * 2]
    bad = pp.Core.ExtractDeflateIndexAsync(slice_of(gz, ix, 3)[:-1], ix, 3, device=dev)   # short slice
    # too small a buffer: the launcher copies async results out itself (r05) -- BUF_ERROR, alone
    small = pp.Core.ExtractDeflateIndexAsync(slice_of(gz, ix, 5), ix, 5, buf=np.zeros(10, np.uint8), device=dev)
    for k, f in futs:
        got, buf, rec = f.result()
        assert sha(buf[:got]) == exp[k][0], k
        assert np.array_equal(rec, exp[k][1]), k
    with pytest.raises(pp.PpgError) as e:
        bad.result()
    assert e.value.code == _lib.PPG_ARG_ERROR
    with pytest.raises(pp.PpgError) as e:
        small.result()
    assert e.value.code == _lib.PPG_BUF_ERROR
    st = dev.decompress_chunk_stats()
    calls, launches = st["calls"] - before["calls"], st["launches"] - before["launches"]
    assert calls == 2 * n + 2 and launches <= 8, (calls, launches, st)


def test_async_and_threads_together(file200k):
    """Asynchronous requests queued beside 8 synchronous caller threads on one ctx: all served, all
    equal to the oracle's."""
    gz, exp = file200k
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(gz, 2000)
    n = ix.Count - 1
    futs = [(k, pp.Core.ExtractDeflateIndexAsync(slice_of(gz, ix, k), ix, k, device=dev)) for k in range(0, n, 2)]

    def check(k, b, rec):
        assert sha(b) == exp[k][0], k
        assert np.array_equal(rec, exp[k][1]), k
    chunk_calls(gz, ix, dev, list(range(1, n, 2)), check)
    for k, f in futs:
        got, buf, rec = f.result()
        check(k, buf[:got], rec)
