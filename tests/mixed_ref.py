"""Shards with failed chunks beside good ones: the corrupt inputs and their reference.

corrupt_chunk finds a byte flip inside one chunk's compressed range the way oracle/make_golden.py finds
corrupt_err: six bytes XORed with 0x5A, from input_k + 8 on in steps of 37, the first position where the oracle's
Extract of chunk k fails.  The flip lies strictly inside the bytes only chunk k reads, so every other chunk
extracts as before (asserted).  The reference of a shard with failed chunks is the clean input's oracle chunks with
each failed chunk replaced by an empty chunk -- no offset, no text, descriptors of shape (0, 4): a failed chunk
has no records (include/ppgpu.h) -- and the stages' references (pack_reference .. select_reference) take it from
there, so record numbers, unit layout, masks, tables and selections of the good chunks follow."""
import functools

import numpy as np

from oracle import oracle as O
import seqpack_ref as R

EMPTY = (b"", b"", np.zeros((0, 4), np.uint32))

# the inputs of tests/test_gpu_failed_chunks.py: (golden case, failed chunks)
L6 = "l6_c20"
MEM = "memlevel1_c10"
CASES = ((L6, (0,)), (L6, (7,)), (L6, (3, 4)), (MEM, (0, 73, 74, 75, 147)))
ALL_FAIL = (L6, 3, (0, 1, 2))        # a shard of the first three chunks, every one failed
CUT = (L6, 4, 16)                    # a shard of the first four chunks whose compressed range is 16 bytes short


def comp_bounds(oi, first, n):
    """[lo, hi) of the file bytes a shard of chunks [first, first + n) is given (Index[first].Input - 1 ..
    Index[first + n].Input, as LazyFileReader reads them)."""
    return oi.point(first)[1] - 1, oi.point(first + n)[1]


def corrupt_chunk(gz, oi, k, clean=None, skip=()):
    """(the bytes with chunk k corrupted, the oracle's code for chunk k).  clean: the chunks' text before (made
    here when not given); skip: chunks that are corrupt already and are not compared."""
    n = oi.count - 1
    if clean is None:
        clean = [O.extract(gz, oi, j) for j in range(n)]
    i0, i1 = oi.point(k)[1], oi.point(k + 1)[1]
    for q in range(i0 + 8, i1 - 8, 37):
        bad = bytearray(gz)
        for j in range(q, q + 6):
            bad[j] ^= 0x5A
        bad = bytes(bad)
        try:
            O.extract(bad, oi, k)
        except O.OracleError as e:
            for j in range(n):
                if j != k and j not in skip:
                    assert O.extract(bad, oi, j) == clean[j], (k, j)
            return bad, e.code
    raise AssertionError(f"no failing flip inside chunk {k}")


def corrupt_chunks(gz, oi, ks):
    """(the bytes with every chunk of ks corrupted, {k: the oracle's code}); the flips of different chunks
    lie in different byte ranges, so they are found one after the other."""
    clean = [O.extract(gz, oi, j) for j in range(oi.count - 1)]
    codes = {}
    for k in ks:
        prev = gz
        gz, codes[k] = corrupt_chunk(gz, oi, k, clean, tuple(codes))
        assert sum(a != b for a, b in zip(prev, gz)) == 6
    for k, c in codes.items():   # every flip still fails with its code in the company of the others
        try:
            O.extract(gz, oi, k)
            raise AssertionError(k)
        except O.OracleError as e:
            assert e.code == c
    return gz, codes


def mixed_chunks(chunks, failed):
    """The oracle chunks with each failed chunk replaced by an empty chunk."""
    return tuple(EMPTY if k in failed else c for k, c in enumerate(chunks))


@functools.lru_cache(maxsize=None)
def mixed_input(name, failed):
    """(corrupt gz, chunksize, {k: code}, the mixed reference chunks, the clean chunks) of a golden case."""
    gz, cs = R.load_input(name)
    oi = O.build_index(gz, cs)
    bad, codes = corrupt_chunks(gz, oi, failed)
    clean = R.oracle_chunks(name)
    return bad, cs, codes, mixed_chunks(clean, set(failed)), clean


def extract_until(gz, oi, k, end):
    """The oracle's Extract of chunk k from a slice that ends at file byte `end` (exclusive) when the chunk's own
    range reaches further: bytes, or OracleError (zlib was handed only the slice, and needing bytes past it is
    the DATA_ERROR of Core.cs:174)."""
    import ctypes as C
    a = np.frombuffer(gz, np.uint8)
    o0, i0 = oi.point(k)[:2]
    o1, i1 = oi.point(k + 1)[:2]
    lo, n = i0 - 1, min(i1, end) - i0 + 1
    buf = np.zeros(max(1, o1 - o0), np.uint8)
    got = O.L.orc_extract(C.c_void_p(a.ctypes.data + lo), n, C.c_void_p(O.L.orc_index_point(oi.h, k)),
                          C.c_void_p(O.L.orc_index_point(oi.h, k + 1)), C.c_void_p(buf.ctypes.data), buf.size)
    if got < 0:
        raise O.OracleError(got)
    return buf[:got].tobytes()


@functools.lru_cache(maxsize=None)
def cut_input(name=CUT[0], n=CUT[1], short=CUT[2]):
    """(the shard's compressed range cut `short` bytes short, chunksize, {n - 1: code}, the mixed reference chunks
    of chunks [0, n)): the last chunk's status is the oracle's on the same bytes, the chunks before it do not
    reach the cut."""
    gz, cs = R.load_input(name)
    oi = O.build_index(gz, cs)
    lo, hi = comp_bounds(oi, 0, n)
    clean = R.oracle_chunks(name)[:n]
    assert oi.point(n - 1)[1] < hi - short               # the cut lies inside the last chunk's own bytes
    for j in range(n - 1):
        assert extract_until(gz, oi, j, hi - short) == clean[j][1][len(clean[j][0]):]
    try:
        extract_until(gz, oi, n - 1, hi - short)
        raise AssertionError("the short range still decodes")
    except O.OracleError as e:
        code = e.code
    return gz[lo:hi - short], cs, {n - 1: code}, mixed_chunks(clean, {n - 1})


def chunks_text(chunks):
    """The chunks' own text (raw_k without its offset carry), for comparing a shard's output."""
    return [c[1][len(c[0]):] for c in chunks]

