"""Reference for the sequence queries (include/ppgpu.h "sequence queries"), restated from the
semantics with bytes and numpy, not from the kernel; plus the forged input the query tests share.

query_reference(chunks, pattern) takes, per chunk k, the oracle's (offset_k, raw_k, descriptors) as
seqpack_ref.oracle_chunks gives them; everything a test expects comes from it:

  S_j = raw_k[n1+1 : n2]; hit_j = pattern in S_j (bytes: ordinal, case sensitive; b"" in S is True);
  counts = np.bincount over all S_j folded into A, C, G, T, other; bases = the sum of len(S_j)."""
import functools
import random
import zlib

import numpy as np

from oracle import oracle as O
import seqpack_ref as R

PATTERNS = (None, b"A", b"ACGT", b"GATTAC", b"T\r")       # the golden cases' patterns

_rng = random.Random(64)
FORGED_PATTERNS = (
    b"A",
    b"GATTACA",
    b"GTTATACACTGC",                                       # Benchmark/Naive.cs RunPattern
    b"ACGTNacgtnACGTNNacgtTGC",                            # 23 bytes, 'N' and lower case
    bytes(_rng.choice(b"ACGT") for _ in range(64)),        # the longest a pattern may be
)
FORGED_CHUNK = 10
FORGED_SEED = 1


def sequences(chunks):
    """Per chunk, the list of Sequence slices (bytes) of its records, in order."""
    out = []
    for _, raw, desc in chunks:
        raw = bytes(raw)
        out.append([raw[int(n1) + 1:int(n2)] for n1, n2, _, _ in np.asarray(desc, np.int64).reshape(-1, 4)])
    return out


def query_reference(chunks, pattern):
    """{records, hits, bases, counts (int64[5]: A C G T other), chunk_hits (int64[n]), hit (bool per
    record), mask (uint32 words, pad bits 0)} over the records of all chunks, in order."""
    pattern = b"" if pattern is None else bytes(pattern)
    seqs = sequences(chunks)
    hit = np.array([pattern in s for ch in seqs for s in ch], bool)
    chunk_hits = np.array([sum(pattern in s for s in ch) for ch in seqs], np.int64)
    allb = np.frombuffer(b"".join(s for ch in seqs for s in ch), np.uint8)
    by = np.bincount(allb, minlength=256).astype(np.int64)
    acgt = [int(by[c]) for c in b"ACGT"]
    counts = np.array(acgt + [int(by.sum()) - sum(acgt)], np.int64)
    bits = np.zeros((hit.size + 31) // 32 * 32, np.uint64)
    bits[:hit.size] = hit
    mask = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return {"records": int(hit.size), "hits": int(hit.sum()), "bases": int(allb.size), "counts": counts,
            "chunk_hits": chunk_hits, "hit": hit, "mask": mask}


@functools.lru_cache(maxsize=None)
def reference(name, pattern):
    """The reference query of a seqpack_ref input (all chunks); shared and read-only."""
    ref = query_reference(R.oracle_chunks(name), pattern)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- the forged input: planted matches where the unit mapping of the kernel can go wrong ----
def forged_records(pattern, seed=FORGED_SEED):
    """[(tag, identifier, sequence, plus, quality)] for one pattern of length m.  Background bases
    avoid the pattern's last byte, so a sequence holds the pattern only where it is planted.
      plain     no pattern (every L of the list, also those below m)
      start     planted at 0            end   planted at L - m
      straddle  planted at p with (p mod 32) + m > 32: the match crosses a 32-base unit boundary
      nearmiss  the sequence ends with pattern[:m-1]
      decoy     identifier, '+' line and quality contain the pattern, the sequence does not"""
    m = len(pattern)
    rng = random.Random(seed * 1000 + m)
    alpha = bytes(c for c in b"ACGT" if c != pattern[-1])
    bg = lambda n: bytes(rng.choice(alpha) for _ in range(n))   # noqa: E731
    recs = []

    def add(tag, seq, plus=b"", qual=None, ident=b""):
        recs.append((tag, b"f%d%s" % (len(recs), ident), seq, plus, b"I" * len(seq) if qual is None else qual))

    def plant(L, p):
        return bg(p) + pattern + bg(L - p - m)

    for L in sorted({0, 1, m - 1, m, m + 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150, 300}):
        add("plain", bg(L))
        if L < m:
            continue
        add("start", plant(L, 0))
        add("end", plant(L, L - m))
        cross = [p for p in range(L - m + 1) if p % 32 + m > 32]
        for p in cross[::max(1, len(cross) // m)][:m]:
            add("straddle", plant(L, p))
        add("nearmiss", bg(L - (m - 1)) + pattern[:m - 1])
        add("decoy", bg(L), plus=pattern, qual=pattern + b"I" * (L - m), ident=b" " + pattern)
    rng.shuffle(recs)
    return recs


def forged_text(pattern, seed=FORGED_SEED):
    return b"".join(b"@%s\n%s\n+%s\n%s\n" % (i, s, p, q) for _, i, s, p, q in forged_records(pattern, seed))


@functools.lru_cache(maxsize=None)
def forged_gz(pattern, seed=FORGED_SEED):
    """The forged text as one gzip member, memLevel 1 (a deflate block every ~100 symbols, so the
    index has a Point, and most chunks an offset carry, every few records)."""
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
    return co.compress(forged_text(pattern, seed)) + co.flush()


def chunks_of(gz, chunksize):
    """Per chunk of any input, from the oracle: (offset_k, raw_k, descriptors (n, 4))."""
    oi = O.build_index(gz, chunksize)
    out = []
    for k in range(oi.count - 1):
        off = oi.point(k)[4]
        ch = O.extract(gz, oi, k)
        out.append((off, off + ch, np.asarray(O.parse(off, ch), np.uint32).reshape(-1, 4)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def forged_chunks(pattern, seed=FORGED_SEED):
    return chunks_of(forged_gz(pattern, seed), FORGED_CHUNK)
