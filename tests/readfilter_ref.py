"""Reference for the read filters (include/ppgpu.h "read filters"), restated from the semantics with
bytes, Python integers and numpy, not from the kernel; plus the forged input and the filters the read
filter tests share.

filter_reference(chunks, flt) takes, per chunk k, the oracle's (offset_k, raw_k, descriptors) as
seqpack_ref.oracle_chunks gives them; everything a test expects comes from it:

  S_j = raw_k[n1+1 : n2], Q_j = raw_k[n3+1 : n4]; L, Lq their lengths; other = the bytes of S_j that are
  none of b"ACGT"; qsum = the sum of the bytes of Q_j; low = the bytes of Q_j below qual_base + low_q;
  the four criteria as integer inequalities; pass = every enabled criterion holds."""
import collections
import functools
import random
import zlib

import numpy as np

import seqpack_ref as R
import seqquery_ref as Q

LENGTH, OTHER, MEAN, LOW, AND_MASK = 1, 2, 4, 8, 0x100
CRITERIA = ("length", "n", "mean_quality", "low_quality")
METRICS_DTYPE = np.dtype([("length", "<u4"), ("other", "<u4"), ("qual_length", "<u4"), ("low", "<u4"),
                          ("qual_sum", "<u8")])

# the fields of a ppg_read_filter, in order
Filter = collections.namedtuple(
    "Filter", "criteria min_len max_len max_other qual_base min_mean_milli low_q max_low_milli")


def measure(chunks, thr):
    """(rows, chunk_of, qual_count): one METRICS_DTYPE row per record of all chunks in order (low counted
    against the byte value thr), the chunk of each record, and the census of the Quality bytes."""
    rows, chunk_of = [], []
    hist = np.zeros(256, np.int64)
    for k, (_, raw, desc) in enumerate(chunks):
        raw = bytes(raw)
        for n1, n2, n3, n4 in np.asarray(desc, np.int64).reshape(-1, 4).tolist():
            s, q = raw[n1 + 1:n2], raw[n3 + 1:n4]
            other = len(s) - sum(s.count(c) for c in b"ACGT")
            rows.append((len(s), other, len(q), sum(c < thr for c in q), sum(q)))
            chunk_of.append(k)
            hist += np.bincount(np.frombuffer(q, np.uint8), minlength=256)
    return np.array(rows, METRICS_DTYPE).reshape(-1), np.array(chunk_of, np.int64), hist


def holds(f, row):
    """The four criteria of filter f on one metrics row, as Python integers: [LENGTH, OTHER, MEAN, LOW]."""
    L, other, Lq, low, qsum = (int(v) for v in row)
    return [f.min_len <= L and (f.max_len < 0 or L <= f.max_len),
            other <= f.max_other,
            1000 * (qsum - f.qual_base * Lq) >= f.min_mean_milli * Lq,
            1000 * low <= f.max_low_milli * Lq]


def words_of(bits):
    """bool per record -> uint32 hit-mask words, pad bits 0."""
    b = np.zeros((bits.size + 31) // 32 * 32, np.uint64)
    b[:bits.size] = bits
    return (b.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def filter_reference(chunks, f, prior=None):
    """{records, passed, failed (int64[4]), bases, other, qual_bytes, qual_count (int64[256]), chunk_passed
    (int64[n]), pass (bool per record), mask (uint32 words), metrics (METRICS_DTYPE rows)}.  prior: uint32
    words the AND_MASK form starts from (bits of records become old & pass, every other bit stays);
    without it the mask is the pass bits with pad bits 0."""
    rows, chunk_of, hist = measure(chunks, f.qual_base + f.low_q)
    enabled = [bool(f.criteria & (1 << c)) for c in range(4)]
    ok = np.ones(rows.size, bool)
    failed = np.zeros(4, np.int64)
    for j, row in enumerate(rows):
        for c, h in enumerate(holds(f, row)):
            if enabled[c] and not h:
                failed[c] += 1
                ok[j] = False
    mask = words_of(ok)
    if prior is not None:
        prior = np.asarray(prior, np.uint32)
        mask = prior.copy()
        keep = np.full(prior.size, 0xFFFFFFFF, np.uint32)
        keep[:words_of(ok).size] = words_of(ok) | ~words_of(np.ones(rows.size, bool))
        mask &= keep
    return {"records": int(rows.size), "passed": int(ok.sum()), "failed": failed,
            "bases": int(rows["length"].sum(dtype=np.int64)), "other": int(rows["other"].sum(dtype=np.int64)),
            "qual_bytes": int(rows["qual_length"].sum(dtype=np.int64)), "qual_count": hist,
            "chunk_passed": np.bincount(chunk_of[ok], minlength=len(chunks)).astype(np.int64),
            "pass": ok, "mask": mask, "metrics": rows}


# ---- the forged input: records at the unit, wave and block boundaries of the kernels' unit map ----
FORGED_L = (0, 1, 31, 32, 33, 63, 64, 65, 150, 2047, 2048, 2049, 8191, 8192, 8193, 12000)
FORGED_CHUNK = 10
FORGED_SEED = 5
SEQ_ALPHABET = b"ACGT" * 30 + b"Nacgtn."                        # ~5.5% of the bytes are not A C G T
QUAL_ALPHABET = bytes(c for c in range(1, 256) if c not in b"\n@")   # no '@' inside a line
QUAL_BASE, LOW_Q = 33, 20


def forged_classes():
    """[(L, Lq)]: every L with Lq in {L, L-1, L+1, L+40, 0} (below 0: 0), and one record with L = 0, Lq = 70."""
    return [(L, max(lq, 0)) for L in FORGED_L for lq in (L, L - 1, L + 1, L + 40, 0)] + [(0, 70)]


# records whose metrics are set by hand, so that every criterion has a record exactly on its threshold
# (it passes) and one a single step beyond (it fails); by (L, Lq), each class occurs once:
#   MEAN   (1, 1) has quality 40 exactly, (0, 1) quality 39;
#   LOW    (0, 40) has 10 of 40 bytes below quality 20 (a quarter), (32, 32) has 9 of 32 (one more than 8);
#   OTHER  (64, 64) holds 3 bytes that are not A C G T, (65, 65) holds 4;
#   LENGTH 32 and 8192 are in FORGED_L, 31 and 8193 beside them.
def _planted(rng, L, lq):
    seq = qual = None
    if (L, lq) == (1, 1):
        qual = bytes([QUAL_BASE + 40])
    elif (L, lq) == (0, 1):
        qual = bytes([QUAL_BASE + 39])
    elif (L, lq) in ((0, 40), (32, 32)):
        nlow = 10 if lq == 40 else 9
        q = [QUAL_BASE + 7] * nlow + [QUAL_BASE + 47] * (lq - nlow)
        rng.shuffle(q)
        qual = bytes(q)
    if (L, lq) in ((64, 64), (65, 65)):
        nother = 3 if L == 64 else 4
        s = [rng.choice(b"ACGT") for _ in range(L - nother)] + [rng.choice(b"Nn.") for _ in range(nother)]
        rng.shuffle(s)
        seq = bytes(s)
    return seq, qual


def forged_records(seed=FORGED_SEED):
    """[(L, Lq, sequence, quality)], shuffled."""
    rng = random.Random(seed)
    recs = []
    for L, lq in forged_classes():
        seq, qual = _planted(rng, L, lq)
        if seq is None:
            seq = bytes(rng.choice(SEQ_ALPHABET) for _ in range(L))
        if qual is None:
            qual = bytes(rng.choice(QUAL_ALPHABET) for _ in range(lq))
        recs.append((L, lq, seq, qual))
    rng.shuffle(recs)
    return recs


@functools.lru_cache(maxsize=None)
def forged_text(seed=FORGED_SEED):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (_, _, s, q) in enumerate(forged_records(seed)))


@functools.lru_cache(maxsize=None)
def forged_gz(seed=FORGED_SEED):
    """The forged text as one gzip member at memLevel 1 (as seqquery_ref.forged_gz)."""
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
    return co.compress(forged_text(seed)) + co.flush()


@functools.lru_cache(maxsize=None)
def forged_chunks(seed=FORGED_SEED):
    return Q.chunks_of(forged_gz(seed), FORGED_CHUNK)


def _base(criteria):
    # thresholds: those the planted records of the forged file sit on (tests/test_readfilter_cpu.py checks it)
    return Filter(criteria, 32, 8192, 3, QUAL_BASE, 40000, LOW_Q, 250)


FILTERS = (_base(0), _base(LENGTH), _base(OTHER), _base(MEAN), _base(LOW), _base(LENGTH | OTHER | MEAN | LOW))
FILTER_IDS = ("none", "length", "n", "mean", "low", "all")
# the golden cases are Illumina-like reads the thresholds above pass or fail wholesale; these split them
# (mean quality 27.5 is the median of memlevel1_c10)
_golden = Filter(0, 40, 150, 0, QUAL_BASE, 27500, LOW_Q, 200)
GOLDEN_FILTERS = tuple(_golden._replace(criteria=c) for c in (LENGTH, OTHER, MEAN, LOW, LENGTH | OTHER | MEAN | LOW))


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, f):
    """The reference filter of a seqpack_ref input (all chunks); shared and read-only."""
    return _frozen(filter_reference(R.oracle_chunks(name), f))


@functools.lru_cache(maxsize=None)
def forged_reference(f):
    return _frozen(filter_reference(forged_chunks(), f))
