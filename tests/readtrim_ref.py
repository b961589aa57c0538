"""Reference for read trimming (include/ppgpu.h "read trimming"), restated from the semantics with bytes
and Python integers -- a plain loop over the positions of every record -- not from the kernel; plus the
forged input and the trims the read trim tests share.

trim_reference(chunks, t) takes, per chunk k, the oracle's (offset_k, raw_k, descriptors) as
seqpack_ref.oracle_chunks gives them; everything a test expects comes from it:

  S = raw_k[n1+1 : n2], Q = raw_k[n3+1 : n4]; qb(i) = Q[i] for i < len(Q), else 0;
  b0 = min(head, L), e0 = max(b0, L - tail); every cut decided on [b0, e0) on its own;
  b = max(b0, lead), e = min(trail, win, adapt), len = max(e - b, 0), start = b if len else 0."""
import collections
import functools
import random
import zlib

import numpy as np

import seqpack_ref as R
import seqquery_ref as Q
import readfilter_ref as F

LEADING, TRAILING, WINDOW, ADAPTER, AND_MASK = 1, 2, 4, 8, 0x100
CUTS = ("fixed", "leading", "trailing", "window", "adapter")

# the fields of a ppg_read_trim, in order; adapter as bytes (adapter_len is its length)
Trim = collections.namedtuple(
    "Trim", "ops head tail qual_base lead_q trail_q win_size win_q min_overlap max_err_milli min_len adapter")


def struct_of(t, and_mask=False):
    """The _lib.PpgReadTrim of a Trim."""
    import ctypes as C
    from parallelparsing_amd import _lib
    s = _lib.PpgReadTrim(*t[:11], len(t.adapter), (C.c_uint8 * 64)(*t.adapter))
    if and_mask:
        s.ops |= AND_MASK
    return s


# ---- the cuts of one record, each on its own; cached: the settings below share most of them ----
@functools.lru_cache(maxsize=None)
def lead_of(q, b0, e0, thr):
    for i in range(b0, e0):
        if (q[i] if i < len(q) else 0) >= thr:
            return i
    return e0


@functools.lru_cache(maxsize=None)
def trail_of(q, b0, e0, thr):
    for i in range(e0 - 1, b0 - 1, -1):
        if (q[i] if i < len(q) else 0) >= thr:
            return i + 1
    return b0


@functools.lru_cache(maxsize=None)
def win_of(q, b0, e0, W, thr):
    for i in range(b0, e0 - W + 1):
        if sum(q[i + t] if i + t < len(q) else 0 for t in range(W)) < W * thr:
            return i
    return e0


@functools.lru_cache(maxsize=None)
def adapt_of(s, b0, e0, A, min_overlap, max_err_milli):
    m = len(A)
    for p in range(b0, e0):
        ov = min(m, e0 - p)
        if ov < min_overlap:
            continue
        mis = sum(1 for t in range(ov) if s[p + t] != A[t])
        if 1000 * mis <= max_err_milli * ov:
            return p
    return e0


def window_of(t, s, q):
    """(start, len, moved): the window of one record and which of the five cuts moved, each on its own."""
    L = len(s)
    b0 = min(t.head, L)
    e0 = max(b0, L - t.tail)
    lead = lead_of(q, b0, e0, t.qual_base + t.lead_q) if t.ops & LEADING else b0
    trail = trail_of(q, b0, e0, t.qual_base + t.trail_q) if t.ops & TRAILING else e0
    win = win_of(q, b0, e0, t.win_size, t.qual_base + t.win_q) if t.ops & WINDOW else e0
    adapt = adapt_of(s, b0, e0, t.adapter, t.min_overlap, t.max_err_milli) if t.ops & ADAPTER else e0
    b, e = max(b0, lead), min(trail, win, adapt)
    n = max(e - b, 0)
    return (b if n > 0 else 0), n, (b0 > 0 or e0 < L, lead > b0, trail < e0, win < e0, adapt < e0)


def fields(chunks):
    """[(chunk, S, Q)] of every record of all chunks in order."""
    out = []
    for k, (_, raw, desc) in enumerate(chunks):
        raw = bytes(raw)
        for n1, n2, n3, n4 in np.asarray(desc, np.int64).reshape(-1, 4).tolist():
            out.append((k, raw[n1 + 1:n2], raw[n3 + 1:n4]))
    return out


def trim_reference(chunks, t, prior=None):
    """{records, kept, trimmed, cut (int64[5]), bases, bases_window, bases_kept, chunk_kept (int64[n]), rows
    (uint32[records, 2]: start, len), keep (bool per record), mask (uint32 words)}.  prior: uint32 words the
    AND_MASK form starts from (bits of records become old & keep, every other bit stays); without it the
    mask is the keep bits with pad bits 0."""
    recs = fields(chunks)
    rows = np.zeros((len(recs), 2), np.uint32)
    keep = np.zeros(len(recs), bool)
    cut = np.zeros(5, np.int64)
    chunk_kept = np.zeros(len(chunks), np.int64)
    trimmed = bases = bases_window = bases_kept = 0
    for j, (k, s, q) in enumerate(recs):
        start, n, moved = window_of(t, s, q)
        rows[j] = (start, n)
        keep[j] = n >= t.min_len
        cut += np.array(moved, np.int64)
        trimmed += (start, n) != (0, len(s))
        bases += len(s)
        bases_window += n
        if keep[j]:
            bases_kept += n
            chunk_kept[k] += 1
    mask = F.words_of(keep)
    if prior is not None:
        prior = np.asarray(prior, np.uint32)
        mask = prior.copy()
        w = np.full(prior.size, 0xFFFFFFFF, np.uint32)
        w[:F.words_of(keep).size] = F.words_of(keep) | ~F.words_of(np.ones(keep.size, bool))
        mask &= w
    return {"records": len(recs), "kept": int(keep.sum()), "trimmed": int(trimmed), "cut": cut, "bases": bases,
            "bases_window": bases_window, "bases_kept": bases_kept, "chunk_kept": chunk_kept, "rows": rows,
            "keep": keep, "mask": mask}


def slices_of(row, s, q):
    """The trimmed (sequence, quality) of one record: S[start, start+len), Q[start, min(start+len, Lq))."""
    a, n = int(row[0]), int(row[1])
    return s[a:a + n], q[a:min(a + n, len(q))]


# ---- the shared settings ----
QUAL_BASE, CUT_Q, W = 33, 20, 4
TRUSEQ = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"      # the first 33 bases of the TruSeq adapter read through
MIN_OVERLAP, MAX_ERR_MILLI = 5, 100
HEAD, TAIL = 3, 7


def _trim(ops, head=0, tail=0, min_len=36):
    return Trim(ops, head, tail, QUAL_BASE, CUT_Q, CUT_Q, W, CUT_Q, MIN_OVERLAP, MAX_ERR_MILLI, min_len, TRUSEQ)


TRIMS = (_trim(0, min_len=0), _trim(0, HEAD, TAIL), _trim(LEADING), _trim(TRAILING), _trim(WINDOW), _trim(ADAPTER),
         _trim(ADAPTER, HEAD, TAIL), _trim(LEADING | TRAILING | WINDOW | ADAPTER, HEAD, TAIL))
TRIM_IDS = ("none", "fixed", "leading", "trailing", "window", "adapter", "adapter_fixed", "all")
NONE, FIXED, LEAD, TRAIL, WIN, ADAPT, ADAPT_FIXED, ALL = TRIMS

# ---- the forged input ----
FORGED_L = F.FORGED_L
FORGED_CHUNK = 10
FORGED_SEED = 9
HI, MID, LO = QUAL_BASE + 40, QUAL_BASE + 17, QUAL_BASE + 2   # MID: four of them fail a window, three and a HI pass
SEAMS = (30, 31, 32, 2047, 2048, 8191, 8192)                  # last / first good base at these indices
WIN_AT = (28, 29, 31, 32, 2046, 8190)                         # the first failing window starts here
ADAPT_AT = (0, 20, 31, 32, 2040, 8180)                        # a full adapter starts here


def forged_classes():
    """[(L, Lq)]: every L with Lq in {L, L-1, L+40, 0} (below 0: 0)."""
    return [(L, max(lq, 0)) for L in FORGED_L for lq in (L, L - 1, L + 40, 0)]


def _mutate(a, where, to=None):
    """a with the bytes at `where` replaced by another base (or by `to`)."""
    a = bytearray(a)
    for i in where:
        a[i] = to if to is not None else (ord("C") if a[i] != ord("C") else ord("T"))
    return bytes(a)


def planted_records(rng):
    """[(tag, identifier suffix, sequence, quality)]: one record per planted property; the tag names it.
    Sequences around an adapter site are C and T alone, so the adapter (which starts AGATCGGAAG) matches
    only where it is planted; tests/test_readtrim_cpu.py checks every expectation against the reference."""
    bg = lambda n: bytes(rng.choice(b"CT") for _ in range(n))   # noqa: E731
    hi = lambda n: bytes([HI]) * n                               # noqa: E731
    lo = lambda n: bytes([LO]) * n                               # noqa: E731
    out = []

    def add(tag, seq, qual, ident=b""):
        out.append((tag, ident, seq, qual))

    # quality edges
    for x in SEAMS:
        add(("trail", x), bg(x + 40), hi(x + 1) + lo(39))
        add(("lead", x), bg(x + 40), lo(x) + hi(40))
    add(("all_low",), bg(100), lo(100))
    add(("no_low",), bg(100), hi(100))
    # good bytes only past the Quality slice: the line is 60 long and low, what follows it in the text
    # (a newline, '@' and an identifier of '~') is no quality
    add(("past_lq",), bg(100), lo(60))
    add(("after_past_lq",), bg(40), hi(40), ident=b"~" * 80)
    # window
    for x in WIN_AT:
        add(("win", x), bg(x + 40), hi(x) + bytes([MID]) * 4 + hi(36))
    on = bytes([QUAL_BASE + CUT_Q])
    add(("win_on",), bg(50), hi(10) + on * 4 + hi(36))                                   # sum = W * 53: passes
    add(("win_below",), bg(50), hi(10) + on * 3 + bytes([QUAL_BASE + CUT_Q - 1]) + hi(36))  # one less: fails at 10
    add(("win_tail",), bg(50), hi(49) + lo(1))                   # fails only where no full window is left
    add(("win_short",), bg(W - 1), lo(W - 1))                    # e0 - b0 = W - 1
    # adapter
    A = TRUSEQ
    for p in ADAPT_AT:
        add(("adapt", p), bg(p) + A + bg(7), hi(p + 40))
    add(("adapt_3mis",), bg(10) + _mutate(A, (5, 15, 25)) + bg(5), hi(48))              # 3000 <= 3300: matches
    add(("adapt_4mis",), bg(10) + _mutate(A, (5, 15, 25, 30)) + bg(5), hi(48))          # 4000 > 3300
    add(("adapt_ov5",), bg(50) + A[:5], hi(55))
    add(("adapt_ov4",), bg(50) + A[:4], hi(54))
    add(("adapt_ov10_1mis",), bg(50) + _mutate(A[:10], (4,)), hi(60))                   # 1000 <= 1000
    add(("adapt_ov10_2mis",), bg(50) + _mutate(A[:10], (4, 7)), hi(60))                 # 2000 > 1000
    add(("adapt_two",), bg(10) + A + bg(10) + A + bg(3), hi(89))
    add(("adapt_n",), bg(10) + _mutate(A, (2, 12, 22, 32), ord("N")) + bg(5), hi(48))   # a match only if N matched anything
    add(("adapt_before_head",), bg(1) + A + bg(20), hi(54))                             # head = 3: the site is at 1
    add(("adapt_in_tail",), bg(50) + A[:6], hi(56))                                     # tail = 7: the site is past e0
    add(("adapt_cut_by_e0",), bg(50) + A[:6] + bg(TAIL), hi(63))                        # tail = 7: ov(50) = 6, not 13
    return out


@functools.lru_cache(maxsize=None)
def forged_records(seed=FORGED_SEED):
    """[(tag, identifier, sequence, quality)]: the classes shuffled, with the planted records (in their
    order, so that after_past_lq follows past_lq) spread among them."""
    rng = random.Random(seed)
    cls = []
    for L, lq in forged_classes():
        cls.append((("class", L, lq), b"", bytes(rng.choice(F.SEQ_ALPHABET) for _ in range(L)),
                    bytes(rng.choice(F.QUAL_ALPHABET) for _ in range(lq))))
    rng.shuffle(cls)
    planted = planted_records(rng)
    recs, step = [], max(1, len(planted) // len(cls) + 1)
    while cls or planted:
        if cls:
            recs.append(cls.pop())
        for _ in range(step):
            if planted:
                tag = planted[0][0]
                recs.append(planted.pop(0))
                if tag == ("past_lq",):                 # ... and what follows it
                    recs.append(planted.pop(0))
    return tuple((tag, b"r%d%s" % (i, ident), s, q) for i, (tag, ident, s, q) in enumerate(recs))


@functools.lru_cache(maxsize=None)
def forged_text(seed=FORGED_SEED):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (i, s, q) for _, i, s, q in forged_records(seed))


@functools.lru_cache(maxsize=None)
def forged_gz(seed=FORGED_SEED):
    """The forged text as one gzip member at memLevel 1 (as readfilter_ref.forged_gz): a Point, and in
    most chunks an offset carry, every few records."""
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
    return co.compress(forged_text(seed)) + co.flush()


@functools.lru_cache(maxsize=None)
def forged_chunks(seed=FORGED_SEED):
    return Q.chunks_of(forged_gz(seed), FORGED_CHUNK)


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, t):
    """The reference trim of a seqpack_ref input (all chunks); shared and read-only."""
    return _frozen(trim_reference(R.oracle_chunks(name), t))


@functools.lru_cache(maxsize=None)
def forged_reference(t):
    return _frozen(trim_reference(forged_chunks(), t))
