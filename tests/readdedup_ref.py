"""Reference for the read dedup (include/ppgpu.h "read dedup"), restated from the header's text with bytes and
Python integers -- a plain loop over the records, a dict for the table -- not from the kernel; plus the forged
input the read dedup tests share.

dedup_reference(chunks, d, keep, rows) takes, per chunk k, the oracle's (offset_k, raw_k, descriptors) as
seqpack_ref.oracle_chunks gives them (every chunk decoded); everything a test expects comes from it:

  S = raw_k[n1+1 : n2]; the window (s, w) = (0, L), or row j clamped: s = min(start, L), w = min(len, L - s);
  Ld = w, or min(w, max_bases) when max_bases > 0; D = S[s : s + Ld]; a record participates when its bit of
  `keep` is set (all without one);
  unit i = D[32 i : 32 i + 32] zero-padded, as four little-endian uint64 w_0 .. w_3;
  mix(x): x ^= x >> 32; x *= 0xD6E8FEB86659FD93; x ^= x >> 32; x *= 0xD6E8FEB86659FD93; x ^= x >> 32 (mod 2^64);
  h_i: a = mix(0x9E3779B97F4A7C15 * (i + 1)); a = mix(a ^ w_t) for t = 0 .. 3;
  G = sum of h_i over i < ceil(Ld / 32); F = mix(G ^ mix(Ld + 0x632BE59BD9B4E019)), 0 becomes 1;
  records are duplicates of each other iff F is equal; the table has one row (F, lowest record number, count)
  per distinct F; home slot = (F * 0x9E3779B97F4A7C15) >> (64 - log2 slots)."""
import collections
import functools
import random
import zlib

import numpy as np

import seqpack_ref as R
import seqquery_ref as Q
import readfilter_ref as F
import readtrim_ref as T

USE_WINDOWS, AND_MASK = 2, 0x100
M64 = (1 << 64) - 1
MUL, GOLD, LEN = 0xD6E8FEB86659FD93, 0x9E3779B97F4A7C15, 0x632BE59BD9B4E019
TOTALS = ("records", "participating", "unique", "bases", "bases_unique", "overflow", "max_count", "max_first")
LEVEL_LO = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)     # the least count of each bin
MAX_BASES = (0, 1, 32, 33, 50)

# the fields of a ppg_read_dedup, in order (reserved[2] as two fields)
Dedup = collections.namedtuple("Dedup", "flags max_bases reserved0 reserved1")


def dedup(max_bases=0, flags=0):
    return Dedup(flags, max_bases, 0, 0)


def struct_of(d, and_mask=False, windows=False):
    """The _lib.PpgReadDedup of a Dedup, with the flags of the buffers it is called with."""
    import ctypes as C
    from parallelparsing_amd import _lib
    return _lib.PpgReadDedup(d.flags | (AND_MASK if and_mask else 0) | (USE_WINDOWS if windows else 0), d.max_bases,
                             (C.c_int64 * 2)(d.reserved0, d.reserved1))


# ---- the fingerprint ----
def mix(x):
    x ^= x >> 32
    x = x * MUL & M64
    x ^= x >> 32
    x = x * MUL & M64
    return x ^ x >> 32


@functools.lru_cache(maxsize=None)
def fingerprint(D):
    """F of the key bytes D."""
    G = 0
    for i in range((len(D) + 31) // 32):
        unit = D[32 * i:32 * i + 32].ljust(32, b"\0")
        a = mix(GOLD * (i + 1) & M64)
        for t in range(4):
            a = mix(a ^ int.from_bytes(unit[8 * t:8 * t + 8], "little"))
        G = G + a & M64
    return mix(G ^ mix(len(D) + LEN & M64)) or 1


def home_slot(Fv, slots):
    assert slots >= 64 and slots & (slots - 1) == 0
    return (Fv * GOLD & M64) >> (64 - (slots.bit_length() - 1))


def min_slots(records):
    """The smallest legal table of a run of `records` records."""
    return max(64, 1 << max(2 * records - 1, 0).bit_length())


def level_of(count):
    return max(b for b, lo in enumerate(LEVEL_LO) if count >= lo)


def key_bytes(S, d, row=None):
    s, w = 0, len(S)
    if row is not None:
        s = min(int(row[0]), len(S))
        w = min(int(row[1]), len(S) - s)
    Ld = min(w, d.max_bases) if d.max_bases > 0 else w
    return S[s:s + Ld]


def dedup_reference(chunks, d, keep=None, rows=None, prior=None):
    """{the TOTALS, level_distinct, level_reads (int64[16]), chunk_unique (int64[n]), unique (bool per record),
    first (int64 per record, -1: does not participate), mask (uint32 words), table (uint64[rows, 3]: key, first,
    count, sorted), keys (the key bytes of every record), F (uint64 per record)}.  keep: bool per record or
    None; rows: uint32[records, 2] or None; prior: uint32 words the AND_MASK form starts from (bits of records
    become old & unique, every other bit stays); without it the mask is the unique bits with pad bits 0."""
    recs = T.fields(chunks)
    n = len(recs)
    keys = [key_bytes(S, d, None if rows is None else rows[j]) for j, (_, S, _) in enumerate(recs)]
    Fs = np.array([fingerprint(D) for D in keys], np.uint64)
    table = {}                                         # F -> [first, count]
    first = np.full(n, -1, np.int64)
    part = np.ones(n, bool) if keep is None else np.asarray(keep, bool)[:n].copy()
    for j in np.flatnonzero(part).tolist():
        row = table.setdefault(int(Fs[j]), [j, 0])
        row[1] += 1
    for j in np.flatnonzero(part).tolist():
        first[j] = table[int(Fs[j])][0]
    unique = part & (first == np.arange(n))
    chunk_of = np.array([k for k, _, _ in recs], np.int64)
    Ld = np.array([len(D) for D in keys], np.int64)
    level_distinct, level_reads = np.zeros(16, np.int64), np.zeros(16, np.int64)
    for _, c in table.values():
        level_distinct[level_of(c)] += 1
        level_reads[level_of(c)] += c
    top = min(table.values(), key=lambda r: (-r[1], r[0])) if table else (-1, 0)
    mask = F.words_of(unique)
    if prior is not None:
        prior = np.asarray(prior, np.uint32)
        mask = prior.copy()
        w = np.full(prior.size, 0xFFFFFFFF, np.uint32)
        w[:F.words_of(unique).size] = F.words_of(unique) | ~F.words_of(np.ones(n, bool))
        mask &= w
    rows_sorted = np.array(sorted((k, f, c) for k, (f, c) in table.items()), np.uint64).reshape(-1, 3)
    return {"records": n, "participating": int(part.sum()), "unique": int(unique.sum()),
            "bases": int(Ld[part].sum()), "bases_unique": int(Ld[unique].sum()), "overflow": 0,
            "max_count": int(top[1]), "max_first": int(top[0]), "level_distinct": level_distinct,
            "level_reads": level_reads, "chunk_unique": np.bincount(chunk_of[unique], minlength=len(chunks)).astype(np.int64),
            "unique_bits": unique, "first": first, "mask": mask, "table": rows_sorted, "keys": keys, "F": Fs}


def top_of(ref, k):
    """[(count, first)] of the k greatest rows of a reference's table, ties to the lower first."""
    rows = sorted(((int(c), int(f)) for _, f, c in ref["table"]), key=lambda r: (-r[0], r[1]))
    return rows[:k]


def sorted_rows(table):
    """The non-empty rows of a device table (int64 or uint64 [slots, 3]) sorted as the reference's, and whether
    every other row is exactly empty (0, all ones, 0)."""
    t = np.ascontiguousarray(table).view(np.uint64).reshape(-1, 3)
    full = t[:, 0] != 0
    empty_ok = bool((t[~full] == np.array([0, M64, 0], np.uint64)).all())
    rows = t[full]
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))], empty_ok


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, d):
    """The reference dedup of a seqpack_ref input (all chunks, no mask, no windows); shared and read-only."""
    return _frozen(dedup_reference(R.oracle_chunks(name), d))


def content_rows(chunks, seed=3):
    """uint32[records, 2]: a window per record that depends on the record's Sequence alone (copies keep equal
    windows, so they stay duplicates): honest windows whose start is often no multiple of 4, and hostile ones
    (start past the read, len past its end, both huge) for the clamp."""
    recs = T.fields(chunks)
    rows = np.zeros((len(recs), 2), np.uint32)
    for j, (_, S, _) in enumerate(recs):
        L, h = len(S), zlib.crc32(S, seed)
        kind, a, b = h % 6, (h >> 8) % (L + 1), (h >> 20) % 97
        if kind == 0:
            rows[j] = (L + 1 + b, b)                     # start > L
        elif kind == 1:
            rows[j] = (a, L + 1 + b)                     # len past the end
        elif kind == 2:
            rows[j] = (0xFFFFFFFF, 0xFFFFFFFF)
        elif kind == 3:
            rows[j] = (a, 0xFFFFFFFF)
        else:
            rows[j] = (a, (h >> 12) % (L - a + 1))
    return rows


# ---- the forged input ----
FORGED_CHUNK = 10
FORGED_SEED = 21
COPIES = tuple(range(1, 12)) + (49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000)
HOT = b"A"                                     # the 10,000 copies: 1-base reads, the hot key
LENGTHS = (0, 1, 31, 32, 33, 64, 65, 2100)     # each as a single and as a pair of copies
SINGLES = 1500                                 # distinct short reads that fill the table's home slots
WINDOW_CORE = b"GATTACAGATTACAGATTACA"
WINDOW_ROWS = ((3, len(WINDOW_CORE)), (5, len(WINDOW_CORE)))
# Three reads whose fingerprints have the table's last row as their home slot at the smallest legal table of this
# input (131,072 rows): found by search over random 24-base reads; tests/test_readdedup_cpu.py checks it.
LAST_ROW = (b"TGCGTAGCAGCGCAGCGAGTGTCT", b"ACTTAACATTTTTAACCTGAGCTC", b"CGACAGTGTGCCCGTGTCTGTGCC")


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def planted_pairs(rng):
    """[(tag, a, b)]: two reads that differ in exactly the way the tag names."""
    x40, y40, z40, x64, y64, x60 = (_seq(rng, n) for n in (40, 40, 40, 64, 64, 60))
    flip = lambda s, i: s[:i] + (b"C" if s[i:i + 1] != b"C" else b"T") + s[i + 1:]   # noqa: E731
    return [("last_byte", x40, flip(x40, 39)),
            ("second_unit", x64, flip(x64, 45)),
            ("prefix", y40, y40[:39]),
            ("pad_alike", z40[:32], z40[:32] + b"\x01"),
            ("units_swapped", y64, y64[32:] + y64[:32]),
            ("first_50", x60, x60[:50] + flip(x60, 55)[50:]),
            ("window_only", b"GGG" + WINDOW_CORE + b"T", b"CCCCC" + WINDOW_CORE + b"AA")]


@functools.lru_cache(maxsize=None)
def forged_records(seed=FORGED_SEED):
    """[(tag, sequence)] in file order: the copy classes shuffled among the singles, with adjacent copies, the
    lengths, the planted pairs and the last-row reads spread among them."""
    rng = random.Random(seed)
    recs, seen = [], {HOT}

    def fresh(n):
        while True:
            s = _seq(rng, n)
            if s not in seen:
                seen.add(s)
                return s

    for c in COPIES:
        s = HOT if c == 10000 else fresh(rng.randrange(12, 25))
        recs += [(("copies", c), s)] * c
    recs += [(("single",), fresh(rng.randrange(8, 30))) for _ in range(SINGLES)]
    for L in LENGTHS:
        recs.append((("length", L, 1), fresh(L) if L > 1 else (b"" if L == 0 else b"N")))
        recs += [(("length", L, 2), b"" if L == 0 else (b"C" if L == 1 else fresh(L)))] * 2
    for tag, a, b in planted_pairs(rng):
        recs += [(("pair", tag, 0), a), (("pair", tag, 1), b)]
    recs += [(("last_row", i), s) for i, s in enumerate(LAST_ROW)]
    rng.shuffle(recs)
    # copies next to each other, which a shuffle of mostly hot reads makes only of the hot key
    adj = fresh(20)
    at = len(recs) // 3
    recs[at:at] = [(("adjacent",), adj)] * 3
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def forged_text(seed=FORGED_SEED):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, (_, s) in enumerate(forged_records(seed)))


@functools.lru_cache(maxsize=None)
def forged_gz(seed=FORGED_SEED):
    """The forged text as one gzip member at memLevel 1 (as readfilter_ref.forged_gz): a Point, and in most
    chunks an offset carry, every few records."""
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
    return co.compress(forged_text(seed)) + co.flush()


@functools.lru_cache(maxsize=None)
def forged_chunks(seed=FORGED_SEED):
    return Q.chunks_of(forged_gz(seed), FORGED_CHUNK)


@functools.lru_cache(maxsize=None)
def forged_random_mask(extra_words=2, seed=13):
    """uint32 words, two more than the forged file's records need: three bits in four set at random."""
    n = len(forged_records())
    rng = np.random.default_rng(seed)
    a, b = (rng.integers(0, 1 << 32, (n + 31) // 32 + extra_words, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    w = a | b
    w.setflags(write=False)
    return w


def bits_of(words, n):
    """bool per record of the first n bits of hit-mask words."""
    w = np.asarray(words, np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:n].astype(bool)


@functools.lru_cache(maxsize=None)
def forged_rows():
    """content_rows of the forged file, with the window_only pair's rows set so that only their windows agree."""
    rows = content_rows(forged_chunks())
    for j, (tag, _) in enumerate(forged_records()):
        if tag[:2] == ("pair", "window_only"):
            rows[j] = WINDOW_ROWS[tag[2]]
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def forged_reference(d, which="plain"):
    """The forged file's reference under one of the test's input combinations: plain, mask (the random mask
    decides participation), rows (the windows), mask_rows (both)."""
    chunks = forged_chunks()
    n = len(forged_records())
    keep = bits_of(forged_random_mask(), n) if which in ("mask", "mask_rows") else None
    rows = forged_rows() if which in ("rows", "mask_rows") else None
    prior = forged_random_mask() if keep is not None else None
    return _frozen(dedup_reference(chunks, d, keep, rows, prior))
