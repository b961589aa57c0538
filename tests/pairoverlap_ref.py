"""Reference for the pair overlap (include/ppgpu.h "pair overlap"), restated in plain Python from that
section's text, not from the kernel and not from any tool; plus the forge of read pairs the overlap tests
share.  Reads are byte strings; a base is one of ACGT, anything else is an N (its 2-bit code 0, its mask
bit 1, as the packed reads have it).

overlap_one does one pair by brute force over every d in the stated order; overlap_reference applies the
maps, the rows' format, the found mask, the windows rule, the totals and the histogram."""
import collections
import functools

import numpy as np

MAX_LEN, HIST = 1024, 2048
TOTALS = ("pairs", "unmapped", "too_long", "analysed", "found", "negative", "adapter", "overlap_bases", "mismatches")

# the fields of a ppg_pair_overlap that are not 0
Params = collections.namedtuple("Params", "min_overlap max_diff max_err_milli")
DEFAULTS = Params(30, 5, 200)                 # fastp's
EXACT = Params(1, 0, 200)                     # any overlap, no mismatch
ALWAYS = Params(30, 1000, 1000)               # the first candidate of 30 bases is accepted
RATE = Params(30, 5, 100)                     # the milli rate binds before max_diff (3 of 30): see "rate" below
PARAM_SETS = {"defaults": DEFAULTS, "exact": EXACT, "always": ALWAYS, "rate": RATE}

_CODE = np.zeros(256, np.int8)
_ISN = np.ones(256, bool)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c], _ISN[_c] = _i, False
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def struct_of(p):
    from parallelparsing_amd import _lib
    import ctypes as C
    return _lib.PpgPairOverlap(0, p.min_overlap, p.max_diff, p.max_err_milli, (C.c_int64 * 4)())


def revcomp(s):
    """The reverse complement as text (an N stays an N)."""
    return bytes(s).translate(_COMP)[::-1]


def codes(s):
    """(c, n): the 2-bit codes and the mask bits of a read."""
    b = np.frombuffer(bytes(s), np.uint8)
    return _CODE[b].astype(np.int64), _ISN[b]


def candidates(L1, L2):
    """Every d with -L2 < d < L1 in the order of the semantics."""
    return [d for d in list(range(0, L1)) + [-k for k in range(1, L2)] if -L2 < d < L1]


def mis_at(s1, s2, d):
    """(ov(d), mis(d)) of a pair, position by position."""
    c1, n1 = codes(s1)
    c2, n2 = codes(s2)
    L1, L2 = len(s1), len(s2)
    ov = mis = 0
    for i in range(max(0, d), min(L1, L2 + d)):
        t = i - d
        cR, nR = 3 - c2[L2 - 1 - t], n2[L2 - 1 - t]
        ov += 1
        mis += bool(n1[i] or nR or c1[i] != cR)
    return ov, mis


def accepted(ov, mis, p):
    return ov >= p.min_overlap and mis <= p.max_diff and 1000 * mis <= p.max_err_milli * ov


@functools.lru_cache(maxsize=None)
def overlap_one(s1, s2, p):
    """"long" for a long pair, None for a pair that is not found, else (d, ov, mis, I)."""
    L1, L2 = len(s1), len(s2)
    if L1 > MAX_LEN or L2 > MAX_LEN:
        return "long"
    c1, n1 = codes(s1)
    c2, n2 = codes(s2)
    cR, nR = 3 - c2[::-1], n2[::-1]
    for d in candidates(L1, L2):
        lo, hi = max(0, d), min(L1, L2 + d)
        ov = hi - lo
        if ov < p.min_overlap:
            continue
        bad = n1[lo:hi] | nR[lo - d:hi - d] | (c1[lo:hi] != cR[lo - d:hi - d])
        mis = int(np.count_nonzero(bad))
        if accepted(ov, mis, p):
            return d, ov, mis, L2 + d
    return None


def clip_row(row, L, I):
    """The windows rule: a row (s, n) of a read of length L, clipped to the insert size I."""
    s = min(int(row[0]), L)
    n = min(int(row[1]), L - s)
    e = min(s + n, I)
    return (s, e - s) if e > s else (0, 0)


def overlap_reference(set1, set2, p, rec1=None, rec2=None, npairs=None, windows1=None, windows2=None):
    """{the TOTALS, clipped (2), rows int32[npairs, 4], found_bits bool[npairs], mask uint32 words, hist int64[HIST],
    windows1 / windows2 (uint32[records, 2] after the call, or None)}.  set1 / set2: lists of reads by record
    number; rec1 / rec2: int64 per pair or None (identity)."""
    if npairs is None:
        npairs = len(rec1) if rec1 is not None else len(rec2) if rec2 is not None else min(len(set1), len(set2))
    rows = np.zeros((npairs, 4), np.int32)
    found = np.zeros(npairs, bool)
    hist = np.zeros(HIST, np.int64)
    tot = dict.fromkeys(TOTALS, 0)
    clipped = [0, 0]
    w = [None if x is None else np.array(x, np.uint32).reshape(-1, 2) for x in (windows1, windows2)]
    for i in range(npairs):
        r1 = int(rec1[i]) if rec1 is not None else i
        r2 = int(rec2[i]) if rec2 is not None else i
        tot["pairs"] += 1
        if not (0 <= r1 < len(set1) and 0 <= r2 < len(set2)):
            tot["unmapped"] += 1
            continue
        s1, s2 = set1[r1], set2[r2]
        res = overlap_one(s1, s2, p)
        if res == "long":
            tot["too_long"] += 1
            continue
        tot["analysed"] += 1
        if res is None:
            continue
        d, ov, mis, I = res
        rows[i] = res
        found[i] = True
        hist[I] += 1
        tot["found"] += 1
        tot["negative"] += d < 0
        tot["adapter"] += I < len(s1) or I < len(s2)
        tot["overlap_bases"] += ov
        tot["mismatches"] += mis
        for m, (r, s) in enumerate(((r1, s1), (r2, s2))):
            clipped[m] += max(len(s) - I, 0)
            if w[m] is not None:
                w[m][r] = clip_row(w[m][r], len(s), I)
    return dict(tot, clipped=tuple(clipped), rows=rows, found_bits=found, mask=mask_words(found), hist=hist,
                windows1=w[0], windows2=w[1])


def mask_words(bits):
    """The hit-mask words of a bool array: bit j & 31 of word j >> 5, pad bits 0."""
    b = np.zeros((len(bits) + 31) // 32 * 32, np.uint64)
    b[:len(bits)] = bits
    return (b.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def whole_rows(reads):
    """The rows of a caller without a trim: (0, seq_len)."""
    return np.array([(0, len(s)) for s in reads], np.uint32).reshape(-1, 2)


def pack_strings(reads):
    """{seq_off, seq_len, bases, mask} of the packed reads format for a list of reads, from the format's text."""
    L = np.array([len(s) for s in reads], np.int64)
    seq_off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum((L + 31) // 32 * 32, out=seq_off[1:])
    T = int(seq_off[-1])
    code, mbit = np.zeros(T, np.uint64), np.zeros(T, np.uint64)
    for j, s in enumerate(reads):
        c, n = codes(s)
        b = int(seq_off[j])
        code[b:b + len(s)] = c
        mbit[b:b + len(s)] = n
    bases = (code.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    mask = (mbit.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return {"seq_off": seq_off, "seq_len": L.astype(np.uint32), "bases": bases, "mask": mask}


# ---- the forge ----
# Every pair carries the category it was made for; tests/test_pairoverlap_cpu.py checks that each category is
# what it claims under the reference.
Pair = collections.namedtuple("Pair", "r1 r2 cat note")
ADAPTER1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
FRAG_LENGTHS = (31, 32, 33, 63, 64, 65, 150)
UNEQUAL = ((150, 100), (40, 150), (1024, 1024), (1025, 150), (0, 150), (150, 0), (1, 1))


def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


def mates(frag, L1, L2, rng):
    """The two reads of a fragment: its first L1 bases and the first L2 of its reverse complement, the
    read-through of a short fragment filled with the adapters and then random bases."""
    fill = _rand(rng, L1 + L2)
    return (frag + ADAPTER1 + fill)[:L1], (revcomp(frag) + ADAPTER2 + fill[::-1])[:L2]


def substitute(s, positions, to=None):
    """s with the bases at `positions` replaced: by `to`, or by the next of ACGT (always another base)."""
    b = bytearray(s)
    for i in positions:
        b[i] = to if to is not None else b"CGTA"[b"ACGT".index(bytes([b[i]]))]
    return bytes(b)


@functools.lru_cache(maxsize=None)
def forge():
    """The list of Pairs, about 3,000, the same on every call."""
    rng = np.random.default_rng(20260421)
    out = []
    # fragment shapes: every fragment length around, below and above the read length
    for L in FRAG_LENGTHS:
        for F in range(1, 2 * L + 6):
            out.append(Pair(*mates(_rand(rng, F), L, L, rng), "frag", (L, F)))
    for L1, L2 in UNEQUAL:
        if max(L1, L2) > 1000:
            lens = (min(L1, L2) // 2 + 1, 1100, 1500, 2030)
        else:
            lens = sorted(set(list(range(1, L1 + L2 + 6, 7)) + [L1, L2, L1 + L2 - 30, L1 + L2 - 29]))
        for F in lens:
            if F >= 1:
                out.append(Pair(*mates(_rand(rng, F), L1, L2, rng), "unequal", (L1, L2, F)))
    # mismatch boundaries: 100 / 100 reads of a 130-base fragment, d = 30 and ov = 70; read-1 position i
    # faces R position i - 30, which is read-2 position 99 - (i - 30)
    L, F, d = 100, 130, 30
    spots = {"first": 30, "last": 99, "w1lo": 31, "w1hi": 32, "w1lo2": 63, "w1hi2": 64, "wRlo": 30 + 31, "wRhi": 30 + 32,
             "wRlo2": 30 + 63, "wRhi2": 30 + 64}
    for name, at in spots.items():
        for nmis in (DEFAULTS.max_diff, DEFAULTS.max_diff + 1):
            for side in (1, 2):
                r1, r2 = mates(_rand(rng, F), L, L, rng)
                others = [p for p in (40, 50, 55, 70, 75, 85, 90) if p != at][:nmis - 1]
                pos = [at] + others
                if side == 1:
                    r1 = substitute(r1, pos)
                else:
                    r2 = substitute(r2, [L - 1 - (i - d) for i in pos])
                out.append(Pair(r1, r2, "boundary", (name, nmis, side)))
    # N on either mate: inside the overlap it is one more mismatch, just outside it changes nothing
    for where in ("in", "out"):
        for side in (1, 2):
            for nmis in (DEFAULTS.max_diff - 1, DEFAULTS.max_diff):
                r1, r2 = mates(_rand(rng, F), L, L, rng)
                r1 = substitute(r1, [41, 52, 63, 74, 85, 96][:nmis])
                if side == 1:
                    r1 = substitute(r1, [d if where == "in" else d - 1], ord("N"))
                else:   # R position 69 is the overlap's last, read-2 position 30; read-2 position 29 is outside
                    r2 = substitute(r2, [30 if where == "in" else 29], ord("N"))
                out.append(Pair(r1, r2, "n_" + where, (side, nmis)))
    # the two limits at ov = min_overlap - 1, min_overlap, min_overlap + 1: 100 / 100 reads, F = 200 - ov
    for ov in (29, 30, 31):
        for nmis in (3, 4, 5, 6):
            r1, r2 = mates(_rand(rng, 2 * L - ov), L, L, rng)
            r1 = substitute(r1, [L - 1 - 4 * k for k in range(nmis)])
            out.append(Pair(r1, r2, "limits", (ov, nmis)))
    # several accepted d: the order decides
    unit = b"ACGTTGCA"
    for r1, r2 in ((unit * 12, revcomp(unit * 12)), (unit * 12 + b"AC", revcomp(unit * 9)), (b"A" * 100, b"T" * 100),
                   (b"G" * 80, b"C" * 120), (b"A" * 64, b"T" * 33), (unit * 4, revcomp(unit * 16)),
                   (b"AC" * 75, revcomp(b"AC" * 75)), (b"N" * 50, b"N" * 50)):
        out.append(Pair(r1, r2, "repeat", None))
    # unrelated reads
    for _ in range(200):
        out.append(Pair(_rand(rng, 150), _rand(rng, 150), "random", None))
    # fragments of 150 / 150 reads with sequencing errors and an occasional N
    for k in range(1600):
        F = int(rng.integers(20, 330))
        r1, r2 = mates(_rand(rng, F), 150, 150, rng)
        r1 = substitute(r1, sorted(set(rng.integers(0, 150, size=int(rng.integers(0, 6))).tolist())))
        r2 = substitute(r2, sorted(set(rng.integers(0, 150, size=int(rng.integers(0, 6))).tolist())))
        if k % 9 == 0:
            r1 = substitute(r1, [int(rng.integers(0, 150))], ord("N"))
        out.append(Pair(r1, r2, "noisy", F))
    return tuple(out)


def forge_sets(which="identity"):
    """(set1, set2, rec1, rec2) of the forge under a map: "identity" (no maps), "permutation" (set 2 stored in
    a shuffled order, set 1 reversed) or "holes" (the permutation with entries of -1, the set's size and 2^40,
    which leave their pairs out, and fewer pairs than records)."""
    pairs = forge()
    n = len(pairs)
    r1s, r2s = [p.r1 for p in pairs], [p.r2 for p in pairs]
    if which == "identity":
        return r1s, r2s, None, None
    rng = np.random.default_rng(7)
    rec1 = np.arange(n - 1, -1, -1, dtype=np.int64)
    rec2 = rng.permutation(n).astype(np.int64)
    set1, set2 = [None] * n, [None] * n
    for i in range(n):
        set1[rec1[i]], set2[rec2[i]] = r1s[i], r2s[i]
    if which == "holes":
        rec1, rec2 = rec1[:n - 37].copy(), rec2[:n - 37].copy()
        rec1[3::41] = -1
        rec2[5::43] = n
        rec1[7::97] = 1 << 40
        rec2[11::101] = -(1 << 40)
    return set1, set2, rec1, rec2


@functools.lru_cache(maxsize=None)
def forge_reference(pname, which="identity", windows=True):
    """overlap_reference of the forge under a parameter set and a map, from whole-read rows; shared, read-only."""
    set1, set2, rec1, rec2 = forge_sets(which)
    ref = overlap_reference(set1, set2, PARAM_SETS[pname], rec1, rec2, windows1=whole_rows(set1) if windows else None,
                            windows2=whole_rows(set2) if windows else None)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
