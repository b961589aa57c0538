"""Reference for the k-mer counts (include/ppgpu.h "k-mer counts"), restated in numpy from that section's text, not
from the kernel and not from any tool; plus the forge of reads the k-mer tests share.  Reads are byte strings; a
base is one of ACGT, anything else breaks a k-mer (its mask bit is set, as the packed reads have it).

read_keys gives one read's positions and valid keys; reference applies the mask, the windows rule, counts by
np.unique, and makes the totals, the spectrum and max_key."""
import collections
import functools

import numpy as np

from pairoverlap_ref import codes, mask_words, pack_strings, revcomp  # noqa: F401  (pack_strings: the tests pack through it)

SPECTRUM = 1024
KS = (1, 2, 15, 16, 17, 21, 31)
CALL_TOTALS = ("records", "participating", "short_reads", "bases", "positions", "kmers", "invalid")
TABLE_TOTALS = ("distinct", "singletons", "max_count", "max_key", "total_count")
TOTALS = CALL_TOTALS + TABLE_TOTALS
CANONICAL, USE_WINDOWS, USE_MASK, ACCUMULATE = 1, 2, 4, 8


def struct_of(k, flags):
    from parallelparsing_amd import _lib
    import ctypes as C
    return _lib.PpgKmerCount(flags, k, (C.c_int64 * 6)())


def window(row, L):
    """The windows rule: a row (start, len) of a read of length L clamped to (s, w)."""
    s = min(int(row[0]), L)
    return s, min(int(row[1]), L - s)


def read_keys(read, k, canonical, s=0, w=None):
    """(positions, keys): the number of positions of the window (s, w) of a read and the keys (uint64) of the valid
    ones, in read order."""
    L = len(read)
    w = L - s if w is None else w
    npos = max(w - k + 1, 0)
    if npos == 0:
        return 0, np.zeros(0, np.uint64)
    c, n = codes(read[s:s + w])
    cw = np.lib.stride_tricks.sliding_window_view(c.astype(np.uint64), k)
    ok = ~np.lib.stride_tricks.sliding_window_view(n, k).any(axis=1)
    wt = np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64)        # the first base is most significant
    fwd = (cw * wt).sum(axis=1, dtype=np.uint64)
    if canonical:
        rc = ((np.uint64(3) - cw[:, ::-1]) * wt).sum(axis=1, dtype=np.uint64)
        fwd = np.minimum(fwd, rc)
    return npos, fwd[ok]


def tally(keys):
    """(sorted distinct keys, their counts) of an array of keys."""
    if len(keys) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    u, c = np.unique(np.asarray(keys, np.uint64), return_counts=True)
    return u, c.astype(np.int64)


def merge_tallies(a, b):
    """The tally of two tallies' union."""
    keys = np.concatenate([a[0], b[0]])
    u, inv = np.unique(keys, return_inverse=True)
    c = np.zeros(len(u), np.int64)
    np.add.at(c, inv, np.concatenate([a[1], b[1]]))
    return u, c


def table_totals(keys, counts):
    """The totals "of the table" and the spectrum of a tally."""
    spec = np.bincount(np.minimum(counts, SPECTRUM - 1), minlength=SPECTRUM).astype(np.int64) if len(counts) else np.zeros(SPECTRUM, np.int64)
    mx = int(counts.max()) if len(counts) else 0
    return {"distinct": len(keys), "singletons": int((counts == 1).sum()), "max_count": mx,
            "max_key": int(keys[counts == mx].min()) if mx else -1, "total_count": int(counts.sum()), "spectrum": spec}


def reference(reads, k, canonical, bits=None, rows=None, prior=None):
    """{the TOTALS, keys, counts, spectrum} of one call: reads by record number; bits: bool per record (None: all
    participate); rows: (start, len) per record (None: whole reads); prior: the (keys, counts) of the table before
    an ACCUMULATE call."""
    tot = dict.fromkeys(CALL_TOTALS, 0)
    tot["records"] = len(reads)
    got = []
    for j, r in enumerate(reads):
        if bits is not None and not bits[j]:
            continue
        s, w = window(rows[j], len(r)) if rows is not None else (0, len(r))
        npos, keys = read_keys(r, k, canonical, s, w)
        tot["participating"] += 1
        tot["short_reads"] += w < k
        tot["bases"] += w
        tot["positions"] += npos
        tot["kmers"] += len(keys)
        got.append(keys)
    tot["invalid"] = tot["positions"] - tot["kmers"]
    keys, counts = tally(np.concatenate(got) if got else [])
    if prior is not None:
        keys, counts = merge_tallies(prior, (keys, counts))
    return dict(tot, keys=keys, counts=counts, **table_totals(keys, counts))


def top(ref, n):
    """[(key, count)] of the n greatest counts of a reference, ties by the lower key."""
    order = np.lexsort((ref["keys"], -ref["counts"]))[:n]
    return [(int(ref["keys"][i]), int(ref["counts"][i])) for i in order]


def word_of(key, k):
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - i))) & 3] for i in range(k))


# ---- the forge ----
Read = collections.namedtuple("Read", "seq cat note")
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150)
N_AT = (0, 31, 32, 63, 64, 149)
GENOME = 4000
POLY = 12          # reads per poly-X: 12 x (150 - 31 + 1) = 1,440 > 1,023 at the largest k


def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


@functools.lru_cache(maxsize=None)
def forge():
    """The tuple of Reads, about 1,500 and fewer than 200 k bases, the same on every call."""
    rng = np.random.default_rng(20261021)
    out = []
    for k in KS:                                   # every length at which a unit or a k-mer begins or ends
        for L in sorted(set(LENGTHS + (k - 1, k, k + 1))):
            out.append(Read(_rand(rng, L), "length", (k, L)))
    for at in N_AT:                                # an N at the borders of the 32-base units
        r = bytearray(_rand(rng, 150))
        r[at] = ord("N")
        out.append(Read(bytes(r), "n_at", at))
    for run in (32, 40, 70):                       # N runs longer than k
        r = bytearray(_rand(rng, 150))
        r[50:50 + run] = b"N" * run
        out.append(Read(bytes(r), "n_run", run))
    for L in (1, 32, 150):
        out.append(Read(b"N" * L, "all_n", L))
    r = bytearray(_rand(rng, 150))
    r[40:45] = bytes(r[40:45]).lower()
    out.append(Read(bytes(r), "lower", None))
    out.append(Read(_rand(rng, 149) + b"\r", "crlf", None))
    for base in b"ATG":                            # hot keys: one count above the spectrum's last bin
        for _ in range(POLY):
            out.append(Read(bytes([base]) * 150, "poly", chr(base)))
    for half in (1, 8):                            # reverse-complement palindromes of even k = 2, 16
        w = _rand(rng, half)
        out.append(Read(_rand(rng, 40) + w + revcomp(w) + _rand(rng, 40), "palindrome", 2 * half))
    r = _rand(rng, 150)
    out += [Read(r, "strand", "+"), Read(revcomp(r), "strand", "-")]
    genome = _rand(rng, GENOME)                    # coverage ~40: a singleton peak from the errors and a coverage peak
    for _ in range(1100):
        a = int(rng.integers(0, GENOME - 150))
        r = bytearray(genome[a:a + 150])
        for i in np.nonzero(rng.random(150) < 0.01)[0]:
            r[i] = b"CGTA"[b"ACGT".index(bytes([r[i]]))]
        out.append(Read(revcomp(bytes(r)) if rng.random() < 0.5 else bytes(r), "genome", a))
    while len(out) % 64 == 0 or len(out) % 64 == 63:
        out.append(Read(_rand(rng, 77), "pad", None))
    return tuple(out)


def forge_reads():
    return [r.seq for r in forge()]


@functools.lru_cache(maxsize=None)
def forge_reference(k, canonical):
    """reference of the whole forge; shared, read-only."""
    ref = reference(forge_reads(), k, canonical)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
