"""Reference for the pair merge (include/ppgpu.h "pair merge"), restated in plain Python from that section's
text, not from the kernel and not from any tool; plus the qualities of the forge of read pairs
(tests/pairoverlap_ref.py) and the helpers the merge tests share.  Reads are byte strings as in the overlap's
reference; qualities are byte strings of the same length, the bytes of the packed set's qual plane.

merge_one does one merged pair position by position; merge_reference applies the maps, the classes, the
compaction, the planes, pair_of and the counters."""
import collections
import functools
import zlib

import numpy as np

import pairoverlap_ref as V

MAX_LEN = V.MAX_LEN
CLASSES = ("unmapped", "too_long", "unmerged", "stale", "merged")
COUNTERS = ("overlap_bases", "disagree", "from2", "ties", "n_filled", "n_both")
TOTALS = ("pairs",) + CLASSES + ("merged_bases", "padded_bases") + COUNTERS

Merge = collections.namedtuple("Merge", "qual_hi qual_lo")
DEFAULT = Merge(63, 47)


def struct_of(m):
    from parallelparsing_amd import _lib
    import ctypes as C
    return _lib.PpgPairMerge(0, m.qual_hi, m.qual_lo, (C.c_int64 * 5)())


@functools.lru_cache(maxsize=None)
def merge_one(s1, q1, s2, q2, d, m=DEFAULT):
    """(sequence, quality, counters) of a merged pair: -L2 < d < L1, I = L2 + d.  counters: the COUNTERS and
    corrected0 / corrected1."""
    L1, L2 = len(s1), len(s2)
    I = L2 + d
    assert -L2 < d < L1 and len(q1) == L1 and len(q2) == L2
    c1, n1 = V.codes(s1)
    c2, n2 = V.codes(s2)
    cnt = dict.fromkeys(COUNTERS + ("corrected0", "corrected1"), 0)
    seq, qual = bytearray(), bytearray()
    for p in range(I):
        side1 = side_r = None
        if p < L1:
            side1 = (int(c1[p]), bool(n1[p]), q1[p])
        if p >= d:
            t = p - d
            side_r = (3 - int(c2[L2 - 1 - t]), bool(n2[L2 - 1 - t]), q2[L2 - 1 - t])
        assert side1 or side_r
        if side1 and side_r:
            (ca, na, qa), (cr, nr, qr) = side1, side_r
            take_r = (na and not nr) or (na == nr and qr > qa)
            cnt["overlap_bases"] += 1
            if na and nr:
                cnt["n_both"] += 1
            elif na or nr:
                cnt["n_filled"] += 1
            elif ca != cr:
                cnt["disagree"] += 1
                cnt["from2"] += take_r
                cnt["ties"] += qr == qa
                (qt, qo) = (qr, qa) if take_r else (qa, qr)
                if qt >= m.qual_hi and qo <= m.qual_lo:
                    cnt["corrected0" if take_r else "corrected1"] += 1
            c, n, q = side_r if take_r else side1
        else:
            c, n, q = side1 or side_r
        seq.append(ord("N") if n else b"ACGT"[c])
        qual.append(q)
    return bytes(seq), bytes(qual), cnt


def classify(L1, L2, row):
    """The class of a mapped pair with the row (d, ., ., I), in Python's integers."""
    d, I = int(row[0]), int(row[3])
    if L1 > MAX_LEN or L2 > MAX_LEN:
        return "too_long"
    if I == 0:
        return "unmerged"
    if not (-L2 < d < L1 and I == L2 + d):
        return "stale"
    return "merged"


def merge_reference(set1, qual1, set2, qual2, rows, m=DEFAULT, rec1=None, rec2=None, npairs=None):
    """{the TOTALS, corrected (2), seqs / quals (the merged reads in order), pair_of int64[merged], and the merged
    set's planes seq_off, seq_len, bases, mask, qual (numpy, exactly seq_off[merged] bases)}."""
    if npairs is None:
        npairs = len(rec1) if rec1 is not None else len(rec2) if rec2 is not None else min(len(set1), len(set2))
    tot = dict.fromkeys(TOTALS, 0)
    corrected = [0, 0]
    seqs, quals, pair_of = [], [], []
    for i in range(npairs):
        r1 = int(rec1[i]) if rec1 is not None else i
        r2 = int(rec2[i]) if rec2 is not None else i
        tot["pairs"] += 1
        if not (0 <= r1 < len(set1) and 0 <= r2 < len(set2)):
            tot["unmapped"] += 1
            continue
        cls = classify(len(set1[r1]), len(set2[r2]), rows[i])
        tot[cls] += 1
        if cls != "merged":
            continue
        s, q, cnt = merge_one(set1[r1], qual1[r1], set2[r2], qual2[r2], int(rows[i][0]), m)
        assert len(s) == int(rows[i][3]) and 1 <= len(s) <= 2047
        seqs.append(s)
        quals.append(q)
        pair_of.append(i)
        for k in COUNTERS:
            tot[k] += cnt[k]
        corrected[0] += cnt["corrected0"]
        corrected[1] += cnt["corrected1"]
    planes = pack_strings(seqs, quals)
    tot["merged_bases"] = sum(len(s) for s in seqs)
    tot["padded_bases"] = int(planes["seq_off"][-1])
    return dict(tot, corrected=tuple(corrected), seqs=seqs, quals=quals, pair_of=np.array(pair_of, np.int64), **planes)


def pack_strings(reads, quals):
    """{seq_off, seq_len, bases, mask, qual} of the packed reads format for lists of reads and their quality
    strings (cut or zero-filled to the read's length), from the format's text."""
    h = V.pack_strings(reads)
    qual = np.zeros(int(h["seq_off"][-1]), np.uint8)
    for j, (s, q) in enumerate(zip(reads, quals)):
        b, n = int(h["seq_off"][j]), min(len(s), len(q))
        qual[b:b + n] = np.frombuffer(bytes(q[:n]), np.uint8)
    return dict(h, qual=qual)


# ---- the forge's qualities ----
@functools.lru_cache(maxsize=None)
def forge_quals():
    """(quals of r1, quals of r2) for every pair of V.forge(), the same on every call: independent bytes in
    [35, 74) per base, so ties, both directions of a choice and both kinds of corrected occur by chance.  Every
    11th pair has a zero-filled tail on one mate (the packed format's malformed record), every 13th constant
    quality on both (every disagreement a tie)."""
    rng = np.random.default_rng(20261021)
    q1s, q2s = [], []
    for k, p in enumerate(V.forge()):
        qs = [rng.integers(35, 74, size=len(s)).astype(np.uint8) for s in (p.r1, p.r2)]
        cut = int(rng.integers(1, 60))
        if k % 11 == 3:
            q = qs[(k // 11) & 1]
            q[max(len(q) - cut, 0):] = 0
        if k % 13 == 5:
            for q in qs:
                q[:] = 73
        q1s.append(qs[0].tobytes())
        q2s.append(qs[1].tobytes())
    return tuple(q1s), tuple(q2s)


def forge_sets(which="identity"):
    """(set1, qual1, set2, qual2, rec1, rec2): V.forge_sets with the qualities stored beside their reads."""
    set1, set2, rec1, rec2 = V.forge_sets(which)
    q1s, q2s = forge_quals()
    if which == "identity":
        return set1, list(q1s), set2, list(q2s), None, None
    n = len(set1)
    # the maps before V.forge_sets punches its holes: pair i's records
    rng = np.random.default_rng(7)
    full1 = np.arange(n - 1, -1, -1, dtype=np.int64)
    full2 = rng.permutation(n).astype(np.int64)
    qual1, qual2 = [None] * n, [None] * n
    for i in range(n):
        qual1[full1[i]], qual2[full2[i]] = q1s[i], q2s[i]
    return set1, qual1, set2, qual2, rec1, rec2


@functools.lru_cache(maxsize=None)
def forge_reference(pname, which="identity", m=DEFAULT):
    """merge_reference of the forge with the reference overlap's rows under a parameter set and a map; shared,
    read-only."""
    set1, qual1, set2, qual2, rec1, rec2 = forge_sets(which)
    rows = V.forge_reference(pname, which, windows=False)["rows"]
    ref = merge_reference(set1, qual1, set2, qual2, rows, m, rec1, rec2)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- a forged R1 / R2 pair of files with qualities ----
# mate_file and oracle_chunks restate the helpers of tests/test_gpu_pairoverlap.py (which writes constant qualities
# and is a test file, not a module to import from): a change to the flush or the duplicate-record rule belongs in both.
def file_quals(q):
    """A quality string as it can stand in a FASTQ line of these files: the zero bytes of a malformed tail as '#',
    and no '@', which the index takes for a record start when it follows a flush."""
    return bytes(q).replace(b"\0", b"#").replace(b"@", b"A")


def mate_file(pairs, quals, mate, flush_every):
    """The mate's FASTQ as one gzip member with the given quality strings, a full flush after every flush_every
    records: Points fall on record starts, so the reference parses some records twice."""
    recs = []
    for i, (p, q) in enumerate(zip(pairs, quals)):
        s = p.r1 if mate == 1 else p.r2
        assert len(q) == len(s)
        recs.append(b"@SRR9.%d.%d\n%s\n+\n%s\n" % (i + 1, mate, s, q))
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = []
    for g in range(0, len(recs), flush_every):
        out.append(co.compress(b"".join(recs[g:g + flush_every])))
        out.append(co.flush(zlib.Z_FULL_FLUSH))
    out.append(co.flush())
    return b"".join(out)


def oracle_chunks(gz, cs):
    """Per chunk, from the oracle: (offset_k, raw_k, descriptors), and per shard record whether it is a Q1 duplicate."""
    from oracle import oracle as O
    oi = O.build_index(gz, cs)
    chunks, dup = [], []
    for k in range(oi.count - 1):
        off = oi.point(k)[4]
        desc = np.asarray(O.parse(off, O.extract(gz, oi, k)), np.uint32).reshape(-1, 4)
        chunks.append((off, off + O.extract(gz, oi, k), desc))
        dup += [j == 0 and int(d[3]) < len(off) for j, d in enumerate(desc)]
    return chunks, np.array(dup, bool)


def words(t):
    """A CUDA tensor of 32-bit words as a numpy uint32 array."""
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
