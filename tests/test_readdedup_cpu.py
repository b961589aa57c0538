"""The read dedup without a GPU: the reference of the semantics (tests/readdedup_ref.py) on hand-made inputs, the
guards that the inputs of tests/test_gpu_readdedup.py are what they claim, the struct checks through the
host-only path of the library, and the ABI's presence in the header, the binding and the C# externs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import fastq_forge as FF
import seqpack_ref as R
import readtrim_ref as T
import readdedup_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk_of(seqs):
    """One chunk (no offset carry) of records with these Sequences, as the oracle would describe it."""
    raw, desc, pos = b"", [], 0
    for i, s in enumerate(seqs):
        rec = b"@h%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s))
        n1 = pos + rec.index(b"\n")
        n2 = n1 + 1 + len(s)
        n3 = n2 + 2
        desc.append((n1, n2, n3, n3 + 1 + len(s)))
        raw += rec
        pos += len(rec)
    return (b"", raw, np.array(desc, np.uint32).reshape(-1, 4))


# ---- 1. the fingerprint, restated once more with numpy's wrapping uint64 arithmetic ----
def _mix_np(x):
    m, s = np.uint64(D.MUL), np.uint64(32)
    x = x ^ (x >> s)
    x = x * m
    x = x ^ (x >> s)
    x = x * m
    return x ^ (x >> s)


def fingerprint_np(key):
    with np.errstate(over="ignore"):
        G = np.uint64(0)
        for i in range((len(key) + 31) // 32):
            w = np.frombuffer(key[32 * i:32 * i + 32].ljust(32, b"\0"), "<u8")
            a = _mix_np(np.uint64(D.GOLD) * np.uint64(i + 1))
            for t in range(4):
                a = _mix_np(a ^ w[t])
            G = G + a
        f = _mix_np(G ^ _mix_np(np.uint64(len(key)) + np.uint64(D.LEN)))
    return int(f) or 1


def test_fingerprint_two_ways():
    rng = np.random.default_rng(2)
    for n in (0, 1, 7, 8, 31, 32, 33, 63, 64, 65, 150, 2100):
        key = rng.integers(1, 256, n, dtype=np.uint8).tobytes()
        assert D.fingerprint(key) == fingerprint_np(key) != 0, n
    assert D.mix(0) == 0 and D.mix(1) != 1 and len({D.mix(x) for x in range(1000)}) == 1000
    # the home slot is the top bits of the product; the smallest legal table
    assert D.home_slot(1, 64) == D.GOLD >> 58 and D.home_slot(D.M64, 1 << 20) < 1 << 20
    assert [D.min_slots(n) for n in (0, 1, 32, 33, 64, 65, 34904)] == [64, 64, 64, 128, 128, 256, 131072]
    assert [pp.ReadDedup.min_slots(n) for n in (0, 32, 33, 34904)] == [64, 64, 128, 131072]
    assert [D.level_of(c) for c in (1, 9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000, 10 ** 6)] == \
        [0, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15]


def test_reference_on_a_hand_made_chunk():
    seqs = [b"ACGT", b"TTTT", b"ACGT", b"", b"ACGTA", b"", b"TTTT", b"ACGT"]
    ch = [chunk_of(seqs)]
    r = D.dedup_reference(ch, D.dedup())
    assert [r[k] for k in D.TOTALS] == [8, 8, 4, 25, 13, 0, 3, 0]
    assert r["first"].tolist() == [0, 1, 0, 3, 4, 3, 1, 0] and r["unique_bits"].tolist() == [1, 1, 0, 1, 1, 0, 0, 0]
    assert r["level_distinct"].tolist() == [1, 2, 1] + [0] * 13 and r["level_reads"].tolist() == [1, 4, 3] + [0] * 13
    assert r["mask"].tolist() == [0b00011011] and r["chunk_unique"].tolist() == [4]
    assert D.top_of(r, 2) == [(3, 0), (2, 1)] and D.top_of(r, 9) == [(3, 0), (2, 1), (2, 3), (1, 4)]
    # max_bases cuts the key: ACGT and ACGTA merge at 4, everything non-empty but TTTT at 1
    assert D.dedup_reference(ch, D.dedup(4))["first"].tolist() == [0, 1, 0, 3, 0, 3, 1, 0]
    assert D.dedup_reference(ch, D.dedup(1))["unique"] == 3
    # a mask that clears record 0 makes record 2 the first; cleared records get -1 and keep their cleared bit
    keep = np.array([0, 1, 1, 1, 1, 0, 1, 1], bool)
    m = D.dedup_reference(ch, D.dedup(), keep, prior=np.array([0xFFFFFF00 | 0b11011110], np.uint32))
    assert m["first"].tolist() == [-1, 1, 2, 3, 4, -1, 1, 2] and m["participating"] == 6 and m["max_first"] == 1
    assert m["mask"].tolist() == [0xFFFFFF00 | 0b00011110]
    # windows: rows are clamped, and only the window's bytes count
    rows = np.array([(1, 2), (9, 9), (1, 2), (0, 5), (1, 2), (7, 0), (4, 4), (1, 0xFFFFFFFF)], np.uint32)
    w = D.dedup_reference(ch, D.dedup(), None, rows)
    assert w["keys"] == [b"CG", b"", b"CG", b"", b"CG", b"", b"", b"CGT"] and w["first"].tolist() == [0, 1, 0, 1, 0, 1, 1, 7]
    # an empty input: an empty table
    e = D.dedup_reference([], D.dedup())
    assert (e["max_count"], e["max_first"], e["unique"]) == (0, -1, 0) and e["table"].shape == (0, 3)


# ---- 2. the inputs of tests/test_gpu_readdedup.py ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_golden_inputs_fingerprints_are_exact(name):
    """On every input used, fingerprint equality coincides with byte equality of the key bytes."""
    for mb in D.MAX_BASES:
        r = D.reference(name, D.dedup(mb))
        assert len(set(r["F"].tolist())) == len(set(r["keys"])) == r["unique"], (name, mb)
        assert r["level_distinct"].sum() == r["unique"] and r["level_reads"].sum() == r["participating"] == r["records"]


def test_forged_input_is_what_it_claims():
    chunks, recs = D.forged_chunks(), D.forged_records()
    fields = T.fields(chunks)
    assert [s for _, s, _ in fields] == [s for _, s in recs]                  # the oracle parses what was forged
    n = len(recs)
    slots = D.min_slots(n)
    assert n == 34904 and slots == 131072 and 2 * n <= slots < 4 * n
    for which in ("plain", "mask", "rows", "mask_rows"):
        for mb in D.MAX_BASES:
            r = D.forged_reference(D.dedup(mb), which)
            assert len(set(r["F"].tolist())) == len(set(r["keys"])), (which, mb)
            assert r["level_distinct"].sum() == r["unique"] and r["level_reads"].sum() == r["participating"]
    plain = D.forged_reference(D.dedup(0))
    # the copy counts: both edges of every bin, every bin non-empty, the hot key a 1-base read
    counts = sorted(int(c) for c in plain["table"][:, 2])
    assert set(D.COPIES) <= set(counts) and (plain["level_distinct"] > 0).all()
    for b, lo in enumerate(D.LEVEL_LO):
        hi = D.LEVEL_LO[b + 1] - 1 if b < 15 else None
        assert lo in counts and (hi is None or hi in counts), (lo, hi)
    assert (plain["max_count"], plain["keys"][plain["max_first"]]) == (10000, D.HOT)
    # the lengths
    lens = {len(k) for k in plain["keys"]}
    assert {0, 1, 31, 32, 33, 64, 65} <= lens and max(lens) > 2048
    for L in D.LENGTHS:
        pair = [j for j, (tag, _) in enumerate(recs) if tag == ("length", L, 2)]
        assert len(pair) == 2 and plain["first"][pair[1]] == plain["first"][pair[0]] <= pair[0], L
    # where copies sit: adjacent, in one chunk, across chunks, across the offset-carry seam, across batches
    first, chunk = plain["first"], np.array([k for k, _, _ in fields])
    dup = np.flatnonzero(first != np.arange(n))
    cold = [j for j in dup if plain["keys"][j] != D.HOT]
    assert any(first[j] == j - 1 for j in cold) and any(chunk[j] == chunk[first[j]] for j in cold)
    assert any(chunk[j] != chunk[first[j]] for j in cold)
    seam = [j for k, (off, _, desc) in enumerate(chunks) for j0, d in enumerate(desc.tolist())
            if d[0] + 1 < len(off) < d[1] for j in [int(np.flatnonzero(chunk == k)[0]) + j0]]
    assert any(first[j] != j and len(plain["keys"][j]) > 1 for j in seam)      # a copy whose Sequence crosses the seam
    bat = FF.batches([len(raw) - len(off) for off, raw, _ in chunks], 8192)
    assert len(bat) > 100
    batch_of = np.zeros(len(chunks), np.int64)
    for b, (k0, k1) in enumerate(bat):
        batch_of[k0:k1] = b
    assert any(batch_of[chunk[j]] != batch_of[chunk[first[j]]] for j in cold)
    # the planted pairs: a single byte, a unit swap and a length all change F
    F = plain["F"]
    at = {tag[1:]: j for j, (tag, _) in enumerate(recs) if tag[0] == "pair"}
    for name in ("last_byte", "second_unit", "prefix", "pad_alike", "units_swapped", "first_50", "window_only"):
        a, b = at[(name, 0)], at[(name, 1)]
        assert F[a] != F[b] and first[a] == a and first[b] == b, name
    a, b = plain["keys"][at[("prefix", 0)]], plain["keys"][at[("prefix", 1)]]
    assert a.startswith(b) and len(a) == len(b) + 1
    a, b = plain["keys"][at[("pad_alike", 0)]], plain["keys"][at[("pad_alike", 1)]]
    assert len(a) == 32 and b[:32] == a and len(b) == 33 and 0 not in b        # one more byte in the next unit, no NUL
    a, b = plain["keys"][at[("units_swapped", 0)]], plain["keys"][at[("units_swapped", 1)]]
    assert a[:32] == b[32:] and a[32:] == b[:32] and a != b
    # ... equal in their first 50 bases: one key at max_bases = 50, two at 0
    f50 = D.forged_reference(D.dedup(50))["first"]
    assert f50[at[("first_50", 1)]] == f50[at[("first_50", 0)]] == min(at[("first_50", 0)], at[("first_50", 1)])
    # ... equal only inside their windows, which start at 3 and 5
    rows, wref = D.forged_rows(), D.forged_reference(D.dedup(0), "rows")
    a, b = at[("window_only", 0)], at[("window_only", 1)]
    assert rows[a, 0] % 4 and rows[b, 0] % 4 and wref["keys"][a] == wref["keys"][b] == D.WINDOW_CORE
    assert wref["first"][a] == wref["first"][b] == min(a, b)
    # hostile rows of every kind, and the clamp matters
    L = np.array([len(s) for _, s in recs], np.int64)
    assert (rows[:, 0] > L).any() and (rows[:, 0].astype(np.int64) + rows[:, 1] > L).any() and (rows == 0xFFFFFFFF).all(axis=1).any()
    assert 0 < wref["bases"] < plain["bases"]
    # the random mask: neither empty nor full, two words longer, and it clears some first occurrences, so that a
    # later copy becomes the first
    keep = D.bits_of(D.forged_random_mask(), n)
    mref = D.forged_reference(D.dedup(0), "mask")
    assert D.forged_random_mask().size == (n + 31) // 32 + 2 and 0 < keep.sum() < n
    moved = [j for j in np.flatnonzero(keep) if mref["first"][j] > plain["first"][j]]
    assert len(moved) > 10 and (mref["first"][~keep] == -1).all()
    # the table at its smallest: a home slot shared by three distinct keys, and a cluster that wraps past the last row
    homes = np.bincount([D.home_slot(int(k), slots) for k in plain["table"][:, 0]], minlength=slots)
    assert homes.max() >= 3
    assert homes[-1] >= 2 or (homes[-2] >= 3) or (homes[-2:].sum() >= 3 and homes[-1] >= 1)   # more keys than rows up to the end


# ---- 3. the library without a device ----
def test_struct_checks_and_null_handles_without_a_device():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    assert C.sizeof(_lib.PpgReadDedup) == 32 and C.sizeof(_lib.PpgReadDedupResult) == 8 * 40
    assert _lib.PpgReadDedupResult.level_distinct.offset == 64 and _lib.PpgReadDedupResult.level_reads.offset == 8 * 24
    check = lib.ppg_read_dedup_check
    mk = lambda *a: _lib.PpgReadDedup(a[0], a[1], (C.c_int64 * 2)(*a[2:]))   # noqa: E731
    for good in (mk(0, 0, 0, 0), mk(2, 50, 0, 0), mk(0x100, 1, 0, 0), mk(0x102, 1 << 40, 0, 0)):
        assert check(C.byref(good)) == 0
    for bad in (mk(1, 0, 0, 0), mk(4, 0, 0, 0), mk(0x200, 0, 0, 0), mk(0, -1, 0, 0), mk(0, 0, 1, 0), mk(0, 0, 0, 7)):
        assert check(C.byref(bad)) == E
    assert check(None) == E
    s = pp.ReadDedup(50).struct(and_mask=True, use_windows=True)
    assert (s.flags, s.max_bases, list(s.reserved)) == (0x102, 50, [0, 0]) and pp.ReadDedup().struct().flags == 0
    with pytest.raises(ValueError):
        pp.ReadDedup(-1).struct()
    good, res = pp.ReadDedup().struct(), _lib.PpgReadDedupResult()
    assert lib.ppg_shard_dedup_reads(None, C.byref(good), None, 0, None, 0, None, 0, None, 64, None, C.byref(res)) == E
    assert lib.ppg_shard_set_readdedup(None, C.byref(good), None, 0, None, 0, None, 0, None, 64) == E
    assert lib.ppg_shard_readdedup_ready(None, None, C.byref(res)) == E
    b = pp.BatchedFASTQ.__new__(pp.BatchedFASTQ)      # a rank of a job: the counts are single process
    b.world, b.rank = 2, 0
    with pytest.raises(ValueError):
        b.Duplication()
    with pytest.raises(ValueError):
        b.CountUnique()


def test_result_views():
    r = D.dedup_reference([chunk_of([b"ACGT", b"TTTT", b"ACGT", b""])], D.dedup())
    res = _lib.PpgReadDedupResult(*[r[k] for k in D.TOTALS], (C.c_int64 * 16)(*r["level_distinct"]),
                                  (C.c_int64 * 16)(*r["level_reads"]))
    v = pp.ReadDedupResult(res, r["chunk_unique"])
    assert [getattr(v, k) for k in D.TOTALS] == [r[k] for k in D.TOTALS] == [4, 4, 3, 12, 8, 0, 2, 0]
    assert np.array_equal(v.level_distinct, r["level_distinct"]) and np.array_equal(v.level_reads, r["level_reads"])
    assert v.duplication_rate == 0.25 and len(v.LEVELS) == 16
    assert pp.ReadDedupResult(_lib.PpgReadDedupResult()).duplication_rate == 0.0
    with pytest.raises(ValueError):
        v.top(3)


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    for name in ("ppg_read_dedup_check", "ppg_shard_dedup_reads", "ppg_shard_set_readdedup", "ppg_shard_readdedup_ready"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert hasattr(_lib.lib, "ppgx_readdedup_times")
    assert "} ppg_read_dedup;" in h and "} ppg_read_dedup_result;" in h
    assert h.index("read profile:") < h.index("read dedup:") < h.index("typedef struct ppg_cursor ppg_cursor;")
    flat = re.sub(r"\s*\n \*\s*", " ", h)
    assert flat.count("keys, pack, query, filter, trim, dedup, profile, select") >= 2
    assert "if and only if their F is equal" in flat and "N^2 / 2^65" in flat and "0xD6E8FEB86659FD93" in flat
    assert "struct PpgReadDedup " in cs and "struct PpgReadDedupResult" in cs
