"""The read profile without a GPU: the reference of the semantics (tests/readprofile_ref.py) against records
worked by hand and against the references of the query and the filter, ppg_read_profile_check and
ReadProfile.struct() on every refused field, the ABI's presence, and the inputs of
tests/test_gpu_readprofile.py being what that file says they are."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import seqpack_ref as R
import seqquery_ref as Q
import readfilter_ref as F
import readtrim_ref as T
import readprofile_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk_of(records):
    """One chunk (no offset carry) of hand-written (sequence, quality) records: (b"", raw, descriptors)."""
    raw, desc = b"", []
    for i, (s, q) in enumerate(records):
        a = len(raw)
        ident = b"@r%d" % i
        n1 = a + len(ident)
        n2 = n1 + 1 + len(s)
        n3 = n2 + 2
        n4 = n3 + 1 + len(q)
        raw += ident + b"\n" + s + b"\n+\n" + q + b"\n"
        desc.append((n1, n2, n3, n4))
    assert all(raw[n] == 10 for d in desc for n in d)
    return (b"", raw, np.array(desc, np.uint32))


# L = 0; Lq < L; Lq > L; bytes below qual_base and above qual_base + 63, lower case; no Quality at all
HAND = ((b"", b""), (b"ACGTN", b"!#I"), (b"GC", b"~~~~"), (b"acgtAC", bytes([11, 200, 33, 34, 96, 97])), (b"TT", b""))


def _table(rows):
    t = np.zeros(len(rows), P.ROW_DTYPE)
    for p, (base, n, s, here, hist) in enumerate(rows):
        t["base"][p], t["qual_n"][p], t["qual_sum"][p], t["len_here"][p] = base, n, s, here
        for b, v in hist.items():
            t["qhist"][p][b] = v
    return t


def _hist(n, bins):
    h = np.zeros(n, np.int64)
    for b, v in bins.items():
        h[b] = v
    return h


def assert_same(got, want):
    for k in P.TOTALS:
        assert got[k] == want[k], k
    for k in ("gc_hist", "meanq_hist", "chunk_profiled"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k])[0], got[k][np.nonzero(got[k])[0]])
    for f in P.ROW_DTYPE.names:
        assert np.array_equal(got["table"][f], want["table"][f]), (f, got["table"][f])


def test_reference_on_hand_written_records():
    chunks = [chunk_of(HAND)]
    # every record, whole reads, four positions: ACGTN and acgtAC are longer
    want = dict(records=5, profiled=5, longer=2, bases=15, bases_profiled=12, qual_bytes=11, no_quality=1,
                gc_hist=_hist(101, {40: 1, 100: 1, 16: 1, 0: 1}), meanq_hist=_hist(64, {14: 1, 63: 1, 45: 1}),
                chunk_profiled=np.array([5]),
                table=_table([((1, 0, 1, 1, 1), 3, 33 + 126 + 11, 1, {0: 2, 63: 1}),
                              ((0, 2, 0, 1, 1), 3, 35 + 126 + 200, 0, {2: 1, 63: 2}),
                              ((0, 0, 1, 0, 1), 2, 73 + 33, 2, {40: 1, 0: 1}),
                              ((0, 0, 0, 1, 1), 1, 34, 0, {1: 1})]))
    assert_same(P.profile_reference(chunks, P.profile(4)), want)
    # a mask without GC, and rows: past an empty read, inside, and one that runs 94 bases past the end
    keep = np.array([1, 1, 0, 1, 0], bool)
    rows = np.array([(5, 5), (1, 2), (0, 2), (2, 100), (0, 2)], np.uint32)
    want = dict(records=5, profiled=3, longer=1, bases=6, bases_profiled=6, qual_bytes=6, no_quality=0,
                gc_hist=_hist(101, {100: 1, 25: 1}), meanq_hist=_hist(64, {21: 1, 32: 1}), chunk_profiled=np.array([3]),
                table=_table([((0, 1, 0, 0, 1), 2, 35 + 33, 1, {2: 1, 0: 1}),
                              ((0, 0, 1, 0, 1), 2, 73 + 34, 0, {40: 1, 1: 1}),
                              ((1, 0, 0, 0, 0), 1, 96, 1, {63: 1}),
                              ((0, 1, 0, 0, 0), 1, 97, 0, {63: 1})]))
    assert_same(P.profile_reference(chunks, P.profile(4), keep, rows), want)
    # one position: everything but row 0 is `longer` or dropped, the per-record numbers stay whole
    one = P.profile_reference(chunks, P.profile(1), keep, rows)
    assert (one["longer"], one["bases"], one["bases_profiled"], one["qual_bytes"]) == (2, 6, 2, 6)
    assert np.array_equal(one["gc_hist"], want["gc_hist"]) and np.array_equal(one["meanq_hist"], want["meanq_hist"])
    assert one["table"]["base"].tolist() == [[0, 1, 0, 0, 1]] and one["table"]["len_here"].tolist() == [1]
    # another qual_base moves the bins, not the sums
    z = P.profile_reference(chunks, P.profile(4, qual_base=0))
    assert z["table"]["qual_sum"].tolist() == [170, 361, 106, 34] and z["table"]["qhist"][0][[11, 33, 63]].tolist() == [1, 1, 1]
    assert np.array_equal(z["meanq_hist"], _hist(64, {47: 1, 63: 2}))


@pytest.mark.parametrize("name", ("memlevel1_c10", R.SYNTH))
def test_identities_with_the_other_references(name):
    chunks = R.oracle_chunks(name)
    qref, fref = Q.reference(name, None), F.reference(name, F.FILTERS[0])
    longest = int(fref["metrics"]["length"].max())
    assert longest < P.MAX_POS
    ref = P.reference(name, P.profile(longest + 1))
    assert ref["longer"] == 0 and ref["records"] == ref["profiled"] == qref["records"]
    assert np.array_equal(ref["table"]["base"].sum(axis=0), qref["counts"])
    assert np.array_equal(ref["table"]["len_here"], np.bincount(fref["metrics"]["length"], minlength=longest + 1))
    assert ref["bases"] == ref["bases_profiled"] == fref["bases"] == qref["bases"]
    assert np.array_equal(ref["chunk_profiled"], [len(np.asarray(d).reshape(-1, 4)) for _, _, d in chunks])
    assert np.array_equal(ref["table"]["qhist"].sum(axis=1), ref["table"]["qual_n"])
    assert int(ref["gc_hist"].sum()) == int((fref["metrics"]["length"] > 0).sum())
    if name == R.SYNTH:    # Lq = L: every Quality byte belongs to a base, so the census folds into the bins
        assert np.array_equal(fref["metrics"]["length"], fref["metrics"]["qual_length"])
        folded = np.bincount(np.clip(np.arange(256) - 33, 0, 63), weights=fref["qual_count"], minlength=64).astype(np.int64)
        assert np.array_equal(ref["table"]["qhist"].sum(axis=0), folded)
        assert ref["qual_bytes"] == fref["qual_bytes"]
        assert int(ref["table"]["qual_sum"].sum()) == int(fref["metrics"]["qual_sum"].sum())


def _check(**kw):
    good = dict(flags=0, qual_base=33, max_pos=256, reserved=0)
    good.update(kw)
    return _lib.lib.ppg_read_profile_check(C.byref(_lib.PpgReadProfile(**good)))


def test_read_profile_check_rules():
    OK, E = _lib.PPG_OK, _lib.PPG_ARG_ERROR
    assert _lib.lib.ppg_read_profile_check(None) == E
    assert _check() == OK
    assert _check(flags=1) == OK and _check(flags=2) == OK and _check(flags=3) == OK
    assert _check(flags=4) == E and _check(flags=0x100) == E and _check(flags=-1) == E
    assert _check(qual_base=0) == OK and _check(qual_base=255) == OK and _check(qual_base=-1) == E and _check(qual_base=256) == E
    assert _check(max_pos=1) == OK and _check(max_pos=1024) == OK
    assert _check(max_pos=0) == E and _check(max_pos=1025) == E and _check(max_pos=-5) == E and _check(max_pos=1 << 40) == E
    assert _check(reserved=1) == E and _check(reserved=-1) == E


def test_read_profile_struct_conversion():
    s = pp.ReadProfile().struct()
    assert (s.flags, s.qual_base, s.max_pos, s.reserved) == (0, 33, 256, 0)
    s = pp.ReadProfile(max_positions=160, qual_base=64).struct(use_mask=True, use_windows=True)
    assert (s.flags, s.qual_base, s.max_pos, s.reserved) == (3, 64, 160, 0)
    assert pp.ReadProfile(1).struct(use_windows=True).flags == P.USE_WINDOWS
    for bad in (pp.ReadProfile(0), pp.ReadProfile(1025), pp.ReadProfile(-1), pp.ReadProfile(256, -1), pp.ReadProfile(256, 256)):
        with pytest.raises(ValueError):
            bad.struct()


def test_struct_sizes_and_null_handles_without_a_device():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    good, res = pp.ReadProfile(4).struct(), _lib.PpgReadProfileResult()
    assert C.sizeof(_lib.PpgReadProfile) == 32 and C.sizeof(res) == 8 * 173
    assert _lib.PpgReadProfileResult.gc_hist.offset == 64 and _lib.PpgReadProfileResult.meanq_hist.offset == 8 * 109
    assert P.ROW_DTYPE.itemsize == pp.ReadProfileResult.ROW_DTYPE.itemsize == 8 * 72
    table = np.zeros((4, 72), np.int64)
    tp = table.ctypes.data_as(C.c_void_p)
    assert lib.ppg_shard_profile_reads(None, C.byref(good), None, 0, None, 0, None, C.byref(res), tp, 4) == E
    assert lib.ppg_shard_set_readprofile(None, C.byref(good), None, 0, None, 0) == E
    assert lib.ppg_shard_readprofile_ready(None, None, C.byref(res), tp, 4) == E
    b = pp.BatchedFASTQ.__new__(pp.BatchedFASTQ)      # a rank of a job: the counts are single process
    b.world, b.rank = 2, 0
    with pytest.raises(ValueError):
        b.Profile()


def test_result_views():
    ref = P.profile_reference([chunk_of(HAND)], P.profile(4))
    res = _lib.PpgReadProfileResult(*[ref[k] for k in P.TOTALS], 0, (C.c_int64 * 101)(*ref["gc_hist"]),
                                    (C.c_int64 * 64)(*ref["meanq_hist"]))
    r = pp.ReadProfileResult(res, ref["table"].view(np.int64).reshape(-1, 72), ref["chunk_profiled"], 33)
    assert [getattr(r, k) for k in P.TOTALS] == [ref[k] for k in P.TOTALS]
    assert np.array_equal(r.base_counts, ref["table"]["base"]) and np.array_equal(r.length_hist, [1, 0, 2, 0])
    assert np.array_equal(r.gc_hist, ref["gc_hist"]) and np.array_equal(r.meanq_hist, ref["meanq_hist"])
    assert r.mean_quality.tolist() == [170 / 3 - 33, 361 / 3 - 33, 106 / 2 - 33, 34 - 33]
    empty = pp.ReadProfileResult(_lib.PpgReadProfileResult(), np.zeros((2, 72), np.int64))
    assert np.isnan(empty.mean_quality).all()


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    for name in ("ppg_read_profile_check", "ppg_shard_profile_reads", "ppg_shard_set_readprofile",
                 "ppg_shard_readprofile_ready"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert hasattr(_lib.lib, "ppgx_readprofile_times") and hasattr(_lib.lib, "ppgx_readprofile_grid")
    assert "} ppg_read_profile;" in h and "} ppg_read_profile_result;" in h
    assert h.index("read trimming:") < h.index("read profile:") < h.index("typedef struct ppg_cursor ppg_cursor;")
    assert "keys, pack, query, filter, trim, profile, select" in re.sub(r"\s*\n \*\s*", " ", h)
    assert "struct PpgReadProfile " in cs and "struct PpgReadProfileResult" in cs


# ---- the inputs of tests/test_gpu_readprofile.py ----
def test_gpu_test_inputs_are_what_they_claim():
    recs = T.fields(T.forged_chunks())
    assert max(len(s) for _, s, _ in recs) == 12000
    for pos in (1024, 33):
        for which in ("plain", "trim", "random", "hostile"):
            ref = P.forged_reference(P.profile(pos), which)
            assert 0 < ref["longer"] <= ref["profiled"], (pos, which)     # (the trim keeps 36 bases and more)
            assert which == "trim" or ref["longer"] < ref["profiled"], (pos, which)
    # positions past the LDS quality rows (192 at 1,024 positions) hold Quality bytes
    assert P.forged_reference(P.profile(1024))["table"]["qual_n"][192:].sum() > 0
    # the forged file has what the semantics single out
    assert any(len(s) == 0 for _, s, _ in recs) and any(len(q) > len(s) > 0 for _, s, q in recs)
    assert any(0 < len(q) < len(s) for _, s, q in recs) and any(len(q) == 0 < len(s) for _, s, q in recs)
    plain = P.forged_reference(P.profile(33))
    assert plain["no_quality"] > 0 and plain["table"]["len_here"][0] > 0
    # the masks and rows: neither empty nor full, hostile rows of every kind, the clamp matters
    n = len(recs)
    keep = P.bits_of(P.forged_random_mask(), n)
    assert P.forged_random_mask().size == (n + 31) // 32 + 2 and 0 < keep.sum() < n
    t = T.forged_reference(T.ALL)
    assert 0 < t["keep"].sum() < n
    rows = P.forged_hostile_rows()
    L = np.array([len(s) for _, s, _ in recs], np.int64)
    assert (rows[:, 0] > L).any() and (rows[:, 0].astype(np.int64) + rows[:, 1] > L).any() and (rows == 0xFFFFFFFF).all(axis=1).any()
    hostile = P.forged_reference(P.profile(33), "hostile")
    assert 0 < hostile["bases"] < plain["bases"]
    # the chain's mask (test_chain): neither empty nor full
    name, pattern, f, tr = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[2], T.ALL._replace(min_len=60)
    three = Q.reference(name, pattern)["hit"] & F.reference(name, f)["pass"] & T.reference(name, tr)["keep"]
    assert 0 < three.sum() < three.size
