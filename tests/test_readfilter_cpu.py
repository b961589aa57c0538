"""Read filters on the CPU: the reference of the semantics (tests/readfilter_ref.py) against hand-written
records and against the references of the packed reads and the queries, guards that the forged input of
tests/test_gpu_readfilter.py is what it claims (conditions on the input: the reference alone must satisfy
them), ppg_read_filter_check rule by rule (host only: no device), and the ReadFilter -> struct conversion."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(offset, body):
    raw = offset + body
    nl = [i for i, c in enumerate(raw) if c == 10]
    return offset, raw, np.array(nl, np.uint32).reshape(-1, 4)


# ---- 1. the reference against literal records ----
def test_reference_on_hand_written_records():
    c0 = _chunk(b"", b"@r0\nGATTACA\n+\nIIIIII5\n"               # 7 bases, qualities 40 x 6 and 20
                     b"@r1\nACGTNnn\n+\n!!!\n"                   # 3 other; Quality shorter than the Sequence
                     b"@r2\n\n+\nIIII\n")                        # no Sequence, four Quality bytes
    c1 = _chunk(b"@r3\nAC", b"GT\r\n+\n\x05\xff\n"               # starts in the carry; CRLF; bytes below the base, above 127
                            b"@r4\nAAAA\n+\n\n")                 # no Quality: MEAN and LOW hold
    f = F.Filter(0, 4, 7, 1, 33, 30000, 20, 200)
    ref = F.filter_reference((c0, c1), f)
    m = ref["metrics"]
    assert m["length"].tolist() == [7, 7, 0, 5, 4] and m["other"].tolist() == [0, 3, 0, 1, 0]
    assert m["qual_length"].tolist() == [7, 3, 4, 2, 0] and m["low"].tolist() == [0, 3, 0, 1, 0]
    assert m["qual_sum"].tolist() == [73 * 6 + 53, 99, 292, 260, 0]
    assert ref["pass"].all() and ref["passed"] == 5 and ref["failed"].tolist() == [0, 0, 0, 0]
    assert (ref["bases"], ref["other"], ref["qual_bytes"]) == (23, 4, 16)
    assert ref["qual_count"][73] == 10 and ref["qual_count"][255] == 1 and int(ref["qual_count"].sum()) == 16
    assert ref["chunk_passed"].tolist() == [3, 2]
    # each criterion alone: r0 mean (6*40+20)/7 = 37.1, low 0/7; r1 mean 0, low 3/3; r2 mean 40, L = 0;
    # r3 mean (5 + 255 - 66) / 2 = 97, low 1/2; r4 Lq = 0
    got = lambda c: F.filter_reference((c0, c1), f._replace(criteria=c))   # noqa: E731
    assert got(F.LENGTH)["pass"].tolist() == [True, True, False, True, True]
    assert got(F.OTHER)["pass"].tolist() == [True, False, True, True, True]
    assert got(F.MEAN)["pass"].tolist() == [True, False, True, True, True]
    assert got(F.LOW)["pass"].tolist() == [True, False, True, False, True]
    al = got(15)
    assert al["pass"].tolist() == [True, False, False, False, True] and al["failed"].tolist() == [1, 1, 1, 2]
    assert al["mask"].tolist() == [0b10001] and al["chunk_passed"].tolist() == [1, 1]
    # AND with a prior mask: the records' bits become old & pass, the bits past them stay
    for old, new in ((0xFFFFFFFF, 0xFFFFFFF1), (0xFFFFFFEF, 0xFFFFFFE1), (0x0000000E, 0)):
        prior = np.array([old, 0xDEADBEEF], np.uint32)
        assert F.filter_reference((c0, c1), f._replace(criteria=15), prior)["mask"].tolist() == [new, 0xDEADBEEF]
    # equality passes: r3's mean is exactly 97 and half of its bytes are low; r0's mean is 37.142..
    assert F.holds(f._replace(min_mean_milli=37142), m[0])[2] and not F.holds(f._replace(min_mean_milli=37143), m[0])[2]
    assert F.holds(f._replace(min_mean_milli=97000), m[3])[2] and not F.holds(f._replace(min_mean_milli=97001), m[3])[2]
    assert F.holds(f._replace(max_low_milli=500), m[3])[3] and not F.holds(f._replace(max_low_milli=499), m[3])[3]


# ---- 2. the reference against the packed reads' and the queries' references ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_reference_agrees_with_pack_and_query(name):
    ref = F.reference(name, F.FILTERS[0])
    pack, query = R.reference(name), Q.reference(name, None)
    m = ref["metrics"]
    assert ref["records"] == query["records"] == pack["seq_len"].size
    assert np.array_equal(m["length"], pack["seq_len"])
    # other_j = the popcount of the record's bits in the pack's mask plane (whole words: records start on units)
    pop = np.array([bin(int(w)).count("1") for w in pack["mask"]], np.int64)
    per = np.add.reduceat(pop, pack["seq_off"][:-1] // 32)[:m.size] if m.size else pop[:0]
    per = np.where(pack["seq_len"] > 0, per, 0)      # (reduceat of an empty range yields the next word)
    assert np.array_equal(m["other"], per)
    assert ref["other"] == int(m["other"].sum()) == int(query["counts"][4])
    assert ref["bases"] == int(m["length"].sum()) == query["bases"]
    assert ref["qual_bytes"] == int(m["qual_length"].sum()) == int(ref["qual_count"].sum())
    assert int((np.arange(256) * ref["qual_count"]).sum()) == int(m["qual_sum"].sum())
    assert ref["passed"] == ref["records"] and int(ref["chunk_passed"].sum()) == ref["passed"]
    for f in F.FILTERS[1:]:
        r = F.reference(name, f)
        assert int(r["chunk_passed"].sum()) == r["passed"] == int(r["pass"].sum())
        assert np.array_equal(r["metrics"], m)


# ---- 3. the forged input is what it claims ----
def test_forged_input_guard():
    chunks = F.forged_chunks()
    ref = F.forged_reference(F.FILTERS[0])
    m = ref["metrics"]
    # every record came back once, in order
    assert [(int(a), int(b)) for a, b in zip(m["length"], m["qual_length"])] == [(L, lq) for L, lq, _, _ in F.forged_records()]
    assert (len(F.forged_text()), len(chunks), sum(len(off) > 0 for off, _, _ in chunks), ref["records"]) == (389861, 24, 23, 81)
    classes = set(zip(m["length"].tolist(), m["qual_length"].tolist()))
    for L in (0, 1, 31, 32, 33, 63, 64, 65, 150, 2047, 2048, 2049, 8191, 8192, 8193, 12000):
        assert {(L, L), (L, max(L - 1, 0)), (L, L + 1), (L, L + 40), (L, 0)} <= classes, L
    assert (0, 70) in classes
    # a Sequence that straddles the carry / body seam, and a Quality that does
    seam_s = sum(int(n1 + 1 < len(off) < n2) for off, _, d in chunks for n1, n2, _, _ in d.astype(np.int64).tolist())
    seam_q = sum(int(n3 + 1 < len(off) < n4) for off, _, d in chunks for _, _, n3, n4 in d.astype(np.int64).tolist())
    assert seam_s > 0 and seam_q > 0
    # the alphabets: N, lower case and '.' in the Sequences; Quality bytes below the base and above 127
    seq = b"".join(s for ch in Q.sequences(chunks) for s in ch)
    assert all(c in seq for c in b"ACGTNacgtn.") and ref["other"] > 0
    qc = ref["qual_count"]
    assert qc[10] == 0 and qc[64] == 0 and qc[0] == 0 and (np.delete(qc, [0, 10, 64]) > 0).all()
    assert int(qc[:33].sum()) > 0 and int(qc[128:].sum()) > 0


def test_forged_thresholds_have_a_record_on_and_one_beyond():
    m = F.forged_reference(F.FILTERS[0])["metrics"]
    f = F.FILTERS[-1]
    by = {(int(r["length"]), int(r["qual_length"])): r for r in m}
    # LENGTH: 32 and 8192 pass, 31 and 8193 fail
    assert f.min_len == 32 and f.max_len == 8192
    assert F.holds(f, by[(32, 0)])[0] and F.holds(f, by[(8192, 0)])[0]
    assert not F.holds(f, by[(31, 0)])[0] and not F.holds(f, by[(8193, 0)])[0]
    # OTHER: 3 passes, 4 fails
    on, off = by[(64, 64)], by[(65, 65)]
    assert int(on["other"]) == f.max_other and int(off["other"]) == f.max_other + 1
    # MEAN: equality in the integer inequality passes, one unit of qsum less fails
    on, off = by[(1, 1)], by[(0, 1)]
    assert 1000 * (int(on["qual_sum"]) - f.qual_base) == f.min_mean_milli and int(off["qual_sum"]) == int(on["qual_sum"]) - 1
    assert F.holds(f, on)[2] and not F.holds(f, off)[2]
    # LOW: equality passes, one low byte more than the bound allows fails
    on, off = by[(0, 40)], by[(32, 32)]
    assert 1000 * int(on["low"]) == f.max_low_milli * 40 and F.holds(f, on)[3]
    assert int(off["low"]) == f.max_low_milli * 32 // 1000 + 1 and not F.holds(f, off)[3]
    # every filter passes some records and fails some, but the one without criteria, which passes all
    for flt in F.FILTERS:
        r = F.forged_reference(flt)
        if flt.criteria == 0:
            assert r["passed"] == r["records"] == 81
        else:
            assert 0 < r["passed"] < r["records"], flt
    assert F.forged_reference(f)["failed"].tolist() == [F.forged_reference(g)["failed"][c] for c, g in enumerate(F.FILTERS[1:5])]


# ---- 4. ppg_read_filter_check, host only ----
def _check(**kw):
    good = dict(criteria=15, min_len=0, max_len=-1, max_other=0, qual_base=33, min_mean_milli=0, low_q=0, max_low_milli=0)
    good.update(kw)
    f = _lib.PpgReadFilter(*[good[k] for k, _ in _lib.PpgReadFilter._fields_])
    return _lib.lib.ppg_read_filter_check(C.byref(f))


def test_read_filter_check_rules():
    OK, E = 0, _lib.PPG_ARG_ERROR
    assert _lib.lib.ppg_read_filter_check(None) == E
    assert _check() == OK
    assert _check(criteria=0x10F) == OK and _check(criteria=0x10) == E and _check(criteria=0x200) == E and _check(criteria=-1) == E
    assert _check(min_len=0) == OK and _check(min_len=-1) == E
    assert _check(max_len=-1) == OK and _check(max_len=-2) == E
    assert _check(min_len=5, max_len=5) == OK and _check(min_len=5, max_len=4) == E and _check(min_len=5, max_len=0) == E
    assert _check(max_other=0) == OK and _check(max_other=-1) == E
    assert _check(criteria=13, max_other=-1) == OK          # OTHER is not set: its bound is not looked at
    assert _check(qual_base=0) == OK and _check(qual_base=255) == OK and _check(qual_base=-1) == E and _check(qual_base=256) == E
    assert _check(low_q=0) == OK and _check(low_q=-1) == E
    assert _check(qual_base=33, low_q=223) == OK and _check(qual_base=33, low_q=224) == E
    assert _check(max_low_milli=0) == OK and _check(max_low_milli=1000) == OK
    assert _check(max_low_milli=-1) == E and _check(max_low_milli=1001) == E
    assert _check(min_mean_milli=255000) == OK and _check(min_mean_milli=-255000) == OK
    assert _check(min_mean_milli=255001) == E and _check(min_mean_milli=-255001) == E
    # the filters the tests share are valid
    for f in F.FILTERS:
        assert _lib.lib.ppg_read_filter_check(C.byref(_lib.PpgReadFilter(*f))) == OK


def test_null_handles_and_bad_filters_without_a_device():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    good = _lib.PpgReadFilter(*F.FILTERS[-1])
    res = _lib.PpgReadFilterResult()
    assert C.sizeof(_lib.PpgReadFilter) == 64 and C.sizeof(res) == 8 * 265
    assert lib.ppg_shard_filter_reads(None, C.byref(good), None, 0, None, 0, None, C.byref(res)) == E
    assert lib.ppg_shard_set_readfilter(None, C.byref(good), None, 0, None, 0) == E
    assert lib.ppg_shard_readfilter_ready(None, None, C.byref(res)) == E
    assert lib.ppg_cursor_filter_result(None, C.byref(res)) == E
    h = C.c_void_p()
    bad = _lib.PpgReadFilter(*F.FILTERS[-1]._replace(min_len=-1))
    assert lib.ppg_cursor_open_filter(None, None, b"x", 0, 0, 0, 1, None, 0, C.byref(bad), C.byref(h)) == E
    b = pp.BatchedFASTQ.__new__(pp.BatchedFASTQ)      # a rank of a job: the counts are single process
    b.world, b.rank = 2, 0
    with pytest.raises(ValueError):
        b.CountPassing(pp.ReadFilter())


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    for name in ("ppg_read_filter_check", "ppg_shard_filter_reads", "ppg_shard_set_readfilter", "ppg_shard_readfilter_ready",
                 "ppg_cursor_open_filter", "ppg_cursor_filter_result"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert "} ppg_read_filter;" in h and "} ppg_read_filter_result;" in h
    assert h.index("} ppg_read_filter_result;") < h.index("typedef struct ppg_cursor ppg_cursor;")
    assert "struct PpgReadFilter" in cs and "struct PpgReadFilterResult" in cs
    with open(os.path.join(ROOT, "interop", "GpuBatchedFASTQ.cs")) as f:
        assert "Where(string pattern, PpgReadFilter filter)" in f.read()


# ---- 5. ReadFilter -> ppg_read_filter ----
def _fields(s):
    return tuple(getattr(s, k) for k, _ in _lib.PpgReadFilter._fields_)


def test_read_filter_struct_conversion():
    assert _fields(pp.ReadFilter().struct()) == (0, 0, -1, 0, 33, 0, 0, 0)
    f = pp.ReadFilter(min_length=32, max_length=8192, max_n=3, min_mean_quality=40, low_quality=20, max_low_fraction=0.25)
    assert _fields(f.struct()) == tuple(F.FILTERS[-1])
    assert f.struct(and_mask=True).criteria == 15 | F.AND_MASK and f.struct().criteria == 15
    # one criterion each
    assert pp.ReadFilter(min_length=1).struct().criteria == F.LENGTH
    assert pp.ReadFilter(max_length=0).struct().criteria == F.LENGTH
    assert pp.ReadFilter(max_n=0).struct().criteria == F.OTHER
    assert pp.ReadFilter(min_mean_quality=0).struct().criteria == F.MEAN
    assert pp.ReadFilter(low_quality=2, max_low_fraction=1).struct().criteria == F.LOW
    # milli values by round(1000 * x)
    assert pp.ReadFilter(min_mean_quality=20.0004).struct().min_mean_milli == 20000
    assert pp.ReadFilter(min_mean_quality=20.0006).struct().min_mean_milli == 20001
    assert pp.ReadFilter(min_mean_quality=-1.5).struct().min_mean_milli == -1500
    assert pp.ReadFilter(low_quality=10, max_low_fraction=0.1234).struct().max_low_milli == 123
    assert pp.ReadFilter(low_quality=10, max_low_fraction=0.1236).struct().max_low_milli == 124
    assert pp.ReadFilter(quality_base=64).struct().qual_base == 64
    for kw in (dict(low_quality=10), dict(max_low_fraction=0.5)):
        with pytest.raises(ValueError):
            pp.ReadFilter(**kw)
    for kw in (dict(min_length=-1), dict(min_length=5, max_length=4), dict(max_n=-1), dict(quality_base=300),
               dict(low_quality=10, max_low_fraction=1.5), dict(min_mean_quality=300)):
        with pytest.raises(ValueError):
            pp.ReadFilter(**kw).struct()
    for attr in ("filter_reads", "set_readfilter", "readfilter"):
        assert hasattr(pp.Shard, attr), attr
    assert hasattr(pp, "ReadFilterResult") and hasattr(pp.BatchedFASTQ, "CountPassing") and hasattr(pp.BatchedFASTQ, "QualityCounts")
    assert pp.ReadFilterResult.METRICS_DTYPE == F.METRICS_DTYPE and pp.ReadFilterResult.METRICS_DTYPE.itemsize == 24
