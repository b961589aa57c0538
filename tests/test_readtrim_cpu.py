"""Read trimming on the CPU: the reference of the semantics (tests/readtrim_ref.py) against hand-written
records with their windows spelled out, guards that the forged input of tests/test_gpu_readtrim.py holds
every property it claims to plant (conditions on the input: the reference alone must satisfy them),
ppg_read_trim_check rule by rule (host only: no device), the struct sizes, and the ReadTrim -> struct
conversion."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import seqpack_ref as R
import readfilter_ref as F
import readtrim_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(offset, body):
    raw = offset + body
    nl = [i for i, c in enumerate(raw) if c == 10]
    return offset, raw, np.array(nl, np.uint32).reshape(-1, 4)


def _win(t, s, q):
    return T.window_of(t, s, q)[:2]


# ---- 1. the reference against literal records ('I' is quality 40, '2' 17, '#' 2; the cuts are at 20) ----
def test_reference_on_hand_written_records():
    s10 = b"ACGTACGTAC"
    assert _win(T.NONE, s10, b"##########") == (0, 10)
    assert _win(T.LEAD, s10, b"##IIIIIIII") == (2, 8)
    assert _win(T.LEAD, s10, b"##########") == (0, 0)            # lead = e0: nothing left, start 0
    assert _win(T.TRAIL, s10, b"IIIIIII###") == (0, 7)
    assert _win(T.TRAIL, s10, b"##########") == (0, 0)           # trail = b0
    assert _win(T.TRAIL, s10, b"IIIII") == (0, 5)                # a base without a Quality byte is quality "below 0"
    assert _win(T.TRAIL, s10, b"IIIIIIIIIIIIII") == (0, 10)      # Quality bytes past the Sequence are no bases
    assert _win(T.WIN, s10, b"IIII2222II") == (0, 4)             # 73 + 3 * 50 = 223 >= 212 passes, 4 * 50 fails
    assert _win(T.WIN, s10, b"IIIIIIIII#") == (0, 10)            # the last full window holds three good bases
    assert _win(T.WIN, b"ACG", b"###") == (0, 3)                 # no full window
    assert _win(T.FIXED, s10, b"IIIIIIIIII") == (0, 0)           # b0 = 3, e0 = max(3, 3)
    assert _win(T.FIXED, s10 + s10, b"I" * 20) == (3, 10)
    assert _win(T.FIXED, b"AC", b"II") == (0, 0)                 # b0 = min(3, 2), e0 = max(2, -5)
    assert _win(T.ADAPT, b"CTCTC" + T.TRUSEQ, b"I" * 38) == (0, 5)
    assert _win(T.ADAPT, b"CTCTCTCTCT" + T.TRUSEQ[:5], b"") == (0, 10)
    assert _win(T.ADAPT, b"CTCTCTCTCT" + T.TRUSEQ[:4], b"") == (0, 14)
    assert _win(T.ADAPT, T.TRUSEQ, b"") == (0, 0)                # adapter dimer: cut at 0
    # everything at once: b0 = 3, e0 = 53; lead 5; trail 53; no failing window; the adapter at 20, its 33 bases end at e0
    s = b"CT" * 10 + T.TRUSEQ + b"CTCTCTC"
    q = b"#" * 5 + b"I" * 55
    assert T.window_of(T.ALL, s, q) == (5, 15, (True, True, False, False, True))
    # the independent cuts: the window is judged on the untrimmed read, also where the adapter has cut before it
    q = b"I" * 30 + b"2222" + b"I" * 26
    assert _win(T.ALL, s, q) == (3, 17) and _win(T.ALL._replace(ops=T.WINDOW), s, q) == (3, 27)
    # through trim_reference: rows, keep, totals, chunk_kept, and a chunk that starts in the offset carry
    c0 = _chunk(b"", b"@r0\n" + s10 + b"\n+\nIIIIIII###\n" + b"@r1\n\n+\nIIII\n")
    c1 = _chunk(b"@r2\nAC", b"GTACGTAC\n+\n##IIIIIIII\n")
    t = T.Trim(T.LEADING | T.TRAILING, 0, 0, 33, 20, 20, 4, 20, 5, 100, 8, T.TRUSEQ)
    ref = T.trim_reference((c0, c1), t)
    assert ref["rows"].tolist() == [[0, 7], [0, 0], [2, 8]] and ref["keep"].tolist() == [False, False, True]
    assert (ref["records"], ref["kept"], ref["trimmed"]) == (3, 1, 2) and ref["cut"].tolist() == [0, 1, 1, 0, 0]
    assert (ref["bases"], ref["bases_window"], ref["bases_kept"]) == (20, 15, 8) and ref["chunk_kept"].tolist() == [0, 1]
    assert ref["mask"].tolist() == [0b100]
    prior = np.array([0xFFFFFFFF, 0x12345678], np.uint32)
    assert T.trim_reference((c0, c1), t, prior)["mask"].tolist() == [0xFFFFFFFC, 0x12345678]
    assert T.slices_of(ref["rows"][2], s10, b"##IIIIIIII") == (b"GTACGTAC", b"IIIIIIII")
    assert T.slices_of((2, 8), s10, b"##III") == (b"GTACGTAC", b"III")


# ---- 2. the forged input is what it claims ----
def _planted():
    """{tag: (sequence, quality)} of the forged text's planted records, located in the oracle's chunks."""
    recs = T.forged_records()
    got = T.fields(T.forged_chunks())
    assert len(got) == len(recs)
    for (tag, _, s, q), (_, gs, gq) in zip(recs, got):
        assert (s, q) == (gs, gq), tag           # the oracle parses the text into the records it was made of
    return {tag: (s, q) for tag, _, s, q in recs if tag[0] != "class"}


def test_forged_input_holds_what_it_plants():
    recs, P = T.forged_records(), _planted()
    classes = sorted((t[1], t[2]) for t, *_ in recs if t[0] == "class")
    assert classes == sorted(T.forged_classes()) and {c[0] for c in classes} == set(F.FORGED_L)
    assert {0, 1, 31, 32, 33, 63, 64, 65, 150, 2047, 2048, 2049, 8191, 8192, 8193, 12000} == set(T.FORGED_L)
    for L in T.FORGED_L:
        assert {lq for l, lq in classes if l == L} == {L, max(L - 1, 0), L + 40, 0}
    chunks = T.forged_chunks()
    assert len(chunks) > 5 and sum(bool(c[0]) for c in chunks) > len(chunks) // 2
    # a record that begins in the offset carry and goes on in the body (the carry seam), in several chunks
    assert sum(1 for off, _, d in chunks if len(off) and len(d) and int(d[0][3]) >= len(off)) >= 3
    win = lambda t, tag: _win(t, *P[tag])                        # noqa: E731
    # quality edges
    for x in T.SEAMS:
        L = x + 40
        assert win(T.TRAIL, ("trail", x)) == (0, x + 1) and win(T.LEAD, ("lead", x)) == (x, L - x)
    assert set(T.SEAMS) == {30, 31, 32, 2047, 2048, 8191, 8192}
    assert win(T.TRAIL, ("all_low",)) == (0, 0) == win(T.LEAD, ("all_low",))
    assert win(T.ALL._replace(head=0, tail=0, ops=7), ("no_low",)) == (0, 100)
    s, q = P[("past_lq",)]
    assert len(s) == 100 and len(q) == 60 and win(T.TRAIL, ("past_lq",)) == (0, 0) == win(T.LEAD, ("past_lq",))
    text = T.forged_text()
    after = text[text.index(b"\n" + q + b"\n") + len(q) + 1:][:45]
    assert after[2:].startswith(b"r") and sum(c >= T.QUAL_BASE + T.CUT_Q for c in after) >= 40   # what a read past Lq would find
    # window
    assert set(T.WIN_AT) == {28, 29, 31, 32, 2046, 8190}
    for x in T.WIN_AT:
        assert win(T.WIN, ("win", x)) == (0, x)
        assert T.win_of(P[("win", x)][1], 0, x + 3, T.W, 53) == x + 3           # ... and no window before it fails
    q = P[("win_on",)][1]
    assert sum(q[10:14]) == T.W * 53 and win(T.WIN, ("win_on",)) == (0, 50)
    q = P[("win_below",)][1]
    assert sum(q[10:14]) == T.W * 53 - 1 and win(T.WIN, ("win_below",)) == (0, 10)
    s, q = P[("win_tail",)]
    assert win(T.WIN, ("win_tail",)) == (0, 50) and sum(q[47:50]) + 0 < T.W * 53   # a window padded with qb = 0 would fail
    assert len(P[("win_short",)][0]) == T.W - 1 and win(T.WIN, ("win_short",)) == (0, T.W - 1)
    assert T.win_of(P[("win_short",)][1] + b"#", 0, T.W, T.W, 53) == 0              # one base more and it is cut
    # adapter
    assert len(T.TRUSEQ) == 33 and (T.MIN_OVERLAP, T.MAX_ERR_MILLI) == (5, 100) and set(T.ADAPT_AT) == {0, 20, 31, 32, 2040, 8180}
    for p in T.ADAPT_AT:
        assert win(T.ADAPT, ("adapt", p)) == (0, p)
    mism = lambda tag, p, n: sum(a != b for a, b in zip(P[tag][0][p:p + n], T.TRUSEQ))   # noqa: E731
    assert mism(("adapt_3mis",), 10, 33) == 3 and win(T.ADAPT, ("adapt_3mis",)) == (0, 10)
    assert mism(("adapt_4mis",), 10, 33) == 4 and win(T.ADAPT, ("adapt_4mis",)) == (0, 48)
    assert win(T.ADAPT, ("adapt_ov5",)) == (0, 50) and win(T.ADAPT, ("adapt_ov4",)) == (0, 54)
    assert mism(("adapt_ov10_1mis",), 50, 10) == 1 and win(T.ADAPT, ("adapt_ov10_1mis",)) == (0, 50)
    assert mism(("adapt_ov10_2mis",), 50, 10) == 2 and win(T.ADAPT, ("adapt_ov10_2mis",)) == (0, 60)
    s = P[("adapt_two",)][0]
    assert s[10:43] == s[53:86] == T.TRUSEQ and win(T.ADAPT, ("adapt_two",)) == (0, 10)
    s = P[("adapt_n",)][0]
    assert win(T.ADAPT, ("adapt_n",)) == (0, 48) and mism(("adapt_n",), 10, 33) == 4 == s[10:43].count(b"N")
    assert win(T.ADAPT, ("adapt_before_head",)) == (0, 1) and win(T.ADAPT_FIXED, ("adapt_before_head",)) == (3, 44)
    assert win(T.ADAPT, ("adapt_in_tail",)) == (0, 50) and win(T.ADAPT_FIXED, ("adapt_in_tail",)) == (3, 46)
    s = P[("adapt_cut_by_e0",)][0]
    assert len(s) - T.TAIL == 56 and win(T.ADAPT_FIXED, ("adapt_cut_by_e0",)) == (3, 47)   # ov(50) = 6
    assert win(T.ADAPT, ("adapt_cut_by_e0",)) == (0, 63)                                  # ov(50) = 13 with 7 mismatches
    # every setting keeps some records and drops some, but the one that does nothing
    for t in T.TRIMS:
        r = T.forged_reference(t)
        assert r["records"] == len(recs)
        if t == T.NONE:
            assert r["kept"] == r["records"] and r["trimmed"] == 0 and not r["cut"].any()
        else:
            assert 0 < r["kept"] < r["records"], t
    r = T.forged_reference(T.ALL)
    assert all(r["cut"] > 0) and r["bases_kept"] < r["bases_window"] < r["bases"]


# ---- 3. ppg_read_trim_check, host only ----
def _check(**kw):
    good = dict(ops=15, head=0, tail=0, qual_base=33, lead_q=20, trail_q=20, win_size=4, win_q=20, min_overlap=5,
                max_err_milli=100, min_len=0, adapter=T.TRUSEQ)
    good.update(kw)
    return _lib.lib.ppg_read_trim_check(C.byref(T.struct_of(T.Trim(**good))))


def test_read_trim_check_rules():
    OK, E = 0, _lib.PPG_ARG_ERROR
    assert _lib.lib.ppg_read_trim_check(None) == E
    assert _check() == OK
    assert _check(ops=0x10F) == OK and _check(ops=0x10) == E and _check(ops=0x200) == E and _check(ops=-1) == E
    for k in ("head", "tail", "min_len"):
        assert _check(**{k: 0}) == OK and _check(**{k: 1 << 40}) == OK and _check(**{k: -1}) == E
    q1 = dict(lead_q=1, trail_q=1, win_q=1)                                          # (qual_base + q <= 256 holds beside)
    assert _check(qual_base=0) == OK and _check(qual_base=255, **q1) == OK
    assert _check(qual_base=-1) == E and _check(qual_base=256, ops=0) == E and _check(qual_base=255, ops=0) == OK
    for bit, k in ((1, "lead_q"), (2, "trail_q"), (4, "win_q")):
        assert _check(**{k: 0}) == OK and _check(**{k: -1}) == E
        assert _check(**{k: 223}) == OK and _check(**{k: 224}) == E                 # qual_base + q <= 256
        assert _check(qual_base=0, **{k: 256}) == OK and _check(qual_base=0, **{k: 257}) == E
        assert _check(ops=15 & ~bit, **{k: -1}) == OK                                # not enabled: not looked at
    assert _check(win_size=1) == OK and _check(win_size=32) == OK and _check(win_size=0) == E and _check(win_size=33) == E
    assert _check(ops=11, win_size=0) == OK
    assert _check(adapter=b"A", min_overlap=1) == OK and _check(adapter=b"A" * 64) == OK
    assert _check(adapter=b"", min_overlap=1) == E and _check(ops=7, adapter=b"", min_overlap=0) == OK
    s = T.struct_of(T.Trim(15, 0, 0, 33, 20, 20, 4, 20, 5, 100, 0, T.TRUSEQ))
    s.adapter_len = 65
    assert _lib.lib.ppg_read_trim_check(C.byref(s)) == E
    s.adapter_len = -1
    assert _lib.lib.ppg_read_trim_check(C.byref(s)) == E
    assert _check(adapter=b"ACGT\nACGT") == E and _check(ops=7, adapter=b"ACGT\nACGT") == OK
    s = T.struct_of(T.Trim(15, 0, 0, 33, 20, 20, 4, 20, 5, 100, 0, b"ACGTACGT"))
    s.adapter[20] = 10                                                              # past adapter_len: no adapter byte
    assert _lib.lib.ppg_read_trim_check(C.byref(s)) == OK
    assert _check(min_overlap=1) == OK and _check(min_overlap=33) == OK and _check(min_overlap=0) == E and _check(min_overlap=34) == E
    assert _check(max_err_milli=0) == OK and _check(max_err_milli=1000) == OK
    assert _check(max_err_milli=-1) == E and _check(max_err_milli=1001) == E
    assert _check(ops=7, min_overlap=0, max_err_milli=-1) == OK
    for t in T.TRIMS:                                                               # the trims the tests share are valid
        assert _lib.lib.ppg_read_trim_check(C.byref(T.struct_of(t))) == OK


def test_struct_sizes_null_handles_and_bad_trims_without_a_device():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    good = T.struct_of(T.ALL)
    res = _lib.PpgReadTrimResult()
    assert C.sizeof(_lib.PpgReadTrim) == 160 and C.sizeof(res) == 88
    assert _lib.PpgReadTrim.adapter.offset == 96 and _lib.PpgReadTrimResult.cut.offset == 24
    assert lib.ppg_shard_trim_reads(None, C.byref(good), None, 0, None, 0, None, C.byref(res)) == E
    assert lib.ppg_shard_set_readtrim(None, C.byref(good), None, 0, None, 0) == E
    assert lib.ppg_shard_readtrim_ready(None, None, C.byref(res)) == E
    assert lib.ppg_cursor_trim_result(None, C.byref(res)) == E
    p = C.c_void_p()
    assert lib.ppg_cursor_selected_trim(None, C.byref(p)) == E
    h = C.c_void_p()
    bad = T.struct_of(T.ALL._replace(win_size=33))
    assert lib.ppg_cursor_open_trim(None, None, b"x", 0, 0, 0, 1, None, 0, None, C.byref(bad), C.byref(h)) == E
    assert lib.ppg_cursor_open_trim(None, None, b"x", 0, 0, 0, 1, None, 0, None, C.byref(good), C.byref(h)) == E   # no ctx
    b = pp.BatchedFASTQ.__new__(pp.BatchedFASTQ)      # a rank of a job: the counts are single process
    b.world, b.rank = 2, 0
    with pytest.raises(ValueError):
        b.CountTrimmed(pp.ReadTrim())


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    for name in ("ppg_read_trim_check", "ppg_shard_trim_reads", "ppg_shard_set_readtrim", "ppg_shard_readtrim_ready",
                 "ppg_cursor_open_trim", "ppg_cursor_selected_trim", "ppg_cursor_trim_result"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert hasattr(_lib.lib, "ppgx_readtrim_times")
    assert "} ppg_read_trim;" in h and "} ppg_read_trim_result;" in h
    assert h.index("read filters:") < h.index("read trimming:") < h.index("typedef struct ppg_cursor ppg_cursor;")
    assert "keys, pack, query, filter, trim, select" in h and "keys, pack, query, filter, select" not in h
    assert "struct PpgReadTrim " in cs and "struct PpgReadTrimResult" in cs and "fixed byte AdapterBytes[64]" in cs
    with open(os.path.join(ROOT, "interop", "GpuBatchedFASTQ.cs")) as f:
        src = f.read()
    assert "Where(string pattern, PpgReadFilter? filter, PpgReadTrim trim)" in src
    assert "TrimmedSequence" in src and "TrimmedQuality" in src


# ---- 4. ReadTrim -> ppg_read_trim ----
def _fields(s):
    return tuple(getattr(s, k) for k, _ in _lib.PpgReadTrim._fields_[:12]) + (bytes(s.adapter[:s.adapter_len]),)


def test_read_trim_struct_conversion():
    assert _fields(pp.ReadTrim().struct()) == (0, 0, 0, 33, 0, 0, 0, 0, 0, 0, 0, 0, b"")
    t = pp.ReadTrim(head=3, tail=7, leading_quality=20, trailing_quality=20, window=(4, 20), adapter=T.TRUSEQ,
                    min_overlap=5, max_error_rate=0.1, min_length=36)
    assert _fields(t.struct()) == tuple(T.ALL[:11]) + (33, T.TRUSEQ)
    assert bytes(t.struct().adapter[33:]) == bytes(31)
    assert t.struct(and_mask=True).ops == 15 | T.AND_MASK and t.struct().ops == 15
    # one cut each
    assert pp.ReadTrim(leading_quality=0).struct().ops == T.LEADING
    assert pp.ReadTrim(trailing_quality=3).struct().ops == T.TRAILING
    assert pp.ReadTrim(window=(1, 0)).struct().ops == T.WINDOW
    assert pp.ReadTrim(adapter="ACGT").struct().ops == T.ADAPTER and pp.ReadTrim(adapter="ACGT").struct().min_overlap == 3
    assert pp.ReadTrim(head=1, tail=2, min_length=9).struct().ops == 0
    # the rate by round(1000 * x)
    assert pp.ReadTrim(adapter=b"ACGT", max_error_rate=0.1234).struct().max_err_milli == 123
    assert pp.ReadTrim(adapter=b"ACGT", max_error_rate=0.1236).struct().max_err_milli == 124
    assert pp.ReadTrim(adapter=b"ACGT", max_error_rate=1).struct().max_err_milli == 1000
    assert pp.ReadTrim(quality_base=64).struct().qual_base == 64
    with pytest.raises(ValueError):
        pp.ReadTrim(window=(4,))
    for kw in (dict(head=-1), dict(tail=-1), dict(min_length=-1), dict(quality_base=300), dict(leading_quality=-1),
               dict(trailing_quality=250), dict(window=(0, 20)), dict(window=(33, 20)), dict(window=(4, -1)),
               dict(adapter=b""), dict(adapter=b"A" * 65), dict(adapter=b"AC\nGT"), dict(adapter=b"AC", min_overlap=3),
               dict(adapter=b"ACGT", max_error_rate=1.5), dict(adapter=b"ACGT", min_overlap=0)):
        with pytest.raises(ValueError):
            pp.ReadTrim(**kw).struct()
    for attr in ("trim_reads", "set_readtrim", "readtrim"):
        assert hasattr(pp.Shard, attr), attr
    assert hasattr(pp, "ReadTrimResult") and hasattr(pp.BatchedFASTQ, "CountTrimmed") and hasattr(pp.SelectedRecords, "trimmed")
    assert pp.ReadTrimResult.CUTS == T.CUTS


# ---- 5. against the read filters' reference: a trim that cuts nothing keeps by length ----
@pytest.mark.parametrize("name", [n for n in R.ALL_INPUTS if n != R.SYNTH])
def test_no_cut_keeps_what_the_length_filter_passes(name):
    chunks = R.oracle_chunks(name)
    for x in (0, 36, 101, 151):
        t = T.NONE._replace(min_len=x)
        ref = T.trim_reference(chunks, t)
        f = F.filter_reference(chunks, F.Filter(F.LENGTH, x, -1, 0, 33, 0, 0, 0))
        assert np.array_equal(ref["keep"], f["pass"]) and ref["kept"] == f["passed"]
        assert np.array_equal(ref["chunk_kept"], f["chunk_passed"]) and np.array_equal(ref["mask"], f["mask"])
        assert ref["trimmed"] == 0 and ref["bases"] == ref["bases_window"] == f["bases"]
        assert np.array_equal(ref["rows"][:, 1], f["metrics"]["length"]) and not ref["rows"][:, 0].any()
