"""The pair overlap without a GPU: the brute-force reference of the semantics (tests/pairoverlap_ref.py) against
a second, vectorised restatement and against hand-worked pairs; the forge is what it claims; the struct check
through the host-only path of the library; the windows rule against literals; the ABI's presence."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import pairoverlap_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. a second restatement: the whole mismatch matrix, its diagonals summed at once ----
def overlap_matrix(s1, s2, p):
    L1, L2 = len(s1), len(s2)
    if L1 > V.MAX_LEN or L2 > V.MAX_LEN:
        return "long"
    if L1 == 0 or L2 == 0:
        return None
    c1, n1 = V.codes(s1)
    c2, n2 = V.codes(s2)
    cR, nR = 3 - c2[::-1], n2[::-1]
    bad = n1[:, None] | nR[None, :] | (c1[:, None] != cR[None, :])    # read-1 position i against R position t
    i, t = np.nonzero(bad)
    mis = np.bincount(i - t + L2 - 1, minlength=L1 + L2 - 1)          # diagonal d = i - t at index d + L2 - 1
    d = np.arange(-(L2 - 1), L1)
    ov = np.minimum(L1, L2 + d) - np.maximum(0, d)
    ok = (ov >= p.min_overlap) & (mis <= p.max_diff) & (1000 * mis <= p.max_err_milli * ov)
    if not ok.any():
        return None
    rank = np.where(d >= 0, d, L1 - d - 1)                            # 0 .. L1 - 1, then -1 .. -(L2 - 1)
    k = int(np.argmin(np.where(ok, rank, L1 + L2)))
    return int(d[k]), int(ov[k]), int(mis[k]), int(L2 + d[k])


@pytest.mark.parametrize("pname", sorted(V.PARAM_SETS))
def test_two_restatements_agree_on_the_forge(pname):
    p = V.PARAM_SETS[pname]
    for k, pair in enumerate(V.forge()):
        assert V.overlap_one(pair.r1, pair.r2, p) == overlap_matrix(pair.r1, pair.r2, p), (k, pair.cat, pair.note)


def test_candidate_order():
    assert V.candidates(3, 4) == [0, 1, 2, -1, -2, -3]
    assert V.candidates(0, 3) == [-1, -2] and V.candidates(3, 0) == [1, 2] and V.candidates(0, 0) == []


# ---- 2. pairs worked by hand ----
def test_hand_worked_pairs():
    P = V.Params
    # a 10-base fragment AACCGGTTAC read 6 bases from both ends: R = GGTTAC, the last two bases of read 1 are its
    # first two.  d = 0 .. 3 have 6, 5, 4 and 2 mismatches.
    assert V.revcomp(b"GTAACC") == b"GGTTAC"
    assert V.overlap_one(b"AACCGG", b"GTAACC", P(2, 0, 0)) == (4, 2, 0, 10)
    assert [V.mis_at(b"AACCGG", b"GTAACC", d) for d in range(5)] == [(6, 6), (5, 5), (4, 4), (3, 2), (2, 0)]
    # an N is a mismatch on either side: one in two passes a rate of 1000 and of 500, not of 499; then the order
    # goes on to the negative offsets, where AAC faces TAC at d = -3
    assert V.overlap_one(b"AACCNG", b"GTAACC", P(2, 1, 1000)) == (4, 2, 1, 10)
    assert V.overlap_one(b"AACCNG", b"GTAACC", P(2, 1, 500)) == (4, 2, 1, 10)
    assert V.overlap_one(b"AACCNG", b"GTAACC", P(2, 1, 499)) == (-3, 3, 1, 3)
    assert V.overlap_one(b"AACCGG", b"GTANCC", P(2, 0, 0)) == (4, 2, 0, 10)      # read 2's N faces nothing at d = 4
    assert V.overlap_one(b"AACCGG", b"GTAANC", P(2, 0, 1000)) is None            # ... here it faces read 1's G
    # read-through: a 5-base fragment ACGTT in 8-base reads; R = GGGACGTT, read 1 starts 3 bases into it
    assert V.overlap_one(b"ACGTTGGG", b"AACGTCCC", P(5, 0, 0)) == (-3, 5, 0, 5)
    assert V.overlap_one(b"ACGTTGGG", b"AACGTCCC", P(6, 0, 0)) is None
    # poly-A against poly-T: every offset is accepted, d = 0 is tried first
    assert V.overlap_one(b"A" * 40, b"T" * 50, P(30, 5, 200)) == (0, 40, 0, 50)
    assert V.overlap_one(b"A" * 40, b"T" * 50, P(41, 5, 200)) is None
    # lengths: 1024 is analysed, 1025 is long; an empty read has no overlap
    assert V.overlap_one(b"A" * 1025, b"T" * 40, P(1, 0, 0)) == "long" and V.overlap_one(b"", b"T" * 40, P(1, 0, 0)) is None
    assert V.overlap_one(b"A" * 1024, b"T" * 1024, P(1024, 0, 0)) == (0, 1024, 0, 1024)
    # the whole call on three pairs, with a map: rows, mask, totals, histogram, windows
    set1, set2 = [b"AACCGG", b"ACGTTCAC", b"AAAAAA"], [b"GGGGGG", b"AACGTGAG", b"GTAACC"]
    ref = V.overlap_reference(set1, set2, P(2, 0, 0), rec1=[0, 1, 2, 5], rec2=[2, 1, 0, 0],
                              windows1=[(0, 6), (1, 0xFFFFFFFF), (2, 2)], windows2=[(0, 6), (4, 4), (0, 6)])
    assert ref["rows"].tolist() == [[4, 2, 0, 10], [-3, 5, 0, 5], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert ref["mask"].tolist() == [0b0011] and ref["found_bits"].tolist() == [True, True, False, False]
    assert [ref[k] for k in V.TOTALS] == [4, 1, 0, 3, 2, 1, 1, 7, 0] and ref["clipped"] == (3, 3)
    assert ref["hist"][5] == ref["hist"][10] == 1 and ref["hist"].sum() == 2
    assert ref["windows1"].tolist() == [[0, 6], [1, 4], [2, 2]] and ref["windows2"].tolist() == [[0, 6], [4, 1], [0, 6]]


# ---- 3. the windows rule ----
def test_window_clip_rule():
    assert V.clip_row((0, 150), 150, 200) == (0, 150)          # an insert longer than the read cuts nothing
    assert V.clip_row((0, 150), 150, 100) == (0, 100)
    assert V.clip_row((10, 120), 150, 100) == (10, 90)         # a prior trim row keeps its start
    assert V.clip_row((10, 50), 150, 100) == (10, 50)          # ... and its end when that is inside the insert
    assert V.clip_row((100, 20), 150, 100) == (0, 0)           # start == I: nothing is left
    assert V.clip_row((120, 20), 150, 100) == (0, 0)           # start > I
    assert V.clip_row((0, 0xFFFFFFFF), 150, 100) == (0, 100)   # a length past the read is clamped first
    assert V.clip_row((0xFFFFFFFF, 0xFFFFFFFF), 150, 100) == (0, 0)
    assert V.clip_row((149, 0xFFFFFFFF), 150, 150) == (149, 1)
    assert V.clip_row((0, 0), 150, 100) == (0, 0)
    assert V.clip_row((0, 5), 0, 1) == (0, 0)                  # an empty read


# ---- 4. the forge is what it claims ----
def at_true_offset(pair, d, p):
    ov, mis = V.mis_at(pair.r1, pair.r2, d)
    return ov, mis, V.accepted(ov, mis, p)


def test_forge_is_what_it_claims():
    pairs = V.forge()
    assert 2800 <= len(pairs) <= 3400
    cats = {c: [p for p in pairs if p.cat == c] for c in {p.cat for p in pairs}}
    assert set(cats) == {"frag", "unequal", "boundary", "n_in", "n_out", "limits", "repeat", "random", "noisy"}
    D = V.DEFAULTS
    # fragments: every length 1 .. 2 L + 5; a fragment whose mates overlap by 30 or more is found at d = F - L
    for L in V.FRAG_LENGTHS:
        assert sorted(p.note[1] for p in cats["frag"] if p.note[0] == L) == list(range(1, 2 * L + 6))
    signs = set()
    for p in cats["frag"]:
        L, F = p.note
        assert len(p.r1) == len(p.r2) == L
        ov = F if F <= L else 2 * L - F
        res = V.overlap_one(p.r1, p.r2, D)
        if ov >= D.min_overlap:
            assert res == (F - L, ov, 0, F), p.note
            signs.add(np.sign(F - L))
    assert signs == {-1, 0, 1}
    got = {p.note[:2] for p in cats["unequal"]}
    assert {(150, 100), (40, 150), (1024, 1024), (1025, 150), (0, 150)} <= got
    assert all(V.overlap_one(p.r1, p.r2, D) == "long" for p in cats["unequal"] if p.note[0] == 1025)
    assert any(isinstance(V.overlap_one(p.r1, p.r2, D), tuple) for p in cats["unequal"] if p.note[:2] == (1024, 1024))
    assert any((r := V.overlap_one(p.r1, p.r2, D)) and r[3] < 40 for p in cats["unequal"] if p.note[:2] == (40, 150))
    # read-through: d < 0 and an insert shorter than both mates
    rt = [V.overlap_one(p.r1, p.r2, D) for p in cats["noisy"]]
    assert sum(1 for r in rt if r and r[0] < 0 and r[3] < 150) > 100 and sum(1 for r in rt if r and r[0] > 0) > 100
    # mismatch boundaries: exactly max_diff mismatches at d = 30 are accepted, one more is not, wherever they are
    names = set()
    for p in cats["boundary"]:
        name, nmis, side = p.note
        ov, mis, ok = at_true_offset(p, 30, D)
        assert (ov, mis) == (70, nmis) and ok == (nmis == D.max_diff)
        assert (V.overlap_one(p.r1, p.r2, D) == (30, 70, nmis, 130)) == ok
        names.add((name, nmis, side))
    assert names == {(n, m, s) for n in ("first", "last", "w1lo", "w1hi", "w1lo2", "w1hi2", "wRlo", "wRhi", "wRlo2", "wRhi2")
                     for m in (5, 6) for s in (1, 2)}
    # N just inside the overlap is one more mismatch, just outside it is none
    for p in cats["n_in"] + cats["n_out"]:
        side, nmis = p.note
        ov, mis, ok = at_true_offset(p, 30, D)
        assert (ov, mis) == (70, nmis + (p.cat == "n_in"))
        assert (b"N" in (p.r1 if side == 1 else p.r2)) and (V.overlap_one(p.r1, p.r2, D) is not None) == ok
    assert {(p.cat, *p.note, V.overlap_one(p.r1, p.r2, D) is None) for p in cats["n_in"] + cats["n_out"]} >= {
        ("n_in", 1, 5, True), ("n_in", 2, 5, True), ("n_out", 1, 5, False), ("n_out", 2, 5, False), ("n_in", 1, 4, False)}
    # the two limits around ov = min_overlap: with the defaults max_diff binds (6 of 30 passes the rate alone),
    # with RATE the rate binds (4 of 30 passes max_diff alone)
    for p in cats["limits"]:
        ov, nmis = p.note
        assert V.mis_at(p.r1, p.r2, 100 - ov) == (ov, nmis)
        for prm in (D, V.RATE):
            want = ov >= 30 and nmis <= prm.max_diff and 1000 * nmis <= prm.max_err_milli * ov
            assert (V.overlap_one(p.r1, p.r2, prm) == (100 - ov, ov, nmis, 200 - ov)) == want, (p.note, prm)
    lim = {p.note: p for p in cats["limits"]}
    assert 1000 * 6 <= D.max_err_milli * 30 and 6 > D.max_diff and V.overlap_one(lim[30, 6].r1, lim[30, 6].r2, D) is None
    assert 4 <= V.RATE.max_diff and 1000 * 4 > V.RATE.max_err_milli * 30 and V.overlap_one(lim[30, 4].r1, lim[30, 4].r2, V.RATE) is None
    assert V.overlap_one(lim[29, 3].r1, lim[29, 3].r2, D) is None and V.overlap_one(lim[31, 5].r1, lim[31, 5].r2, D) is not None
    # several accepted offsets: the first of the order is the answer
    several = 0
    for p in cats["repeat"]:
        ok = [d for d in V.candidates(len(p.r1), len(p.r2)) if V.accepted(*V.mis_at(p.r1, p.r2, d), D)]
        res = V.overlap_one(p.r1, p.r2, D)
        assert (res[0] if res else None) == (ok[0] if ok else None)
        several += len(ok) > 1
    assert several >= 6 and V.overlap_one(b"N" * 50, b"N" * 50, V.ALWAYS) == (0, 50, 50, 50)
    assert all(V.overlap_one(p.r1, p.r2, D) is None for p in cats["random"]) and len(cats["random"]) == 200
    # ALWAYS accepts the first candidate of 30 bases or more: d = 0 for every pair of two reads that long
    for p in pairs:
        if 30 <= len(p.r1) <= 1024 and 30 <= len(p.r2) <= 1024:
            assert V.overlap_one(p.r1, p.r2, V.ALWAYS)[0] == 0
    # the maps: a permutation of every record, and one with entries that leave pairs out
    n = len(pairs)
    s1, s2, rec1, rec2 = V.forge_sets("permutation")
    assert sorted(rec1.tolist()) == sorted(rec2.tolist()) == list(range(n)) and (rec2 != np.arange(n)).sum() > n // 2
    assert all(s1[rec1[i]] == pairs[i].r1 and s2[rec2[i]] == pairs[i].r2 for i in range(n))
    _, _, h1, h2 = V.forge_sets("holes")
    assert len(h1) == len(h2) == n - 37 and (h1 == -1).any() and (h2 == n).any() and (h1 == 1 << 40).any() and (h2 < -1).any()
    ref = V.forge_reference("defaults", "holes")
    assert ref["unmapped"] == int(((h1 < 0) | (h1 >= n) | (h2 < 0) | (h2 >= n)).sum()) > 100
    assert ref["too_long"] >= 3 and ref["negative"] > 300 and ref["adapter"] > 300 and ref["pairs"] == n - 37
    assert ref["pairs"] == ref["unmapped"] + ref["too_long"] + ref["analysed"] and ref["found"] == ref["hist"].sum()


def test_pack_strings_is_the_packed_reads_format():
    import seqpack_ref as R
    reads = [b"ACGTN", b"", b"T" * 32, b"GATTACA" * 9 + b"n", b"C" * 33]
    raw, desc = b"", []
    for s in reads:
        n1 = len(raw) + 2
        raw += b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"
        desc.append((n1, n1 + len(s) + 1, n1 + len(s) + 3, len(raw) - 1))
    want = R.pack_reference([raw], [np.array(desc, np.uint32)], quality=False)
    got = V.pack_strings(reads)
    for k in ("seq_off", "seq_len", "bases", "mask"):
        assert np.array_equal(got[k], want[k]), k
    h = pp.PackedReads(got["seq_off"], got["seq_len"], got["bases"], got["mask"])
    assert [h.sequence(j) for j in range(len(reads))] == [b"ACGTN", b"", b"T" * 32, b"GATTACA" * 9 + b"N", b"C" * 33]


# ---- 5. the library without a device ----
def test_struct_check_field_by_field_and_null_handles():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    assert C.sizeof(_lib.PpgPairOverlap) == 64 and C.sizeof(_lib.PpgPairOverlapResult) == 8 * 16
    assert C.sizeof(_lib.PpgPackedView) == 48 and _lib.PpgPairOverlapResult.clipped.offset == 72
    check = lib.ppg_pair_overlap_check
    mk = lambda *a: _lib.PpgPairOverlap(a[0], a[1], a[2], a[3], (C.c_int64 * 4)(*a[4:]))   # noqa: E731
    for good in (mk(0, 30, 5, 200), mk(0, 1, 0, 0), mk(0, 1 << 40, 1 << 40, 1000), mk(0, 1025, 0, 1000)):
        assert check(C.byref(good)) == 0
    for bad in (mk(1, 30, 5, 200), mk(-1, 30, 5, 200), mk(0x100, 30, 5, 200), mk(0, 0, 5, 200), mk(0, -3, 5, 200),
                mk(0, 30, -1, 200), mk(0, 30, 5, -1), mk(0, 30, 5, 1001), mk(0, 30, 5, 200, 1), mk(0, 30, 5, 200, 0, 1),
                mk(0, 30, 5, 200, 0, 0, -1), mk(0, 30, 5, 200, 0, 0, 0, 9)):
        assert check(C.byref(bad)) == E
    assert check(None) == E
    s = pp.PairOverlap().struct()
    assert (s.flags, s.min_overlap, s.max_diff, s.max_err_milli, list(s.reserved)) == (0, 30, 5, 200, [0, 0, 0, 0])
    assert V.struct_of(V.EXACT).min_overlap == 1
    for bad in (pp.PairOverlap(0), pp.PairOverlap(30, -1), pp.PairOverlap(30, 5, 1001)):
        with pytest.raises(ValueError):
            bad.struct()
    good, res, view = pp.PairOverlap().struct(), _lib.PpgPairOverlapResult(), _lib.PpgPackedView()
    assert lib.ppg_pairs_overlap(None, C.byref(good), C.byref(view), C.byref(view), None, None, 0, None, 0, None, 0, None,
                                 0, None, 0, C.byref(res), None, 0) == E
    with pytest.raises(ValueError):     # host arrays are not taken
        h = V.pack_strings([b"ACGT"])
        p = pp.PackedReads(h["seq_off"], h["seq_len"], h["bases"], h["mask"])
        pp.pair_overlap(p, p, pp.PairOverlap())


def test_result_view():
    ref = V.overlap_reference([b"AACCGG", b"ACGTTCAC"], [b"GTAACC", b"AACGTGAG"], V.Params(2, 0, 0))
    res = _lib.PpgPairOverlapResult(*[ref[k] for k in V.TOTALS], (C.c_int64 * 2)(*ref["clipped"]))
    v = pp.PairOverlapResult(res, ref["hist"])
    assert [getattr(v, k) for k in V.TOTALS] == [2, 0, 0, 2, 2, 1, 1, 7, 0] and v.clipped == (3, 3)
    assert v.median_insert == 5 and v.insert_hist.shape == (2048,) and v.rows is None and v.windows1 is None
    assert pp.PairOverlapResult(_lib.PpgPairOverlapResult(), np.zeros(2048, np.int64)).median_insert is None
    h = np.zeros(2048, np.int64)
    h[[100, 200, 300]] = (1, 1, 2)
    assert pp.PairOverlapResult(res, h).median_insert == 200


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    for name in ("ppg_pair_overlap_check", "ppg_pairs_overlap"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert hasattr(_lib.lib, "ppgx_pairoverlap_times") and hasattr(_lib.lib, "ppgx_pairoverlap_grid")
    assert "} ppg_pair_overlap;" in h and "} ppg_pair_overlap_result;" in h and "} ppg_packed_view;" in h
    assert h.index("read trimming:") < h.index("pair overlap:") and "PPG_OVERLAP_MAX_LEN = 1024" in h
    assert (_lib.PPG_OVERLAP_MAX_LEN, _lib.PPG_OVERLAP_HIST) == (V.MAX_LEN, V.HIST) == (1024, 2048)
    flat = re.sub(r"\s*\n \*\s*", " ", h)
    assert "d = 0, 1, ..., L1 - 1, -1, -2, ..., -(L2 - 1)" in flat and "1000 * mis(d) <= max_err_milli * ov(d)" in flat
