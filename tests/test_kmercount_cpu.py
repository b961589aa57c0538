"""The k-mer count's reference (tests/kmercount_ref.py) against a brute force over Python strings, its forge against
what it claims to contain, the key <-> word conversions of the Python layer, and the host-only validator of the C
ABI (ppg_kmer_count_check).  No GPU."""
import collections
import ctypes as C

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import kmercount_ref as K

COMP = str.maketrans("ACGT", "TGCA")


def brute(reads, k, canonical):
    """Counter of k-mer strings, position by position."""
    out = collections.Counter()
    for r in reads:
        s = r.decode("latin-1")
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if all(c in "ACGT" for c in w):
                out[min(w, w.translate(COMP)[::-1]) if canonical else w] += 1
    return out


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_reference_matches_brute_force(k, canonical):
    reads = [r.seq for r in K.forge() if r.cat != "genome"] + [r.seq for r in K.forge() if r.cat == "genome"][:40]
    ref = K.reference(reads, k, canonical)
    want = brute(reads, k, canonical)
    got = {K.word_of(key, k): int(c) for key, c in zip(ref["keys"], ref["counts"])}
    assert got == dict(want)
    assert list(ref["keys"]) == sorted(ref["keys"]) and [K.word_of(x, k) for x in ref["keys"]] == sorted(want)   # unsigned = lexicographic
    assert ref["kmers"] == sum(want.values()) == ref["total_count"] and ref["distinct"] == len(want)
    assert ref["positions"] == sum(max(len(r) - k + 1, 0) for r in reads) and ref["invalid"] == ref["positions"] - ref["kmers"]
    assert ref["short_reads"] == sum(len(r) < k for r in reads) and ref["bases"] == sum(map(len, reads))
    mx = max(want.values())
    assert ref["max_count"] == mx and K.word_of(ref["max_key"], k) == min(w for w, c in want.items() if c == mx)
    assert ref["spectrum"].sum() == ref["distinct"] and ref["spectrum"][0] == 0 and ref["spectrum"][1] == ref["singletons"]


def test_windows_and_mask_in_the_reference():
    reads = [b"ACGTACGTAC", b"ACGNACGTAC", b"AC", b""]
    rows = [(2, 5), (0, 0xFFFFFFFF), (5, 1), (0xFFFFFFFF, 0xFFFFFFFF)]
    ref = K.reference(reads, 3, False, bits=[True, True, False, True], rows=rows)
    # read 0: GTACG -> GTA TAC ACG; read 1 whole: ACG | ACG CGT GTA TAC (the N breaks four positions); read 3: empty
    assert ref["participating"] == 3 and ref["bases"] == 5 + 10 + 0 and ref["positions"] == 3 + 8 and ref["kmers"] == 3 + 5
    assert ref["short_reads"] == 1 and ref["invalid"] == 3
    assert {K.word_of(k, 3): int(c) for k, c in zip(ref["keys"], ref["counts"])} == {"ACG": 3, "GTA": 2, "TAC": 2, "CGT": 1}
    assert K.window((7, 9), 10) == (7, 3) and K.window((12, 1), 10) == (10, 0)


def test_forge_contains_what_it_claims():
    f = K.forge()
    reads = K.forge_reads()
    assert 1200 < len(f) < 1700 and sum(map(len, reads)) < 200_000 and len(f) % 64 not in (0, 63)
    lens = {(r.note[0], len(r.seq)) for r in f if r.cat == "length"}
    for k in K.KS:
        assert {(k, L) for L in (0, 1, k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150)} <= lens
    assert sorted(r.seq.index(b"N") for r in f if r.cat == "n_at") == [0, 31, 32, 63, 64, 149]
    assert all(len(r.seq) == 150 and r.seq.count(b"N") == 1 for r in f if r.cat == "n_at")
    assert max(r.note for r in f if r.cat == "n_run") > max(K.KS) and all(b"N" * r.note in r.seq for r in f if r.cat == "n_run")
    assert {len(r.seq) for r in f if r.cat == "all_n"} == {1, 32, 150}
    assert any(c in next(r.seq for r in f if r.cat == "lower") for c in b"acgt") and next(r.seq for r in f if r.cat == "crlf").endswith(b"\r")
    assert collections.Counter(r.note for r in f if r.cat == "poly") == {"A": K.POLY, "T": K.POLY, "G": K.POLY}
    for r in f:
        if r.cat == "palindrome":
            k = r.note
            assert any(r.seq[p:p + k] == K.revcomp(r.seq[p:p + k]) for p in range(len(r.seq) - k + 1))
    plus, minus = [r.seq for r in f if r.cat == "strand"]
    assert minus == K.revcomp(plus) and sum(r.cat == "genome" for r in f) >= 1000
    for k in K.KS:
        for canonical in (False, True):
            ref = K.forge_reference(k, canonical)
            assert ref["spectrum"][K.SPECTRUM - 1] > 0 and ref["max_count"] > K.SPECTRUM - 1, (k, canonical)
            assert ref["invalid"] > 0 and ref["short_reads"] > 0
    # canonical collapses poly-A and poly-T: one key with both strands' count
    a, c = K.forge_reference(21, False), K.forge_reference(21, True)
    cnt = lambda ref, key: int(ref["counts"][np.searchsorted(ref["keys"], np.uint64(key))])   # noqa: E731
    assert cnt(c, 0) == cnt(a, 0) + cnt(a, 4 ** 21 - 1) and 4 ** 21 - 1 not in set(c["keys"].tolist())
    # a singleton peak and a coverage peak
    s = K.forge_reference(21, True)["spectrum"]
    assert s[1] > 3 * s[5] and s[15:60].max() > 3 * s[5]


@pytest.mark.parametrize("k", K.KS)
def test_key_word_round_trips(k):
    rng = np.random.default_rng(k)
    for canonical in (False, True):
        kc = pp.KmerCount(k, canonical)
        for _ in range(20):
            w = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=k)).decode()
            rc = w.translate(COMP)[::-1]
            key = kc.key(w)
            _, ref = K.read_keys(w.encode(), k, canonical)
            assert key == int(ref[0]) and kc.key(w.encode()) == key
            assert kc.word(key) == (min(w, rc) if canonical else w) and kc.key(kc.word(key)) == key
            assert (kc.key(rc) == key) == (canonical or rc == w)
            assert 0 <= key < 4 ** k
    for bad in ("A" * (k + 1), "A" * (k - 1), "N" * k, "a" * k):
        with pytest.raises(ValueError):
            pp.KmerCount(k).key(bad)
    with pytest.raises(ValueError):
        pp.KmerCount(k).word(4 ** k)


def test_check_struct_and_min_slots():
    chk = _lib.lib.ppg_kmer_count_check
    for k in (1, 21, 31):
        for flags in range(16):
            assert chk(C.byref(K.struct_of(k, flags))) == 0
    for k, flags in ((0, 0), (32, 1), (-1, 0), (21, 16), (21, -1), (21, 1 << 40)):
        assert chk(C.byref(K.struct_of(k, flags))) == _lib.PPG_ARG_ERROR, (k, flags)
    for i in range(6):
        s = K.struct_of(21, 1)
        s.reserved[i] = 1
        assert chk(C.byref(s)) == _lib.PPG_ARG_ERROR
    assert chk(None) == _lib.PPG_ARG_ERROR
    assert C.sizeof(_lib.PpgKmerCount) == 64 and C.sizeof(_lib.PpgKmerCountResult) == 128
    s = pp.KmerCount(17, True).struct(use_windows=True, accumulate=True)
    assert (s.flags, s.k, list(s.reserved)) == (1 | 2 | 8, 17, [0] * 6)
    assert pp.KmerCount(17, False).struct(use_mask=True).flags == 4 and pp.KmerCount().struct().flags == 1 and pp.KmerCount().k == 21
    for k in (0, 32):
        with pytest.raises(ValueError):
            pp.KmerCount(k).struct()
    assert [pp.KmerCount.min_slots(d) for d in (0, 1, 32, 33, 64, 65, 1000)] == [64, 64, 64, 128, 128, 256, 2048]
