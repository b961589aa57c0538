"""What the forged FASTQ members of tests/fastq_forge.py hold, asserted on the CPU: every hazard
at the address its class claims (from the Points' outputs), every class of seam present, the two
restatements of Parsing.Parse equal on every chunk, R-P3 itself on the clean chunks, a reference
that shows a missed decline on every chunk that has one hazard (or the class is listed as
flag-only), the census-capacity boundaries, and the substituted index equal to the oracle's.
tests/test_gpu_record_scan.py runs the same members through the HIP path."""
import collections
import re

import numpy as np
import pytest

import fastq_forge as F
from oracle import oracle as O
from oracle import parse_py

SINGLE = ("nn", "nul", "raw0", "off")


def required_classes():
    """every class of chunk the members must hold: {member: {class: least count}}"""
    seams = {}
    for d in ("-1", "+0", "+1"):
        for fam in ("lane", "head", "step", "tail15"):
            seams[f"nn:{fam}:{d}"] = 3
            seams[f"nl:{fam}:{d}"] = 2
        for U in F.UNITS:
            seams[f"nn:unit{U}x1:{d}"] = seams[f"nn:unit{U}x2:{d}"] = seams[f"nl:unit{U}x1:{d}"] = 4
    for kind in ("nn", "nl"):
        for c in ("head:in", "tail15:in", "tail0:-1", "tail1:-1", "tail1:+0", "edge:1", "edge:2", "edge:last"):
            seams[f"{kind}:{c}"] = 2
    seams["nn:edge:0"] = 4
    for c in ("first", "head", "word0", "word15", "last", "tail"):
        seams[f"nul:{c}"] = 2
    starts = {f"start:{c}": 4 for c in ("empty+nl", "nl+nl", "off=nl", "off-nn", "off-nul", "off-nul-last",
                                         "clean-nl+x", "clean-x+nl")}
    split = {f"split:{c}": 3 for c in ("straddle", "before", "after", "nul-after", "nul-before", "clean-before",
                                        "clean-after", "merge-overflow")}
    split["split:merge-overflow-blank"] = 1
    w = {f"place:olen{n}": 1 for n in (0, 1, 255, 256, 257, 600, 32768)}
    w.update({f"place:onl{k}%4={r}": 1 for k in (0, 1, 3, 4, 5, 8) for r in range(4)})
    w.update({"place:body-no-nl": 1, "place:no-nl-at-all": 1, "place:records-in-offset": 1, "place:cap-boundary": 1,
              "emit:tiles": 6, "chain:gap%4=0": 17, "chain:gap%4=1": 17, "chain:gap%4=2": 17, "chain:gap%4=3": 17,
              "chain:gap-end": 1, "chain:double-blank": 18, "chain:two-skips": 62})
    w.update({f"chain:R{r}": 1 for r in (1, 15, 16, 31, 32, 33)})
    w.update({f"chain:onl{k}": 1 for k in (0, 1, 63, 64, 65, 1023, 1024, 1025)})
    w.update({f"serial:{c}": 1 for c in ("nul-offset", "nul-body0", "nul-id", "nul-seq", "nul-plus", "nul-qual",
                                         "nul-after-record", "nul-plus-skipped")})
    lone = {f"lone:{c[0]}": 3 for c in F.SPLIT_CASES}
    req = {"seams": seams, "starts": starts, "split_seams": split, "lone_pieces": lone, "writers": w}
    for v in F.GROWTH:
        req[f"growth_{v}"] = {"growth:before": 81, "growth:cross": 1, "growth:after": 50}
    return req


def seam_claim(klass, g, out, n):
    """whether address g is where a seams class says its hazard is, for a chunk at [out, out + n)"""
    a0, z, end = out + (-out % 16), (out + n) & ~15, out + n
    fam, _, d = klass.partition(":")[2].rpartition(":")
    if klass.startswith("nul:"):
        fam, d = "nul", klass[4:]
        return {"first": g == out, "head": out <= g < a0, "word0": g == a0 + 32, "word15": g == a0 + 47,
                "last": g == end - 1, "tail": end % 16 == 15 and g == z + 3}[d]
    if d == "in":
        return out <= g < a0 if fam == "head" else z < g < end - 1 and end % 16 == 15
    if fam == "edge":
        return g == (end - 1 if d == "last" else out + int(d))
    b = g - int(d)
    if fam == "lane":
        return b % 16 == 0 and a0 < b < a0 + 1024
    if fam == "head":
        return b == a0
    if fam == "step":
        return b == a0 + 1024
    if fam.startswith("tail"):
        return end % 16 == int(fam[4:]) and b == z
    U, m = map(int, re.fullmatch(r"unit(\d+)x(\d)", fam).groups())
    return b % U == 0 and b // U - (out + 3) // U == m and b + 1 < end


@pytest.mark.parametrize("name", F.NAMES)
def test_hazard_placement(name):
    """Every chunk starts at its Point's output and holds what the oracle extracts there, at both
    levels; its hazard is at the claimed global address, and there is nothing else to decline."""
    for level in F.LEVELS:
        m = F.member(name, level)
        assert m.ix.Count == m.oix.count == m.n + 1
        for k, c in enumerate(m.chunks):
            out = m.ix.point_fields(k)[0]
            n = m.ix.point_fields(k + 1)[0] - out
            assert (out, n) == (c.out, len(c.text)) and O.extract(m.gz, m.oix, k) == c.text, (name, level, k)
            for cut in c.cuts:
                assert out + cut in m.side[1] and 0 < cut < n
    for c in F.chunks_of(name):
        raw, n, ol = c.raw, len(c.text), len(c.offset)
        assert F.must_decline(raw) == (c.kind is not None), c.klass
        hz = F.hazards(raw)
        assert (hz == 0) if c.kind is None else (hz == 1) if c.kind in SINGLE else hz > 1, c.klass
        if c.h is not None:
            at = raw[ol + c.h]
            if c.kind in ("nn", "raw0"):
                assert at == 10 and (raw[ol + c.h - 1] == 10 if c.kind == "nn" else ol == 0 and c.h == 0), c.klass
            elif c.kind == "nul":
                assert at == 0, c.klass
            else:
                assert at == 10 and raw[ol + c.h - 1:ol + c.h] != b"\n" and raw[ol + c.h + 1:ol + c.h + 2] != b"\n"
            if name == "seams":
                assert seam_claim(c.klass, c.out + c.h, c.out, n), (c.klass, c.out, c.h, n)
            if name in ("split_seams", "lone_pieces") and not c.klass.startswith("split:merge"):
                d = {k: d for k, _, d in F.SPLIT_CASES}[c.klass.split(":")[1]]
                assert c.h == c.cuts[-1] + d, c.klass
    if name == "lone_pieces":
        # level 6: the cut is the only block start inside the chunk, in the second LONE_RANGE of its
        # compressed bytes, the last one (a range must leave 1 KiB before the chunk's end)
        m = F.member(name, 6)
        assert {(c.out + c.cuts[0]) % 16 for c in m.chunks if c.cuts} == {0, 1, 15}
        dense = [p[0] for p in O.build_index(m.gz, 9).points()]
        assert sorted(set(dense) - set(m.outs)) == m.cuts
        for k, c in enumerate(m.chunks):
            if c.cuts:
                bit0 = 8 * m.ix.point_fields(k)[1] - m.ix.point_fields(k)[2]
                bit1 = 8 * m.ix.point_fields(k + 1)[1] - m.ix.point_fields(k + 1)[2]
                cut = int(m.side[0][list(m.side[1]).index(c.out + c.cuts[0])])
                assert 8 * F.LONE_RANGE + 64 < cut - bit0 < bit1 - bit0 - 8192 < 16 * F.LONE_RANGE
    if name == "writers":
        for c in F.chunks_of(name):
            if c.klass == "emit:tiles":      # newlines on the body's edges and on both sides of a tile boundary
                t0 = (c.out & ~15) - c.out
                nl = {i for i, b in enumerate(c.text) if b == 10}
                assert len(c.text) > 8192 and ({0, len(c.text) - 1, t0 + 4095, t0 + 8192} <= nl or
                                               {t0 + 4096, t0 + 8191} <= nl)
                prev = next(p for p in F.chunks_of(name) if p.out + len(p.text) == c.out)
                assert prev.text[-1] == 10                       # '\n' right before the body, in its first word
            m = re.fullmatch(r"place:olen(\d+)", c.klass)
            if m:
                assert len(c.offset) == int(m.group(1))
            m = re.fullmatch(r"(place|chain):onl(\d+)(%4=(\d))?", c.klass)
            if m:
                assert c.offset.count(b"\n") == int(m.group(2))
                if m.group(4):
                    assert c.raw.count(b"\n") % 4 == int(m.group(4))
        by = {c.klass: c for c in F.chunks_of(name)}
        assert by["place:body-no-nl"].text.count(b"\n") == 0 and len(O.parse(by["place:body-no-nl"].offset,
                                                                             by["place:body-no-nl"].text)) == 1
        c = by["place:records-in-offset"]                         # limit <= onl
        assert 4 * len(O.parse(c.offset, c.text)) <= c.offset.count(b"\n") and c.text.count(b"\n")
        for r in (1, 15, 16, 31, 32, 33):
            assert len(O.parse(b"", by[f"chain:R{r}"].text)) == r


def test_coverage_census(capsys):
    """class -> chunk count: every class the record scan's seams call for is there, and the seam
    chunks start at every out_off mod 16 they can"""
    req = required_classes()
    lines = []
    for name in F.NAMES:
        have = collections.Counter(c.klass for c in F.chunks_of(name))
        for klass, least in req[name].items():
            assert have[klass] >= least, (name, klass, have[klass])
        assert set(have) - {"filler"} == set(req[name]), set(have) ^ set(req[name])
        fam = collections.Counter(re.sub(r"[:%].*", "", re.sub(r"^(nn|nl):", r"\1-", k)) for k in have.elements())
        lines.append(f"{name}: {sum(have.values())} chunks, " + ", ".join(f"{k} {v}" for k, v in sorted(fam.items())))
        lines += [f"    {k:32} {v}" for k, v in sorted(have.items())]
    mods = collections.defaultdict(set)
    for c in F.chunks_of("seams"):
        mods[c.klass].add(c.mod)
    for klass, s in mods.items():
        if klass == "filler":
            continue
        want = set(F.MODS)
        if klass.endswith("head:-1") or klass == "nul:head" or klass.endswith("head:in"):
            want = {1, 8} if "in" in klass or klass == "nul:head" else {1, 8, 15}
        if klass.startswith("nl:"):
            want -= {15} if klass == "nl:head:-1" else {0} if klass == "nl:head:+0" else set()
        assert s == want, (klass, s)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", F.NAMES)
def test_oracle_agreement_and_rp3(name):
    """oracle.parse == the literal port of Parsing.Parse on every chunk; where R-P3 holds the
    records are the 4-newline grouping; where one hazard breaks it the reference differs from the
    grouping (so a missed decline shows in the records), except in the flag-only classes, where
    it provably cannot."""
    ref = F.reference(name)
    for c, rec in zip(F.chunks_of(name), ref):
        lit = np.array(parse_py.terminators(parse_py.parse_literal(c.offset, c.text)), np.uint32).reshape(-1, 4)
        assert np.array_equal(rec, lit), c.klass
        naive = F.naive_records(c.raw)
        if not F.must_decline(c.raw):
            assert np.array_equal(lit, naive), c.klass
        elif c.kind in SINGLE:
            differs = not np.array_equal(lit, naive)
            assert differs == (c.klass not in F.FLAG_ONLY) and differs == c.seen, (c.klass, c.mod)


def test_writer_routes():
    """the kernel each writers / growth chunk goes to at the default settings, restated"""
    for c in F.chunks_of("writers"):
        want = c.klass.split(":")[0].replace("filler", "place")
        if c.klass == "chain:onl1025" or c.klass == "place:cap-boundary":
            want = {"chain:onl1025": "serial", "place:cap-boundary": "emit"}[c.klass]
        assert F.route(c.offset, c.text) == want, c.klass


def test_capacity_boundary():
    """PPG_NL_BYTES 63 and 64 put the boundary chunk's capacity at its newline count and one
    below; the merge-overflow chunks have more newlines than their own capacity, no more than their
    pieces' capacities together, and no piece overflows alone"""
    c = next(c for c in F.chunks_of("writers") if c.klass == "place:cap-boundary")
    count = c.text.count(b"\n")
    assert F.nl_capacity(len(c.text), 63) == len(c.text) // 63 + 64 == count
    assert F.nl_capacity(len(c.text), 64) == len(c.text) // 64 + 64 == count - 1
    assert F.route(c.offset, c.text, 63) == "place" and F.route(c.offset, c.text, 64) == "emit"
    for c in F.chunks_of("split_seams"):
        if c.klass.startswith("split:merge-overflow"):
            edges = [0, *c.cuts, len(c.text)]
            pieces = [c.text[a:b] for a, b in zip(edges, edges[1:])]
            assert all(p.count(b"\n") <= F.nl_capacity(len(p)) for p in pieces)
            assert F.nl_capacity(len(c.text)) < c.text.count(b"\n") <= sum(F.nl_capacity(len(p)) for p in pieces)


@pytest.mark.parametrize("variant", F.GROWTH)
def test_growth_crossing(variant):
    """the chunk whose records cross the descriptor buffer's initial capacity is the variant's
    writer's, in the first of one batch and in a later one of several"""
    ch = F.chunks_of(f"growth_{variant}")
    ref = F.reference(f"growth_{variant}")
    cap = F.initial_record_capacity(sum(len(c.text) for c in ch))
    base = np.concatenate([[0], np.cumsum([len(r) for r in ref])])
    assert base[-1] >= 3000
    k = next(i for i, c in enumerate(ch) if c.klass == "growth:cross")
    assert base[k] < cap < base[k + 1]
    assert F.route(ch[k].offset, ch[k].text) == variant
    assert all(F.route(c.offset, c.text) == "place" for i, c in enumerate(ch) if i != k)
    bs = F.batches([len(c.text) for c in ch], F.GROWTH_OUT_CAPACITY)
    assert len(bs) >= 3 and bs[0][1] <= k < bs[-1][0]


@pytest.mark.parametrize("name", F.NAMES)
def test_index_agreement(name):
    """the substituted index: the library's and the oracle's agree field by field, the offsets are
    the chunks', and the inner cuts are the oracle's dense Points inside the chunks"""
    for level in F.LEVELS:
        m = F.member(name, level)
        dense = O.build_index(m.gz, 9).points()
        by_out = {p[0]: p for p in dense[:-1]}
        inside = [(8 * n - b, o) for o, n, b, _, _ in dense if o not in m.outs]
        assert set(zip(m.side[0].tolist(), m.side[1].tolist())) <= set(inside)
        assert m.side[2].size == F.WIN * len(m.cuts)
        for i in range(m.n + 1):
            p, q = m.ix[i], m.oix.point(i)
            assert (p.Output, p.Input, p.Bits, p.Window, p.offset) == q, (name, level, i)
            assert p.offset == (m.chunks[i].offset if i < m.n else b"")
            assert (by_out[p.Output] if i < m.n else dense[-1])[:4] == q[:4]
