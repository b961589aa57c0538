"""Sequence queries on the CPU: the reference of the semantics (tests/seqquery_ref.py) against
hand-written records, guards that the inputs of tests/test_gpu_seqquery.py exercise what the kernel
can get wrong (conditions on the inputs: the reference alone must satisfy them), and the presence
of the ABI in the header, the Python binding and the C# binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import seqpack_ref as R
import seqquery_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(offset, body):
    """(offset_k, raw_k, descriptors) of a hand-written chunk: the newline positions of raw_k, four
    per record, as Parsing.Parse finds them for well-formed text."""
    raw = offset + body
    nl = [i for i, c in enumerate(raw) if c == 10]
    return offset, raw, np.array(nl, np.uint32).reshape(-1, 4)


# ---- 1. the reference against literal records ----
def test_reference_on_hand_written_records():
    c0 = _chunk(b"", b"@r0\nGATTACA\n+\nIIIIIII\n"            # hit at 0, ends at L
                     b"@r1 GATTAC\nACGTN\n+GATTAC\nGATTA\n"    # pattern in the other lines only
                     b"@r2\n\n+\n\n")                          # empty Sequence
    c1 = _chunk(b"@r3\nTTGAT", b"TACgattac\n+\nIIIIIIIIIIIIII\n"   # starts in the carry, straddles it
                               b"@r4\nGATTA\n+\nCIIII\n"           # a near miss: the 'C' is the quality's
                               b"@r5\nacgtGATTAC\r\n+\nIIIIIIIIIII\n")   # CRLF: '\r' is part of the Sequence
    ref = Q.query_reference((c0, c1), b"GATTAC")
    assert ref["hit"].tolist() == [True, False, False, True, False, True]
    assert (ref["records"], ref["hits"], ref["bases"]) == (6, 3, 7 + 5 + 0 + 14 + 5 + 11)
    assert ref["chunk_hits"].tolist() == [1, 2]
    #                                A  C  G  T  other
    # GATTACA         3  1  1  2  0;  ACGTN 1 1 1 1 1;  TTGATTACgattac 2 1 1 4 6;  GATTA 2 0 1 2 0;
    # acgtGATTAC\r    2  1  1  2  5
    assert ref["counts"].tolist() == [10, 4, 5, 11, 12]
    assert int(ref["counts"].sum()) == ref["bases"]
    assert ref["mask"].tolist() == [0b101001]
    # no pattern: the census alone, every record a hit (Contains("") is true), also the empty one
    none = Q.query_reference((c0, c1), None)
    assert none["hits"] == 6 and none["mask"].tolist() == [0b111111] and none["chunk_hits"].tolist() == [3, 3]
    assert none["counts"].tolist() == ref["counts"].tolist()
    # case sensitive, and "T\r" only matches before the line end of a CRLF record
    assert Q.query_reference((c0, c1), b"gattac")["hit"].tolist() == [False, False, False, True, False, False]
    assert Q.query_reference((c0, c1), b"C\r")["hit"].tolist() == [False] * 5 + [True]
    # a record listed twice counts twice
    twice = (c1[0], c1[1], np.concatenate([c1[2][:1], c1[2]]))
    assert Q.query_reference((twice,), b"GATTAC")["hit"].tolist() == [True, True, False, True]


def test_reference_mask_pads_with_zero_bits():
    seqs = [b"@%d\nA%s\n+\nI\n" % (i, b"C" if i % 3 else b"G") for i in range(70)]
    ref = Q.query_reference((_chunk(b"", b"".join(seqs)),), b"AG")
    assert ref["records"] == 70 and ref["hits"] == 24 and ref["mask"].size == 3
    bits = [(int(ref["mask"][j >> 5]) >> (j & 31)) & 1 for j in range(96)]
    assert bits == [int(j < 70 and j % 3 == 0) for j in range(96)]


# ---- 2. input guards over the golden cases ----
L6_TYPE = [n for n in R.ALL_INPUTS if n != R.SYNTH and R.reference(n)["seq_len"].size == 2400]


def test_golden_inputs_have_hits_and_misses():
    """b"GATTAC" hits some but not all records of every golden case but one_record, b"ACGT" of every
    case but one_record and long_reads_c10; b"T\\r" hits only in crlf_c100."""
    for name in R.ALL_INPUTS:
        g, a, t = (Q.reference(name, p) for p in (b"GATTAC", b"ACGT", b"T\r"))
        if name != "one_record":
            assert 0 < g["hits"] < g["records"], name
            if name != "long_reads_c10":
                assert 0 < a["hits"] < a["records"], name
        assert (t["hits"] > 0) == (name == "crlf_c100"), name
        for ref in (g, a, t, Q.reference(name, None)):
            assert ref["records"] == R.reference(name)["seq_len"].size
            assert ref["bases"] == int(R.reference(name)["seq_len"].sum()) == int(ref["counts"].sum())
            assert int(ref["chunk_hits"].sum()) == ref["hits"] == int(ref["hit"].sum())
        assert Q.reference(name, None)["hits"] == g["records"]
    # the counts the reference finds (the GPU test compares against the reference, not these)
    hits = lambda n, p: (Q.reference(n, p)["hits"], Q.reference(n, p)["records"])   # noqa: E731
    assert len(L6_TYPE) > 4
    for name in L6_TYPE:
        assert hits(name, b"GATTAC") == (79, 2400), name
        assert hits(name, b"ACGT") == (1072, 2400), name
    assert hits("short_reads_c30", b"GATTAC") == (7, 900) and hits("short_reads_c30", b"ACGT") == (94, 900)
    assert hits("long_reads_c10", b"GATTAC") == (41, 120)
    assert hits("malformed_c40", b"GATTAC") == (13, 607)
    assert hits("crlf_c100", b"T\r") == (155, 600)


def test_golden_inputs_reach_the_carry_and_the_duplicates():
    """memlevel1_c10 has 110 of its 600 records starting inside the offset carry, and the inputs hold
    a record the reference parses twice (a chunk's first record ends inside its carry).
    The committed huffonly_c20 has none (600 parsed records for 600 in the text); stored_c50 has one
    (601 for 600), so the duplicate is looked for over all inputs and pinned there."""
    ch = R.oracle_chunks("memlevel1_c10")
    in_carry = sum(int((d[:, 0].astype(np.int64) + 1 < len(off)).sum()) for off, _, d in ch)
    assert (in_carry, sum(len(d) for _, _, d in ch)) == (110, 600)
    q1 = {name: sum(int(len(d) and int(d[0, 3]) < len(off)) for off, _, d in R.oracle_chunks(name))
          for name in R.ALL_INPUTS}
    assert q1["stored_c50"] == 1 and q1["huffonly_c20"] == 0 and sum(q1.values()) > 0
    assert Q.reference("stored_c50", None)["records"] == 601


# ---- 3. the ABI is there ----
NEW = ("ppg_shard_query_seq", "ppg_shard_set_seqquery", "ppg_shard_seqquery_ready")


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert "} ppg_seq_query_result;" in h and "struct PpgSeqQueryResult" in cs
    assert C.sizeof(_lib.PpgSeqQueryResult) == 64
    for attr in ("query_sequences", "set_seqquery", "seqquery"):
        assert hasattr(pp.Shard, attr), attr
    assert hasattr(pp, "SeqQuery") and hasattr(pp.BatchedFASTQ, "CountPattern") and hasattr(pp.BatchedFASTQ, "CountBases")


def test_null_handles_and_single_process():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    res = _lib.PpgSeqQueryResult()
    assert lib.ppg_shard_query_seq(None, b"ACGT", 4, None, 0, None, C.byref(res)) == E
    assert lib.ppg_shard_set_seqquery(None, b"ACGT", 4, None, 0) == E
    assert lib.ppg_shard_set_seqquery(None, None, -1, None, 0) == E
    assert lib.ppg_shard_seqquery_ready(None, None, C.byref(res)) == E
    b = pp.BatchedFASTQ.__new__(pp.BatchedFASTQ)      # a rank of a job: the queries are single process
    b.world, b.rank = 2, 0
    with pytest.raises(ValueError):
        b.CountPattern(b"GATTAC")
    with pytest.raises(ValueError):
        b.CountBases()


# ---- 4. the forged input ----
def _occurrences(seq, pattern):
    out, p = [], seq.find(pattern)
    while p >= 0:
        out.append(p)
        p = seq.find(pattern, p + 1)
    return out


@pytest.mark.parametrize("pattern", Q.FORGED_PATTERNS, ids=lambda p: "m%d" % len(p))
def test_forged_input_guard(pattern):
    m = len(pattern)
    assert 1 <= m <= 64 and b"\n" not in pattern
    chunks = Q.forged_chunks(pattern)
    ref = Q.query_reference(chunks, pattern)
    assert len(chunks) > 8 and 0 < ref["hits"] < ref["records"]
    recs = Q.forged_records(pattern)
    tag_of = {b"@" + ident: tag for tag, ident, _, _, _ in recs}
    carry_hit = straddle = at0 = at_end = decoys = nearmiss = 0
    j = 0
    for off, raw, desc in chunks:
        raw = bytes(raw)
        for n1, n2, _, _ in desc.astype(np.int64):
            seq, hit = raw[n1 + 1:n2], bool(ref["hit"][j])
            j += 1
            start = raw.rfind(b"\n", 0, n1) + 1
            tag = tag_of[raw[start:n1]]
            occ = _occurrences(seq, pattern)
            assert hit == bool(occ) == (tag in ("start", "end", "straddle")), (tag, seq)
            carry_hit += hit and n1 + 1 < len(off)
            straddle += any(p % 32 + m > 32 for p in occ)
            at0 += 0 in occ
            at_end += (len(seq) - m) in occ
            if tag == "decoy":
                decoys += 1
                assert not hit and raw[start:n1].endswith(pattern)
            if tag == "nearmiss":
                nearmiss += 1
                assert seq.endswith(pattern[:m - 1]) and not hit
    assert j == ref["records"] >= len(recs)       # (>: a record the reference parses twice)
    assert carry_hit > 0 and at0 > 0 and at_end > 0 and decoys > 0 and nearmiss > 0
    assert straddle > 0 or m == 1                 # a one-byte match cannot cross a unit boundary
    lengths = {len(s) for ch in Q.sequences(chunks) for s in ch}
    assert lengths >= {0, 1, m - 1, m, m + 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 150, 300}
