"""Record selection on the CPU: the reference of the semantics (tests/seqselect_ref.py) against
hand-written chunks, guards that the inputs of tests/test_gpu_seqselect.py exercise what the kernels
can get wrong (conditions on the inputs: the reference alone must satisfy them), an identity that
needs no reference module (every record selected = the decompressed text), and the presence of the
ABI in the header, the Python binding and the C# binding."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import seqpack_ref as R
import seqquery_ref as Q
import seqselect_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(offset, body):
    """(offset_k, raw_k, descriptors) of a hand-written chunk: the newline positions of raw_k, four
    per record, as Parsing.Parse finds them for well-formed text."""
    raw = offset + body
    nl = [i for i, c in enumerate(raw) if c == 10]
    return offset, raw, np.array(nl, np.uint32).reshape(-1, 4)


# ---- (a) the reference against literal chunks ----
def test_reference_on_hand_written_chunks():
    r0, r1, r2 = b"@r0\nGATTACA\n+\nIIIIIII\n", b"@r1\nACGTN\n+x\nIIIII\n", b"@\n\n+\n\n"
    c0 = _chunk(b"", r0 + r1 + r2)
    r3, r4 = b"@r3\nTTGATTAC\n+\nIIIIIIII\n", b"@r4\nAC\r\n+\r\nII\r\n"        # r3 starts in the carry; r4 is CRLF
    c1 = _chunk(r3[:9], r3[9:] + r4)
    # a duplicate: chunk 2's carry holds all of r4, which is parsed again as its record 0
    r5 = b"@r5\nG\n+\nI\n"
    c2 = _chunk(r4, r5)
    chunks = (c0, c1, c2)
    every = S.select_reference(chunks, np.ones(7, bool))
    assert every["records"] == 7 and every["recno"].tolist() == list(range(7))
    assert every["bytes"].tobytes() == r0 + r1 + r2 + r3 + r4 + r4 + r5
    assert every["sel_off"].tolist() == np.cumsum([0] + [len(x) for x in (r0, r1, r2, r3, r4, r4, r5)]).tolist()
    assert every["nbytes"] == every["sel_off"][-1]
    # descriptors are relative to the record's own first byte: the same for r4 and its duplicate
    assert every["desc"][0].tolist() == [3, 11, 13, 21]
    assert every["desc"][2].tolist() == [1, 2, 4, 5]
    assert every["desc"][3].tolist() == [3, 12, 14, 23]
    assert every["desc"][4].tolist() == every["desc"][5].tolist() == [3, 7, 10, 14]
    for i, text in enumerate((r0, r1, r2, r3, r4, r4, r5)):
        a, e = every["sel_off"][i:i + 2]
        rec = pp.FastqRecord(every["bytes"][a:e].tobytes(), 0, *every["desc"][i].tolist())
        lines = text.split(b"\n")
        assert (rec.identifier, rec.sequence, rec.other, rec.quality) == (lines[0][1:], lines[1], lines[2][1:], lines[3])
    assert pp.FastqRecord(every["bytes"].tobytes()[every["sel_off"][4]:], 0, *every["desc"][4].tolist()).sequence == b"AC\r"
    # a selection: r1, the record from the carry, the duplicate
    some = S.select_reference(chunks, [False, True, False, True, False, True, False])
    assert some["recno"].tolist() == [1, 3, 5] and some["bytes"].tobytes() == r1 + r3 + r4
    assert some["sel_off"].tolist() == [0, len(r1), len(r1) + len(r3), len(r1) + len(r3) + len(r4)]
    assert some["desc"].tolist() == [every["desc"][j].tolist() for j in (1, 3, 5)]
    # entries past the records are ignored; nothing selected is empty arrays and one offset
    assert S.select_reference(chunks, [False, True, False, True, False, True, False, True, True])["recno"].tolist() == [1, 3, 5]
    none = S.select_reference(chunks, np.zeros(7, bool))
    assert (none["records"], none["nbytes"], none["sel_off"].tolist()) == (0, 0, [0])
    assert none["desc"].shape == (0, 4) and none["bytes"].size == 0 and none["recno"].size == 0


def test_mask_words():
    hit = np.array([j % 3 == 0 for j in range(70)])
    w = S.mask_words(hit)
    assert w.size == 3 and [(int(w[j >> 5]) >> (j & 31)) & 1 for j in range(96)] == [int(j < 70 and j % 3 == 0) for j in range(96)]
    g = S.mask_words(np.ones(70, bool), garbage_words=1)
    assert g.tolist() == [0xFFFFFFFF] * 4


# ---- (b) input guards ----
def _carry_census(name, hit):
    """(selected records that start in the carry and reach into the body, that lie wholly in the carry)."""
    ch = S.chunks(name)
    straddle = wholly = 0
    for j, (k, a, e) in enumerate(S.record_spans(ch)):
        olen = len(ch[k][0])
        straddle += bool(hit[j]) and a < olen < e
        wholly += bool(hit[j]) and olen > 0 and e <= olen
    return straddle, wholly


def test_golden_inputs_reach_the_carry():
    for pattern, n in ((None, 147), (b"ACGT", 75)):
        assert _carry_census("memlevel1_c10", Q.reference("memlevel1_c10", pattern)["hit"])[0] == n
        assert _carry_census("stored_c50", Q.reference("stored_c50", pattern)["hit"])[1] == 1
    # these goldens' record lengths are all even: at most 8 destination residues, hence the forged input
    for name in ("memlevel1_c10", "stored_c50"):
        assert len(set((S.reference(name, "all")["sel_off"][:-1] % 16).tolist())) <= 8, name


def test_forged_input_guard():
    ch = S.chunks(S.FORGED)
    spans = S.record_spans(ch)
    ref = S.reference(S.FORGED, "half")
    off, recno = ref["sel_off"], ref["recno"]
    lens = np.diff(off)
    assert len(ch) > 8 and 0 < ref["records"] < len(spans)
    assert set((off[:-1] % 16).tolist()) == set(range(16))            # destination residues
    assert set((lens % 16).tolist()) == set(range(16))                # length residues
    body_res, in_carry = set(), 0
    for j in recno.tolist():
        k, a, _ = spans[j]
        olen = len(ch[k][0])
        if a >= olen:
            body_res.add((a - olen) % 16)                             # source residues within the body
        else:
            in_carry += 1
    assert body_res == set(range(16)) and in_carry >= 1
    per_word = np.bincount(np.concatenate([np.arange(off[i] // 16, (off[i + 1] - 1) // 16 + 1) for i in range(ref["records"])]))
    assert per_word.max() >= 3                                        # a 16-byte word holding three records
    assert (lens > 8192).any() and ((lens >= 100) & (lens <= 400)).sum() > 8 and (lens < 16).sum() > 8
    gaps = np.diff(recno)
    assert (gaps == 1).any()                                          # a run of consecutive selected records
    before = np.concatenate([[2], gaps])
    after = np.concatenate([gaps, [2]])
    assert ((before > 1) & (after > 1)).any()                         # an isolated one
    # the tiny records: more than the copy kernel stages at a time in one destination span, more than a tile
    # per chunk, and in 64 KiB of text more records than a cursor slot is sized for at open, of which b"A"
    # hits more than the 1,024 its pinned side starts with
    tiny = S.reference(S.TINY, "all")
    assert np.bincount(tiny["sel_off"][:-1] // S.SPAN).max() > 2 * 512 and max(len(c[2]) for c in S.chunks(S.TINY)) > 256
    first64k = int(np.searchsorted(tiny["sel_off"], (64 << 10) - 4096))
    assert first64k > (64 << 10) // 64 + 4096
    assert Q.query_reference(S.chunks(S.TINY), b"A")["hit"][:first64k].sum() > 1024


def _whole_spans_inside_a_record(off):
    """Destination spans [s * SPAN, (s + 1) * SPAN) that lie inside one selected record."""
    return sum(max(0, int(off[i + 1]) // S.SPAN - -(-int(off[i]) // S.SPAN)) for i in range(len(off) - 1))


def test_long_input_guard():
    """A selected record longer than the copy kernel's span, and longer than two; whole destination spans
    inside one record (a block with one staged record, both offsets clamped); a record that covers
    several multiples of the span; short records between the long ones."""
    with open(os.path.join(ROOT, "parallelparsing_amd", "csrc", "ppg_device.h")) as f:
        assert re.search(r"kSelSpan\s*=\s*%d\s*;" % S.SPAN, f.read())     # the span the guard is about
    for which in ("half", "all"):
        ref = S.reference(S.LONG, which)
        off = ref["sel_off"]
        lens = np.diff(off)
        assert (lens > S.SPAN).any() and (lens > 2 * S.SPAN).sum() >= 2, which
        assert _whole_spans_inside_a_record(off) >= 3, which
        multiples = [int(off[i + 1] - 1) // S.SPAN - int(off[i] - 1) // S.SPAN for i in range(ref["records"])]
        assert max(multiples) >= 3 and (lens < 16).any() and ((lens >= 100) & (lens <= 400)).any(), which
    assert 0 < S.reference(S.LONG, "half")["records"] < S.reference(S.LONG, "all")["records"]


def test_masks_are_what_they_claim():
    for name in ("memlevel1_c10", "stored_c50", "malformed_c40", S.FORGED):
        n = S.reference(name, "all")["records"]
        nchunks = sum(1 for c in S.chunks(name) if len(c[2]))
        assert S.reference(name, "none")["records"] == 0
        assert S.reference(name, "alternate")["records"] == (n + 1) // 2
        assert S.reference(name, "chunk_first")["records"] == S.reference(name, "chunk_last")["records"] == nchunks
        assert 0.3 * n < S.reference(name, "half")["records"] < 0.7 * n
        assert S.reference(name, "sparse")["records"] < 0.1 * n


# ---- (c) an identity with no reference module in between ----
@pytest.mark.parametrize("name", S.WHOLE_TEXT)
def test_select_all_is_the_text(name):
    gz, _ = R.load_input(name)
    text = zlib.decompress(gz, 31)
    got = S.reference(name, "all")["bytes"].tobytes()
    assert text.startswith(got) and len(got) == len(text)


# ---- (d) the ABI is there ----
NEW = ("ppg_shard_select_size", "ppg_shard_select_records", "ppg_shard_set_select", "ppg_shard_select_ready",
       "ppg_cursor_open_select", "ppg_cursor_selected", "ppg_cursor_selected_index")


def test_abi_presence():
    with open(os.path.join(ROOT, "include", "ppgpu.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "interop", "PpGpu.cs")) as f:
        cs = f.read()
    with open(os.path.join(ROOT, "interop", "GpuBatchedFASTQ.cs")) as f:
        en = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, cs), name
    assert "PpGpu.ppg_cursor_open_select" in en and re.search(r"IEnumerable<FastqRecord>\s+Where\s*\(\s*string", en)
    for attr in ("select_size", "select_records", "set_select", "selected"):
        assert hasattr(pp.Shard, attr), attr
    assert hasattr(pp, "SelectedRecords") and hasattr(pp.BatchedFASTQ, "Where")
    for attr in ("to_host", "record", "__iter__", "__len__", "empty"):
        assert hasattr(pp.SelectedRecords, attr), attr


def test_null_handles_and_exclusive_cursor_modes():
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    a, b = C.c_int64(), C.c_int64()
    assert lib.ppg_shard_select_size(None, None, 0, C.byref(a), C.byref(b)) == E
    assert lib.ppg_shard_select_records(None, None, 0, None, None, None, 0, None, 0, C.byref(a), C.byref(b)) == E
    assert lib.ppg_shard_set_select(None, None, 0, None, None, None, 0, None, 0) == E
    assert lib.ppg_shard_select_ready(None, C.byref(a), C.byref(b)) == E
    h = C.c_void_p()
    assert lib.ppg_cursor_open_select(None, None, b"x", 0, 0, 0, 0, b"ACGT", 4, C.byref(h)) == E
    assert lib.ppg_cursor_selected(None, None, None, C.byref(a), C.byref(b)) == E
    assert lib.ppg_cursor_selected_index(None, None, None, 0) == E
    with pytest.raises(ValueError):
        pp.Cursor(None, "x.gz", n=0, packed=True, pattern=b"ACGT")


def test_selected_records_host_container():
    ref = S.reference(S.FORGED, "half")
    sel = pp.SelectedRecords(ref["bytes"], ref["sel_off"], ref["desc"], ref["recno"])
    assert len(sel) == sel.records == ref["records"] and sel.nbytes == ref["nbytes"] and not sel.on_device
    texts = [ref["bytes"][a:e].tobytes() for a, e in zip(ref["sel_off"][:-1], ref["sel_off"][1:])]
    for rec, text in zip(sel, texts):
        lines = text.split(b"\n")
        assert (rec.identifier, rec.sequence, rec.other, rec.quality) == (lines[0][1:], lines[1], lines[2][1:], lines[3])
    assert sel.record(0).identifier == texts[0].split(b"\n")[0][1:]
    with pytest.raises(IndexError):
        sel.record(sel.records)
    e = pp.SelectedRecords.empty(5, 100)
    assert (e.sel_cap, e.byte_cap, len(e)) == (5, 100, 0) and e.sel_off.size == 6 and e.desc.shape == (5, 4)
