"""Sequence queries on the GPU (ppg_seqquery.hip through the shard ABI and the Python layer) against
the reference of the semantics (tests/seqquery_ref.py): totals, census, hits per chunk and the mask
words, all exact (integer work: no tolerance).  Inputs: every golden case, the synthetic Illumina
file, and per pattern a forged file with matches planted at unit boundaries, in the offset carry and
in the lines that must not match; tests/test_seqquery_cpu.py guards that they are what they claim."""
import ctypes as C
import os

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
from conftest import GOLDEN, load_case
import seqpack_ref as R
import seqquery_ref as Q

pytestmark = pytest.mark.gpu


def comp_range(gz, index, first, n):
    _, i0, _, _ = index.point_fields(first)
    _, i1, _, _ = index.point_fields(first + n)
    return np.frombuffer(gz[i0 - 1:i1], np.uint8)


def shard_of(gz, cs, device, **kw):
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    n = ix.Count - 1
    return pp.Shard(ix, comp_range(gz, ix, 0, n), 0, n, device=device, **kw)


def make_shard(name, device, **kw):
    return shard_of(*R.load_input(name), device, **kw)


def mask_words(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def assert_equals_reference(q, ref, mask=True):
    assert (q.records, q.hits, q.bases) == (ref["records"], ref["hits"], ref["bases"])
    assert [q.counts[c] for c in pp.SeqQuery.CLASSES] == ref["counts"].tolist()
    assert q.chunk_hits.dtype == np.int64 and np.array_equal(q.chunk_hits, ref["chunk_hits"])
    if mask:
        got = mask_words(q.hit_mask)
        assert got.size >= ref["mask"].size and np.array_equal(got[:ref["mask"].size], ref["mask"])   # pad bits 0
        assert np.array_equal(q.hit_records().cpu().numpy(), np.nonzero(ref["hit"])[0])
    else:
        assert q.hit_mask is None


@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_query_sequences_matches_reference(name, device):
    sh = make_shard(name, device).run()
    for pattern in Q.PATTERNS:
        ref = Q.reference(name, pattern)
        assert_equals_reference(sh.query_sequences(pattern, mask=True), ref)
        assert_equals_reference(sh.query_sequences(pattern), ref, mask=False)
    assert sh.seqquery is None      # no hook was attached


@pytest.mark.parametrize("pattern", Q.FORGED_PATTERNS, ids=lambda p: "m%d" % len(p))
def test_forged_input(pattern, device):
    """Matches at start 0, at L - m, across every kind of unit boundary, in records that start in the
    offset carry; near misses and decoys: mask and totals equal the reference (64 bytes included)."""
    ref = Q.query_reference(Q.forged_chunks(pattern), pattern)
    sh = shard_of(Q.forged_gz(pattern), Q.FORGED_CHUNK, device).run()
    assert_equals_reference(sh.query_sequences(pattern, mask=True), ref)
    assert_equals_reference(sh.query_sequences(pattern), ref, mask=False)


def test_bad_patterns_are_argument_errors(device):
    sh = make_shard("one_record", device).run()
    assert sh.query_sequences(b"A" * 64).records == 1
    for bad in (b"A" * 65, b"AC\nGT", b"\n"):
        with pytest.raises(pp.PpgError) as e:
            sh.query_sequences(bad)
        assert e.value.code == _lib.PPG_ARG_ERROR
        with pytest.raises(pp.PpgError) as e:
            sh.set_seqquery(bad)
        assert e.value.code == _lib.PPG_ARG_ERROR


def test_multi_batch_hook(device):
    """memlevel1_c10 through an 8 KiB output buffer (more than 4 batches), queried batch by batch."""
    import torch
    name = "memlevel1_c10"
    ref = Q.reference(name, b"GATTAC")
    words = ref["mask"].size
    plain = make_shard(name, device, out_capacity=8192).run()
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4 and sh.seqquery is None
    mask = torch.full((words,), -1, dtype=torch.int32, device=torch.device("cuda", device.device))
    sh.set_seqquery(b"GATTAC", mask)
    assert sh.seqquery is None                  # attached, not run yet
    for _ in range(2):                          # a second run starts its totals from 0 again
        sh.run()
        assert_equals_reference(sh.seqquery, ref)
        assert np.array_equal(mask_words(mask), ref["mask"])
    # ... which is the one-batch result, and the run itself is the run without the hook
    assert_equals_reference(make_shard(name, device).run().query_sequences(b"GATTAC", mask=True), ref)
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    for k in range(sh.n):
        assert np.array_equal(plain.chunk_records(k), sh.chunk_records(k)), k
    # without a mask the hits are counted from batch scratch
    assert_equals_reference(sh.set_seqquery(b"GATTAC").run().seqquery, ref, mask=False)
    # the census alone: every record a hit, the words batches share filled from both sides
    mask.fill_(0x5A5A5A5A)
    assert_equals_reference(sh.set_seqquery(b"", mask).run().seqquery, Q.reference(name, None))
    # off: the next run leaves nothing ready
    assert sh.set_seqquery(None).run().seqquery is None


def _buffer(device, words):
    """A mask buffer 4 KiB larger than `words` words need, every byte 0xA5."""
    import torch
    t = torch.full((4 * words + 4096,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", device.device))
    torch.cuda.synchronize(t.device)
    return t


def _query_seq(sh, pattern, buf, rec_cap):
    res = _lib.PpgSeqQueryResult()
    rc = _lib.lib.ppg_shard_query_seq(sh.handle, pattern, len(pattern), C.c_void_p(buf.data_ptr()), rec_cap, None,
                                      C.byref(res))
    return rc, res


def test_capacities(device):
    name, pattern = R.SYNTH, b"ACGT"
    ref = Q.reference(name, pattern)
    rec = ref["records"]
    cap = (rec + 31) // 32 * 32
    assert cap - 32 < rec
    sh = make_shard(name, device)
    buf = _buffer(device, cap // 32)
    assert _query_seq(sh, pattern, buf, cap)[0] == _lib.PPG_ARG_ERROR          # before any run
    sh.run()
    device.after_torch()
    assert _query_seq(sh, pattern, buf, cap + 1)[0] == _lib.PPG_ARG_ERROR      # rec_cap no multiple of 32
    assert _query_seq(sh, pattern, buf, cap - 32)[0] == _lib.PPG_BUF_ERROR     # one unit short
    assert bool((buf == 0xA5).all())                                           # ... and nothing was written
    rc, res = _query_seq(sh, pattern, buf, cap)                                # exact
    assert rc == 0 and (res.records, res.hits, res.bases) == (rec, ref["hits"], ref["bases"])
    assert list(res.count) == ref["counts"].tolist()
    assert np.array_equal(buf[:cap // 8].cpu().numpy().view(np.uint32), ref["mask"])
    assert bool((buf[cap // 8:] == 0xA5).all())
    # a multi-batch shard has no resident output to query in one call
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    assert mb.batches > 1
    assert _query_seq(mb, pattern, _buffer(device, 32), 1024)[0] == _lib.PPG_ARG_ERROR
    # the hook checks its cap too: the run fails, nothing is ready
    import torch
    small = torch.zeros(mb.total_records // 32 - 1, dtype=torch.int32, device=buf.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_seqquery(pattern, small).run()
    assert e.value.code == _lib.PPG_BUF_ERROR and mb.seqquery is None


def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_seqpack.test_failed_run_leaves_hook_unready builds it, with the hook attached."""
    import torch
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    sh.set_seqquery(b"GATTAC", torch.zeros((1 << 12) // 32, dtype=torch.int32, device=torch.device("cuda", device.device)))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert sh.seqquery is None


def test_batched_fastq_counts(tmp_path, device):
    """CountPattern / CountBases through BatchedFASTQ: RunPattern's count and Program.cs's base count."""
    for name in ("l6_c200", "l6_c20"):
        gz, cs = R.load_input(name)
        p = tmp_path / (name + ".fastq.gz")
        p.write_bytes(gz)
        ix = pp.Core.BuildDeflateIndex(gz, cs)
        ref = Q.reference(name, b"GATTAC")
        b = pp.BatchedFASTQ(ix, str(p), device=device)
        if name == "l6_c200":
            assert b.CountPattern(b"GATTAC") == ref["hits"] == 79
            assert b.CountPattern("GATTAC") == 79
        else:
            bases = b.CountBases()
            assert bases["A"] == int(ref["counts"][0])
            assert [bases[c] for c in pp.SeqQuery.CLASSES] == ref["counts"].tolist()
            b.query_out_capacity = 256 << 10          # several batches: the same counts
            assert b.CountBases() == bases and b.CountPattern(b"GATTAC") == ref["hits"]
