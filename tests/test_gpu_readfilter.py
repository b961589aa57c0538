"""Read filters on the GPU (ppg_readfilter.hip through the shard ABI, the cursor and the Python layer)
against the reference of the semantics (tests/readfilter_ref.py): totals, fail counts, Quality census,
passes per chunk, mask words and metrics rows, all exact (integer work: no tolerance).  Inputs: every
golden case, the synthetic Illumina file, and a forged file with records at the unit, wave and block
boundaries of the kernels' unit map and Quality lines shorter and longer than their Sequence;
tests/test_readfilter_cpu.py guards that they are what they claim."""
import ctypes as C
import os

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
from conftest import GOLDEN, load_case
import seqpack_ref as R
import seqquery_ref as Q
import seqselect_ref as S
import readfilter_ref as F

pytestmark = pytest.mark.gpu

SEL_ARRAYS = ("recno", "sel_off", "desc", "bytes")


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


def struct_of(f, and_mask=False):
    s = _lib.PpgReadFilter(*f)
    if and_mask:
        s.criteria |= F.AND_MASK
    return s


def mask_words(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def dev_words(words, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(torch.device("cuda", device.device))


def assert_totals(r, ref):
    assert (r.records, r.passed) == (ref["records"], ref["passed"])
    assert [r.failed[c] for c in pp.ReadFilterResult.CRITERIA] == ref["failed"].tolist()
    assert (r.bases, r.other, r.qual_bytes) == (ref["bases"], ref["other"], ref["qual_bytes"])
    assert r.qual_count.dtype == np.int64 and np.array_equal(r.qual_count, ref["qual_count"])


def assert_equals_reference(r, ref, mask=True, metrics=True):
    assert_totals(r, ref)
    assert r.chunk_passed.dtype == np.int64 and np.array_equal(r.chunk_passed, ref["chunk_passed"])
    if mask:
        got = mask_words(r.pass_mask)
        assert got.size >= ref["mask"].size and np.array_equal(got[:ref["mask"].size], ref["mask"])   # pad bits 0
        assert np.array_equal(r.pass_records().cpu().numpy(), np.nonzero(ref["pass"])[0])
    else:
        assert r.pass_mask is None
    if metrics:
        got = r.metrics_host()
        assert got.dtype == F.METRICS_DTYPE and got.shape == ref["metrics"].shape
        for field in F.METRICS_DTYPE.names:                    # row by row, field by field
            assert np.array_equal(got[field], ref["metrics"][field]), field
    else:
        assert r.metrics is None


# ---- 1. parity ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_filter_reads_matches_reference(name, device):
    sh = make_shard(name, device).run()
    for f in F.FILTERS + F.GOLDEN_FILTERS:
        ref = F.reference(name, f)
        assert_equals_reference(sh.filter_reads(struct_of(f), mask=True, metrics=True), ref)
        assert_equals_reference(sh.filter_reads(struct_of(f)), ref, mask=False, metrics=False)
    assert sh.readfilter is None      # no hook was attached


@pytest.mark.parametrize("f", F.FILTERS, ids=F.FILTER_IDS)
def test_forged_input(f, device):
    """Records at the unit, wave and block boundaries, Quality lines one short, one long, 40 long and
    empty, records without a Sequence, records across the carry seam: every output equals the reference."""
    ref = F.forged_reference(f)
    sh = shard_of(F.forged_gz(), F.FORGED_CHUNK, device).run()
    assert_equals_reference(sh.filter_reads(struct_of(f), mask=True, metrics=True), ref)
    assert_equals_reference(sh.filter_reads(struct_of(f), mask=True), ref, metrics=False)
    assert_equals_reference(sh.filter_reads(struct_of(f), metrics=True), ref, mask=False)
    # AND with a prior mask: the records' bits become old & pass, the bits past them stay
    rng = np.random.default_rng(3)
    prior = rng.integers(0, 1 << 32, ref["mask"].size + 2, dtype=np.uint64).astype(np.uint32)
    want = F.filter_reference(F.forged_chunks(), f, prior)["mask"]
    t = dev_words(prior, device)
    r = sh.filter_reads(struct_of(f), mask=t)
    assert_totals(r, ref)
    assert np.array_equal(mask_words(t), want) and r.pass_mask is t


# ---- 2. capacities ----
def _buffer(device, nbytes):
    """A buffer 4 KiB larger than asked for, every byte 0xA5."""
    import torch
    t = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", device.device))
    torch.cuda.synchronize(t.device)
    return t


def _filter_reads(sh, f, mask, rec_cap, metrics, metrics_cap, shift=0):
    res = _lib.PpgReadFilterResult()
    rc = _lib.lib.ppg_shard_filter_reads(sh.handle, C.byref(f), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                         rec_cap, C.c_void_p(metrics.data_ptr() + shift) if metrics is not None else None,
                                         metrics_cap, None, C.byref(res))
    return rc, res


def test_capacities(device):
    name, f = R.SYNTH, struct_of(F.GOLDEN_FILTERS[-1])
    ref = F.reference(name, F.GOLDEN_FILTERS[-1])
    rec = ref["records"]
    cap = (rec + 31) // 32 * 32
    assert cap - 32 < rec
    sh = make_shard(name, device)
    mask, rows = _buffer(device, cap // 8), _buffer(device, 24 * rec)
    assert _filter_reads(sh, f, mask, cap, rows, rec)[0] == _lib.PPG_ARG_ERROR          # before any run
    sh.run()
    device.after_torch()
    untouched = lambda: bool((mask == 0xA5).all()) and bool((rows == 0xA5).all())       # noqa: E731
    assert _filter_reads(sh, f, mask, cap + 1, rows, rec)[0] == _lib.PPG_ARG_ERROR      # rec_cap no multiple of 32
    assert _filter_reads(sh, f, mask, cap - 32, rows, rec)[0] == _lib.PPG_BUF_ERROR     # one unit short
    assert _filter_reads(sh, f, mask, cap, rows, rec - 1)[0] == _lib.PPG_BUF_ERROR      # one row short
    assert _filter_reads(sh, f, mask, cap, rows, rec, shift=4)[0] == _lib.PPG_ARG_ERROR  # metrics not 8-byte aligned
    assert _filter_reads(sh, f, mask, cap, rows, -1)[0] == _lib.PPG_ARG_ERROR
    assert _filter_reads(sh, f, None, 0, None, rec)[0] == _lib.PPG_ARG_ERROR            # a cap without its buffer
    assert _filter_reads(sh, struct_of(F.GOLDEN_FILTERS[-1], and_mask=True), None, 0, rows, rec)[0] == _lib.PPG_ARG_ERROR
    assert untouched()                                                                  # ... and nothing was written
    rc, res = _filter_reads(sh, f, mask, cap, rows, rec)                                # exact
    assert rc == 0 and (res.records, res.passed) == (rec, ref["passed"]) and list(res.failed) == ref["failed"].tolist()
    assert np.array_equal(mask[:cap // 8].cpu().numpy().view(np.uint32), ref["mask"])
    assert bool((mask[cap // 8:] == 0xA5).all())
    assert np.array_equal(rows[:24 * rec].cpu().numpy().view(F.METRICS_DTYPE), ref["metrics"])
    assert bool((rows[24 * rec:] == 0xA5).all())
    # a multi-batch shard has no resident output to filter in one call
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    assert mb.batches > 1
    total = mb.total_records                 # (a failed run below resets it)
    assert _filter_reads(mb, f, _buffer(device, 128), 1024, None, 0)[0] == _lib.PPG_ARG_ERROR
    # the hook checks its caps too: the run fails, nothing is ready
    import torch
    small = torch.zeros(total // 32 - 1, dtype=torch.int32, device=mask.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_readfilter(f, small).run()
    assert e.value.code == _lib.PPG_BUF_ERROR and mb.readfilter is None
    few = torch.zeros(24 * (total - 1), dtype=torch.uint8, device=mask.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_readfilter(f, None, few).run()
    assert e.value.code == _lib.PPG_BUF_ERROR and mb.readfilter is None


# ---- 3. the hook ----
def test_multi_batch_hook(device):
    """memlevel1_c10 through an 8 KiB output buffer (more than 4 batches), filtered batch by batch."""
    import torch
    name, f = "memlevel1_c10", F.GOLDEN_FILTERS[-1]
    ref = F.reference(name, f)
    assert 0 < ref["passed"] < ref["records"]
    dev = torch.device("cuda", device.device)
    plain = make_shard(name, device, out_capacity=8192).run()
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4 and sh.readfilter is None
    mask = torch.full((ref["mask"].size,), -1, dtype=torch.int32, device=dev)
    rows = torch.full((24 * ref["records"],), 0xA5, dtype=torch.uint8, device=dev)
    sh.set_readfilter(struct_of(f), mask, rows)
    assert sh.readfilter is None                # attached, not run yet
    for _ in range(2):                          # a second run starts its totals from 0 again
        sh.run()
        assert_equals_reference(sh.readfilter, ref)
        assert np.array_equal(mask_words(mask), ref["mask"])
    # ... which is the one-batch result, and the run itself is the run without the hook
    assert_equals_reference(make_shard(name, device).run().filter_reads(struct_of(f), mask=True, metrics=True), ref)
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    for k in range(sh.n):
        assert np.array_equal(plain.chunk_records(k), sh.chunk_records(k)), k
    # totals alone; then no criteria into a mask of garbage: every record passes, the words batches share
    # are filled from both sides
    assert_equals_reference(sh.set_readfilter(struct_of(f)).run().readfilter, ref, mask=False, metrics=False)
    mask.fill_(0x5A5A5A5A)
    assert_equals_reference(sh.set_readfilter(struct_of(F.FILTERS[0]), mask).run().readfilter, F.reference(name, F.FILTERS[0]),
                            metrics=False)
    # off: the next run leaves nothing ready
    assert sh.set_readfilter(None).run().readfilter is None


def test_query_filter_select_chain(device):
    """The three hooks on one mask tensor: the query writes the batch's hit bits, the filter ANDs them with
    the pass bits, the selection reads the product."""
    import torch
    name, pattern, f = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[2]
    ch = R.oracle_chunks(name)
    qref, fref = Q.reference(name, pattern), F.reference(name, f)
    both = qref["hit"] & fref["pass"]
    assert 0 < both.sum() < qref["hits"]
    sref = S.select_reference(ch, both)
    dev = torch.device("cuda", device.device)
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    out = pp.SelectedRecords.empty(sref["records"], sref["nbytes"], device.device)
    sh.set_seqquery(pattern, mask).set_readfilter(struct_of(f), mask, and_mask=True).set_select(mask, out)
    for _ in range(2):
        sh.run()
        assert np.array_equal(mask_words(mask), F.words_of(both))
        h = sh.selected.to_host()
        assert (h.records, h.nbytes) == (sref["records"], sref["nbytes"])
        for key in SEL_ARRAYS:
            assert np.array_equal(getattr(h, key), sref[key]), key
        # the query's own result is the query's, the filter's its own (over every record, hit or not)
        q = sh.seqquery
        assert (q.records, q.hits, q.bases) == (qref["records"], qref["hits"], qref["bases"])
        assert [q.counts[c] for c in pp.SeqQuery.CLASSES] == qref["counts"].tolist()
        assert np.array_equal(q.chunk_hits, qref["chunk_hits"])
        assert_totals(sh.readfilter, fref)
        assert np.array_equal(sh.readfilter.chunk_passed, fref["chunk_passed"])
    # the query hook alone gives the same query result: sharing its layout with the filter changes nothing
    q2 = make_shard(name, device, out_capacity=8192).set_seqquery(pattern, torch.zeros_like(mask)).run().seqquery
    assert (q2.records, q2.hits, q2.bases, q2.counts) == (q.records, q.hits, q.bases, q.counts)


def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_seqquery.test_failed_run_leaves_hook_unready builds it, with the hook attached."""
    import torch
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    dev = torch.device("cuda", device.device)
    sh.set_readfilter(struct_of(F.FILTERS[-1]), torch.zeros((1 << 12) // 32, dtype=torch.int32, device=dev),
                      torch.zeros(24 << 12, dtype=torch.uint8, device=dev))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert sh.readfilter is None


# ---- 4. the cursor and BatchedFASTQ ----
def _fields(r):
    return (r.identifier, r.sequence, r.other, r.quality)


def _inputs(which):
    if which == "forged":
        return F.forged_gz(), F.FORGED_CHUNK, F.forged_chunks(), F.FILTERS[-1], F.FILTERS[4], b"ACG"
    gz, cs = R.load_input(which)
    return gz, cs, R.oracle_chunks(which), F.GOLDEN_FILTERS[-1], F.GOLDEN_FILTERS[2], b"GATTAC"


@pytest.mark.parametrize("which", ("forged", "memlevel1_c10"))
def test_filter_cursor_and_where(which, tmp_path, device):
    gz, cs, chunks, f_all, f_one, pattern = _inputs(which)
    p = tmp_path / (which + ".fastq.gz")
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    batch_bytes = 64 << 10
    hit = Q.query_reference(chunks, pattern)["hit"]
    for pat, f in ((pattern, f_all), (pattern, f_one), (None, f_all), (None, f_one)):
        fref = F.filter_reference(chunks, f)
        want = fref["pass"] & hit if pat is not None else fref["pass"]
        assert 0 < want.sum() < want.size, (pat, f)
        ref = S.select_reference(chunks, want)
        cur = pp.Cursor(ix, str(p), batch_bytes=batch_bytes, device=device, pattern=pat, filter=struct_of(f))
        assert cur.batches > 1
        scanned = nbytes = nsel = 0
        totals = np.zeros(265, np.int64)
        for b in cur:
            sel, r = b.selected, b.filter_result
            assert b.text is None and b.desc is None and b.record_base == scanned
            # batch by batch: the reference's records of [record_base, + nrecords)
            lo, hi = np.searchsorted(ref["recno"], [b.record_base, b.record_base + b.nrecords])
            assert sel.records == hi - lo and lo == nsel
            assert np.array_equal(sel.recno, ref["recno"][lo:hi])
            assert np.array_equal(sel.sel_off + nbytes, ref["sel_off"][lo:hi + 1])
            assert np.array_equal(sel.desc, ref["desc"][lo:hi])
            assert np.array_equal(sel.bytes, ref["bytes"][nbytes:nbytes + sel.nbytes])
            in_batch = slice(b.record_base, b.record_base + b.nrecords)
            assert (r.records, r.passed) == (b.nrecords, int(fref["pass"][in_batch].sum()))
            totals += np.array([r.records, r.passed] + [r.failed[c] for c in pp.ReadFilterResult.CRITERIA] +
                               [r.bases, r.other, r.qual_bytes] + r.qual_count.tolist(), np.int64)
            scanned += b.nrecords
            nbytes += sel.nbytes
            nsel += sel.records
        cur.close()
        assert scanned == fref["records"] and nsel == ref["records"] and nbytes == ref["nbytes"]
        assert totals.tolist() == ([fref["records"], fref["passed"]] + fref["failed"].tolist() +
                                   [fref["bases"], fref["other"], fref["qual_bytes"]] + fref["qual_count"].tolist())
    # filter=None is the select cursor: no filter result, the pattern's hits
    ref = S.select_reference(chunks, hit)
    cur = pp.Cursor(ix, str(p), batch_bytes=batch_bytes, device=device, pattern=pattern, filter=None)
    got = []
    for b in cur:
        assert b.filter_result is None
        got.append(b.selected.recno.copy())
    res = _lib.PpgReadFilterResult()
    assert _lib.lib.ppg_cursor_filter_result(cur._h, C.byref(res)) == _lib.PPG_ARG_ERROR
    cur.close()
    assert np.array_equal(np.concatenate(got), ref["recno"])
    with pytest.raises(ValueError):
        pp.Cursor(ix, str(p), device=device, packed=True, filter=struct_of(f_all))
    # BatchedFASTQ against the text enumerator filtered on the host by the reference's pass bits
    b = pp.BatchedFASTQ(ix, str(p), device=device)
    b.batch_bytes = batch_bytes
    everything = [_fields(r) for r in b]
    fref = F.filter_reference(chunks, f_one)
    assert len(everything) == fref["records"]
    assert [_fields(r) for r in b.Where(filter=struct_of(f_one))] == [e for e, ok in zip(everything, fref["pass"]) if ok]
    assert [_fields(r) for r in b.Where(pattern, struct_of(f_one))] == \
        [e for e, ok, h in zip(everything, fref["pass"], hit) if ok and h]
    assert [_fields(r) for r in b.Where(pattern)] == [e for e, h in zip(everything, hit) if h]   # the positional call
    none = F.filter_reference(chunks, F.FILTERS[0])
    for cap in (pp.BatchedFASTQ.query_out_capacity, 64 << 10):          # one batch; several batches
        b.query_out_capacity = cap
        assert_totals(b.CountPassing(struct_of(f_one)), fref)
        assert np.array_equal(b.CountPassing(struct_of(f_one)).chunk_passed, fref["chunk_passed"])
        assert np.array_equal(b.QualityCounts(), none["qual_count"])
        assert b.CountPattern(pattern) == int(hit.sum())                # the query hook still works beside it
    b.Dispose()


# ---- 5. bad filters ----
def test_bad_filters_are_argument_errors(tmp_path, device):
    import torch
    gz, cs = R.load_input("one_record")
    sh = shard_of(gz, cs, device).run()
    assert sh.filter_reads(struct_of(F.FILTERS[-1])).records == 1
    p = tmp_path / "one.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    mask = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", device.device))
    good = F.FILTERS[-1]
    for bad in (good._replace(criteria=0x20), good._replace(min_len=-1), good._replace(max_len=5), good._replace(max_other=-1),
                good._replace(qual_base=256), good._replace(low_q=224), good._replace(max_low_milli=1001),
                good._replace(min_mean_milli=255001)):
        for call in (lambda s: sh.filter_reads(s), lambda s: sh.filter_reads(s, mask=mask), lambda s: sh.set_readfilter(s),
                     lambda s: pp.Cursor(ix, str(p), device=device, filter=s),
                     lambda s: pp.Cursor(ix, str(p), device=device, pattern=b"A", filter=s)):
            with pytest.raises(pp.PpgError) as e:
                call(struct_of(bad))
            assert e.value.code == _lib.PPG_ARG_ERROR, bad
        with pytest.raises(ValueError):                     # CountPassing / Where take the same road
            pp.ReadFilter(min_length=5, max_length=4).struct()
    # AND_MASK needs a mask
    with pytest.raises(pp.PpgError) as e:
        sh.set_readfilter(struct_of(good), None, and_mask=True)
    assert e.value.code == _lib.PPG_ARG_ERROR
    assert sh.run().readfilter is None                      # none of the refused calls attached anything
