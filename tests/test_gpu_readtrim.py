"""Read trimming on the GPU (ppg_readtrim.hip through the shard ABI, the cursor and the Python layer)
against the reference of the semantics (tests/readtrim_ref.py): the (start, len) rows, keep mask words,
keeps per chunk and every total, all exact (integer work: no tolerance).  Inputs: every golden case, the
synthetic Illumina file, and a forged file with records at the unit, wave and block boundaries of the
kernels' unit map and a planted record for every rule of the semantics; tests/test_readtrim_cpu.py guards
that they are what they claim."""
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
import readtrim_ref as T

pytestmark = pytest.mark.gpu

SEL_ARRAYS = ("recno", "sel_off", "desc", "bytes")
TOTALS = ("records", "kept", "trimmed", "bases", "bases_window", "bases_kept")


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


def dev_words(words, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(torch.device("cuda", device.device))


def assert_totals(r, ref):
    assert [getattr(r, k) for k in TOTALS] == [ref[k] for k in TOTALS]
    assert [r.cut[c] for c in pp.ReadTrimResult.CUTS] == ref["cut"].tolist()


def assert_equals_reference(r, ref, mask=True, windows=True):
    assert_totals(r, ref)
    assert r.chunk_kept.dtype == np.int64 and np.array_equal(r.chunk_kept, ref["chunk_kept"])
    if mask:
        got = mask_words(r.keep_mask)
        assert got.size >= ref["mask"].size and np.array_equal(got[:ref["mask"].size], ref["mask"])   # pad bits 0
        assert np.array_equal(r.keep_records().cpu().numpy(), np.nonzero(ref["keep"])[0])
    else:
        assert r.keep_mask is None
    if windows:
        got = r.windows_host()
        assert got.dtype == np.uint32 and got.shape == ref["rows"].shape
        bad = np.nonzero((got != ref["rows"]).any(axis=1))[0]
        assert bad.size == 0, (bad[:8], got[bad[:8]], ref["rows"][bad[:8]])
    else:
        assert r.windows is None


# ---- 1. parity ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_trim_reads_matches_reference(name, device):
    sh = make_shard(name, device).run()
    for t in T.TRIMS:
        ref = T.reference(name, t)
        assert_equals_reference(sh.trim_reads(T.struct_of(t), mask=True, windows=True), ref)
        assert_equals_reference(sh.trim_reads(T.struct_of(t), windows=False), ref, mask=False, windows=False)
    assert sh.readtrim is None      # no hook was attached


@pytest.mark.parametrize("t", T.TRIMS, ids=T.TRIM_IDS)
def test_forged_input(t, device):
    """Records at the unit, wave and block boundaries, Quality lines one short, 40 long and empty, records
    without a Sequence, records across the carry seam, and the planted quality edges, windows and adapter
    sites: every output equals the reference."""
    ref = T.forged_reference(t)
    sh = shard_of(T.forged_gz(), T.FORGED_CHUNK, device).run()
    assert_equals_reference(sh.trim_reads(T.struct_of(t), mask=True, windows=True), ref)
    assert_equals_reference(sh.trim_reads(T.struct_of(t), mask=True, windows=False), ref, windows=False)
    assert_equals_reference(sh.trim_reads(T.struct_of(t), windows=True), ref, mask=False)
    # AND with a prior mask two words longer than the records: their bits become old & keep, the others stay
    rng = np.random.default_rng(3)
    prior = rng.integers(0, 1 << 32, ref["mask"].size + 2, dtype=np.uint64).astype(np.uint32)
    want = T.trim_reference(T.forged_chunks(), t, prior)["mask"]
    tm = dev_words(prior, device)
    r = sh.trim_reads(T.struct_of(t), mask=tm)
    assert_totals(r, ref)
    assert np.array_equal(mask_words(tm), want) and r.keep_mask is tm
    assert np.array_equal(mask_words(tm)[-2:], prior[-2:])


# ---- 2. capacities ----
def _buffer(device, nbytes):
    """A buffer 4 KiB larger than asked for, every byte 0xA5."""
    import torch
    t = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", device.device))
    torch.cuda.synchronize(t.device)
    return t


def _trim_reads(sh, t, mask, rec_cap, rows, rows_cap, shift=0):
    res = _lib.PpgReadTrimResult()
    rc = _lib.lib.ppg_shard_trim_reads(sh.handle, C.byref(t), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                       rec_cap, C.c_void_p(rows.data_ptr() + shift) if rows is not None else None,
                                       rows_cap, None, C.byref(res))
    return rc, res


def test_capacities(device):
    name, t = R.SYNTH, T.struct_of(T.ALL)
    ref = T.reference(name, T.ALL)
    rec = ref["records"]
    cap = (rec + 31) // 32 * 32
    assert cap - 32 < rec
    sh = make_shard(name, device)
    mask, rows = _buffer(device, cap // 8), _buffer(device, 8 * rec)
    assert _trim_reads(sh, t, mask, cap, rows, rec)[0] == _lib.PPG_ARG_ERROR          # before any run
    sh.run()
    device.after_torch()
    untouched = lambda: bool((mask == 0xA5).all()) and bool((rows == 0xA5).all())     # noqa: E731
    assert _trim_reads(sh, t, mask, cap + 1, rows, rec)[0] == _lib.PPG_ARG_ERROR      # rec_cap no multiple of 32
    assert _trim_reads(sh, t, mask, cap - 32, rows, rec)[0] == _lib.PPG_BUF_ERROR     # one unit short
    assert _trim_reads(sh, t, mask, cap, rows, rec - 1)[0] == _lib.PPG_BUF_ERROR      # one row short
    assert _trim_reads(sh, t, mask, cap, rows, rec, shift=4)[0] == _lib.PPG_ARG_ERROR  # rows not 8-byte aligned
    assert _trim_reads(sh, t, mask, cap, rows, -1)[0] == _lib.PPG_ARG_ERROR
    assert _trim_reads(sh, t, None, 0, None, rec)[0] == _lib.PPG_ARG_ERROR            # a cap without its buffer
    assert _trim_reads(sh, t, None, 32, rows, rec)[0] == _lib.PPG_ARG_ERROR
    assert _trim_reads(sh, T.struct_of(T.ALL, and_mask=True), None, 0, rows, rec)[0] == _lib.PPG_ARG_ERROR
    assert untouched()                                                                # ... and nothing was written
    rc, res = _trim_reads(sh, t, mask, cap, rows, rec)                                # exact
    assert rc == 0 and (res.records, res.kept, res.trimmed) == (rec, ref["kept"], ref["trimmed"])
    assert list(res.cut) == ref["cut"].tolist()
    assert np.array_equal(mask[:cap // 8].cpu().numpy().view(np.uint32), ref["mask"])
    assert bool((mask[cap // 8:] == 0xA5).all())
    assert np.array_equal(rows[:8 * rec].cpu().numpy().view(np.uint32).reshape(-1, 2), ref["rows"])
    assert bool((rows[8 * rec:] == 0xA5).all())
    # a multi-batch shard has no resident output to trim in one call
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    assert mb.batches > 1
    total = mb.total_records                 # (a failed run below resets it)
    assert _trim_reads(mb, t, _buffer(device, 128), 1024, None, 0)[0] == _lib.PPG_ARG_ERROR
    # the hook checks its caps too: the run fails, nothing is ready
    import torch
    small = torch.zeros(total // 32 - 1, dtype=torch.int32, device=mask.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_readtrim(t, small).run()
    assert e.value.code == _lib.PPG_BUF_ERROR and mb.readtrim is None
    few = torch.zeros(2 * (total - 1), dtype=torch.int32, device=mask.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_readtrim(t, None, few).run()
    assert e.value.code == _lib.PPG_BUF_ERROR and mb.readtrim is None


# ---- 3. the hook ----
def _hook_inputs(which):
    if which == "forged":
        return T.forged_gz(), T.FORGED_CHUNK, T.forged_reference(T.ALL), 64 << 10
    gz, cs = R.load_input(which)
    return gz, cs, T.reference(which, T.ALL), 8192


@pytest.mark.parametrize("which", ("forged", "memlevel1_c10"))
def test_multi_batch_hook(which, device):
    """The input through an output buffer that forces several batches, trimmed batch by batch."""
    import torch
    gz, cs, ref, cap = _hook_inputs(which)
    t = T.struct_of(T.ALL)
    assert 0 < ref["kept"] < ref["records"]
    dev = torch.device("cuda", device.device)
    plain = shard_of(gz, cs, device, out_capacity=cap).run()
    sh = shard_of(gz, cs, device, out_capacity=cap)
    assert sh.batches > 2 and sh.readtrim is None
    mask = torch.full((ref["mask"].size,), -1, dtype=torch.int32, device=dev)
    rows = torch.full((2 * ref["records"],), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    sh.set_readtrim(t, mask, rows)
    assert sh.readtrim is None                  # attached, not run yet
    for _ in range(2):                          # a second run starts its totals from 0 again
        sh.run()
        assert_equals_reference(sh.readtrim, ref)
        assert np.array_equal(mask_words(mask), ref["mask"])
    # ... which is the one-batch result, and the run itself is the run without the hook
    assert_equals_reference(shard_of(gz, cs, device).run().trim_reads(t, mask=True, windows=True), ref)
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    for k in range(sh.n):
        assert np.array_equal(plain.chunk_records(k), sh.chunk_records(k)), k
    # totals alone; then a trim that keeps everything into a mask of garbage: the words batches share are
    # filled from both sides
    assert_equals_reference(sh.set_readtrim(t).run().readtrim, ref, mask=False, windows=False)
    mask.fill_(0x5A5A5A5A)
    none = T.trim_reference(Q.chunks_of(gz, cs), T.NONE)
    assert none["kept"] == none["records"]
    assert_equals_reference(sh.set_readtrim(T.struct_of(T.NONE), mask).run().readtrim, none, windows=False)
    # attached after the run: nothing is ready; off: the next run leaves nothing ready
    assert sh.set_readtrim(t).readtrim is None
    assert sh.set_readtrim(None).run().readtrim is None


def test_query_filter_trim_select_chain(device):
    """The four hooks on one mask tensor: the query writes the batch's hit bits, the filter ANDs them with
    the pass bits, the trim with the keep bits, and the selection reads the product."""
    import torch
    name, pattern, f, t = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[2], T.ALL._replace(min_len=60)
    ch = R.oracle_chunks(name)
    qref, fref, tref = Q.reference(name, pattern), F.reference(name, f), T.reference(name, t)
    three = qref["hit"] & fref["pass"] & tref["keep"]
    assert 0 < three.sum() < (qref["hit"] & fref["pass"]).sum() < qref["hits"]
    sref = S.select_reference(ch, three)
    dev = torch.device("cuda", device.device)
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    rows = torch.full((tref["records"], 2), -1, dtype=torch.int32, device=dev)
    out = pp.SelectedRecords.empty(sref["records"], sref["nbytes"], device.device)
    sh.set_seqquery(pattern, mask).set_readfilter(_lib.PpgReadFilter(*f), mask, and_mask=True)
    sh.set_readtrim(T.struct_of(t), mask, rows, and_mask=True).set_select(mask, out)
    for _ in range(2):
        sh.run()
        assert np.array_equal(mask_words(mask), F.words_of(three))
        h = sh.selected.to_host()
        assert (h.records, h.nbytes) == (sref["records"], sref["nbytes"])
        for key in SEL_ARRAYS:
            assert np.array_equal(getattr(h, key), sref[key]), key
        # what a torch consumer does: the windows of the selected records are windows[recno]
        win = sh.readtrim.windows[sh.selected.recno[:h.records]].cpu().numpy().view(np.uint32)
        assert np.array_equal(win, tref["rows"][sref["recno"]])
        # every hook's own result is its own (the filter's and the trim's over every record, hit or not)
        q = sh.seqquery
        assert (q.records, q.hits, q.bases) == (qref["records"], qref["hits"], qref["bases"])
        assert np.array_equal(q.chunk_hits, qref["chunk_hits"])
        r = sh.readfilter
        assert (r.records, r.passed, r.bases) == (fref["records"], fref["passed"], fref["bases"])
        assert np.array_equal(r.chunk_passed, fref["chunk_passed"])
        assert_totals(sh.readtrim, tref)
        assert np.array_equal(sh.readtrim.chunk_kept, tref["chunk_kept"])
        assert np.array_equal(sh.readtrim.windows_host(), tref["rows"])


def test_paths_without_a_trim_are_unchanged(device):
    """Query, filter and select hooks with no trim attached give what their references say, also on a shard
    that had a trim attached and taken off again."""
    import torch
    name, pattern, f = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[2]
    ch = R.oracle_chunks(name)
    qref, fref = Q.reference(name, pattern), F.reference(name, f)
    both = qref["hit"] & fref["pass"]
    sref = S.select_reference(ch, both)
    dev = torch.device("cuda", device.device)
    sh = make_shard(name, device, out_capacity=8192)
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    out = pp.SelectedRecords.empty(sref["records"], sref["nbytes"], device.device)
    sh.set_seqquery(pattern, mask).set_readfilter(_lib.PpgReadFilter(*f), mask, and_mask=True).set_select(mask, out)
    for attach in (False, True):
        if attach:
            sh.set_readtrim(T.struct_of(T.ALL), mask, and_mask=True).run()
            assert sh.readtrim is not None
            sh.set_readtrim(None)
        sh.run()
        assert sh.readtrim is None
        assert np.array_equal(mask_words(mask), F.words_of(both))
        h = sh.selected.to_host()
        assert (h.records, h.nbytes) == (sref["records"], sref["nbytes"])
        for key in SEL_ARRAYS:
            assert np.array_equal(getattr(h, key), sref[key]), key
        q, r = sh.seqquery, sh.readfilter
        assert (q.records, q.hits, q.bases) == (qref["records"], qref["hits"], qref["bases"])
        assert [q.counts[c] for c in pp.SeqQuery.CLASSES] == qref["counts"].tolist()
        assert (r.records, r.passed) == (fref["records"], fref["passed"])
        assert [r.failed[c] for c in pp.ReadFilterResult.CRITERIA] == fref["failed"].tolist()
        assert np.array_equal(r.qual_count, fref["qual_count"])


def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_readfilter.test_failed_run_leaves_hook_unready builds it, with the hook attached."""
    import torch
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    dev = torch.device("cuda", device.device)
    sh.set_readtrim(T.struct_of(T.ALL), torch.zeros((1 << 12) // 32, dtype=torch.int32, device=dev),
                    torch.zeros(2 << 12, dtype=torch.int32, device=dev))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert sh.readtrim is None


# ---- 3b. every stage beside the others: one layout per batch, no state left from one call to the next ----
def assert_pack(pk, ref):
    h = pk.to_host()
    for key in ("seq_off", "seq_len", "bases", "mask", "qual"):
        got = getattr(h, key)
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key]), key


def assert_query(q, ref):
    assert (q.records, q.hits, q.bases) == (ref["records"], ref["hits"], ref["bases"])
    assert [q.counts[c] for c in pp.SeqQuery.CLASSES] == ref["counts"].tolist()
    assert np.array_equal(q.chunk_hits, ref["chunk_hits"])


def assert_filter(r, ref):
    assert (r.records, r.passed) == (ref["records"], ref["passed"])
    assert [r.failed[c] for c in pp.ReadFilterResult.CRITERIA] == ref["failed"].tolist()
    assert (r.bases, r.other, r.qual_bytes) == (ref["bases"], ref["other"], ref["qual_bytes"])
    assert np.array_equal(r.qual_count, ref["qual_count"]) and np.array_equal(r.chunk_passed, ref["chunk_passed"])


def assert_selection(sel, ref):
    h = sel.to_host()
    assert (h.records, h.nbytes) == (ref["records"], ref["nbytes"])
    for key in SEL_ARRAYS:
        assert np.array_equal(getattr(h, key), ref[key]), key


def test_all_hooks_at_once_then_pack_and_trim_alone(device):
    """Keys, pack, query, filter (AND), trim (AND) and select attached together on several batches: every
    stage gives its reference, over two runs.  Then the pack and the trim alone, the combination in which a
    batch is laid out once from the run's carry (the pack's planes) and once from 0 (the trim's scratch)."""
    import torch
    from parallelparsing_amd import paired
    from test_paired import _ref_keys
    name, pattern, f, t = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[2], T.ALL._replace(min_len=60)
    ch = R.oracle_chunks(name)
    kref = np.array([k for off, raw, desc in ch for k in _ref_keys(raw, desc, len(off))], np.int64)
    pref, qref, fref, tref = R.reference(name), Q.reference(name, pattern), F.reference(name, f), T.reference(name, t)
    three = qref["hit"] & fref["pass"] & tref["keep"]
    assert 0 < three.sum() < qref["hits"]
    sref = S.select_reference(ch, three)
    nrec = tref["records"]
    dev = torch.device("cuda", device.device)
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    rows = torch.full((nrec, 2), -1, dtype=torch.int32, device=dev)
    pk = pp.PackedReads.empty(nrec, int(pref["seq_off"][-1]), True, device.device)
    out = pp.SelectedRecords.empty(sref["records"], sref["nbytes"], device.device)
    paired.attach_keys(sh, nrec)
    sh.set_seqpack(pk).set_seqquery(pattern, mask).set_readfilter(_lib.PpgReadFilter(*f), mask, and_mask=True)
    sh.set_readtrim(T.struct_of(t), mask, rows, and_mask=True).set_select(mask, out)
    for _ in range(2):
        sh.run()
        assert np.array_equal(paired.shard_keys(sh).cpu().numpy(), kref)
        assert sh.seqpack_ready
        assert_pack(pk, pref)
        assert_query(sh.seqquery, qref)
        assert_filter(sh.readfilter, fref)
        assert_totals(sh.readtrim, tref)
        assert np.array_equal(sh.readtrim.chunk_kept, tref["chunk_kept"])
        assert np.array_equal(sh.readtrim.windows_host(), tref["rows"])
        assert np.array_equal(mask_words(mask), F.words_of(three))
        assert_selection(sh.selected, sref)
    # the pack and the trim alone, on the same shard
    aref = T.reference(name, T.ALL)
    sh.set_keys(None).set_seqquery(None).set_readfilter(None).set_select(None)
    for plane in (pk.seq_off, pk.seq_len, pk.bases, pk.mask, pk.qual):
        plane.fill_(0x5A)
    mask.fill_(0x5A5A5A5A)
    rows.fill_(0x5A5A5A5A)
    sh.set_seqpack(pk).set_readtrim(T.struct_of(T.ALL), mask, rows).run()
    assert sh.seqquery is None and sh.readfilter is None and sh.selected is None
    assert sh.seqpack_ready
    assert_pack(pk, pref)
    assert_equals_reference(sh.readtrim, aref)
    assert np.array_equal(mask_words(mask), aref["mask"])


def test_one_shot_calls_in_any_order(device):
    """On a one-batch shard after its run, every one-shot call between two trims: none depends on what the
    one before it left in the shard's scratch."""
    name, pattern, f = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[4]
    pref, qref, fref, tref = R.reference(name), Q.reference(name, pattern), F.reference(name, f), T.reference(name, T.ALL)
    sh = make_shard(name, device).run()
    assert sh.batches == 1
    assert_equals_reference(sh.trim_reads(T.struct_of(T.ALL), mask=True, windows=True), tref)
    assert_pack(sh.pack_sequences(), pref)
    q = sh.query_sequences(pattern, mask=True)
    assert_query(q, qref)
    assert np.array_equal(mask_words(q.hit_mask)[:qref["mask"].size], qref["mask"])
    assert sh.seq_bases() == (int(pref["seq_off"][-1]), pref["seq_len"].size)
    r = sh.filter_reads(_lib.PpgReadFilter(*f), mask=True, metrics=True)
    assert_filter(r, fref)
    assert np.array_equal(mask_words(r.pass_mask)[:fref["mask"].size], fref["mask"])
    got = r.metrics_host()
    for field in F.METRICS_DTYPE.names:
        assert np.array_equal(got[field], fref["metrics"][field]), field
    assert_selection(sh.select_records(q), S.select_reference(R.oracle_chunks(name), qref["hit"]))
    assert_equals_reference(sh.trim_reads(T.struct_of(T.ALL), mask=True, windows=True), tref)
    assert sh.seqquery is None and sh.readfilter is None and sh.readtrim is None and sh.selected is None


def _probe(name, *argtypes):
    fn = getattr(_lib.lib, name)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] + list(argtypes)
    return fn


def test_probe_hooks(device):
    """The measurement hooks of tools/*_probe.py, called the way the tools call them with one repetition:
    they succeed, report times and the sizes the references give, leave no hook result behind, and the
    one-shot calls after them are unharmed."""
    chunks, f, t, pattern = T.forged_chunks(), F.FILTERS[5], T.ALL, b"CTC"
    hit = Q.query_reference(chunks, pattern)["hit"]
    sref = S.select_reference(chunks, hit)
    assert 0 < sref["records"] < hit.size
    sh = shard_of(T.forged_gz(), T.FORGED_CHUNK, device)
    sh.set_seqquery(pattern).set_readfilter(_lib.PpgReadFilter(*f)).set_readtrim(T.struct_of(t)).run()
    assert sh.batches == 1 and all(r is not None for r in (sh.seqquery, sh.readfilter, sh.readtrim))
    words = dev_words(F.words_of(hit), device)
    device.after_torch()
    fp = C.POINTER(C.c_float)
    select = _probe("ppgx_seqselect_times", C.c_void_p, C.c_int64, C.c_int, fp, C.POINTER(C.c_int64))
    pack = _probe("ppgx_seqpack_times", C.c_int, C.c_int, fp, C.POINTER(C.c_int64))
    query = _probe("ppgx_seqquery_times", C.c_char_p, C.c_int32, C.c_int, fp)
    filt = _probe("ppgx_readfilter_times", C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, fp)
    trim = _probe("ppgx_readtrim_times", C.c_void_p, C.c_int, C.c_int, fp)
    fs, ts = _lib.PpgReadFilter(*f), T.struct_of(t)
    mptr, mcap = C.c_void_p(words.data_ptr()), 32 * words.numel()

    def times(n, call):
        ms = (C.c_float * n)(*([-1.0] * n))
        assert call(ms) == _lib.PPG_OK
        assert all(np.isfinite(v) and v >= 0 for v in ms), list(ms)

    for reps in (1, 0):
        ok = reps > 0
        sz, by = (C.c_int64 * 3)(), (C.c_int64 * 2)()
        calls = ((5, lambda ms: select(sh.handle, mptr, mcap, reps, ms, sz)),
                 (4, lambda ms: pack(sh.handle, 1, reps, ms, by)),
                 (4, lambda ms: query(sh.handle, pattern, len(pattern), reps, ms)),
                 (4, lambda ms: query(sh.handle, None, 0, reps, ms)),
                 (3, lambda ms: filt(sh.handle, C.byref(fs), 1, 1, 0, reps, ms)),
                 (3, lambda ms: filt(sh.handle, C.byref(fs), 0, 0, 1, reps, ms)),
                 (4, lambda ms: trim(sh.handle, C.byref(ts), 1, reps, ms)))
        for n, call in calls:
            if ok:
                times(n, call)
            else:
                assert call((C.c_float * n)()) == _lib.PPG_ARG_ERROR
        if ok:
            assert (sz[0], sz[1]) == (sref["records"], sref["nbytes"])
            assert sz[2] == by[1] == sum(len(raw) for _, raw, _ in chunks)
            assert sh.seqquery is None and sh.readfilter is None and sh.readtrim is None
    ms = (C.c_float * 4)()
    assert filt(sh.handle, C.byref(struct_and(fs)), 1, 0, 0, 1, ms) == _lib.PPG_ARG_ERROR
    assert trim(sh.handle, C.byref(T.struct_of(t, and_mask=True)), 1, 1, ms) == _lib.PPG_ARG_ERROR
    fref = F.filter_reference(chunks, f)
    r = sh.filter_reads(fs, mask=True, metrics=True)
    assert_filter(r, fref)
    assert np.array_equal(mask_words(r.pass_mask)[:fref["mask"].size], fref["mask"])
    assert_equals_reference(sh.trim_reads(ts, mask=True, windows=True), T.forged_reference(t))


def struct_and(f):
    s = _lib.PpgReadFilter.from_buffer_copy(f)
    s.criteria |= F.AND_MASK
    return s


# ---- 4. the cursor and BatchedFASTQ ----
def _fields(r):
    return (r.identifier, r.sequence, r.other, r.quality)


def test_trim_cursor_and_where(tmp_path, device):
    gz, cs, chunks = T.forged_gz(), T.FORGED_CHUNK, T.forged_chunks()
    f, pattern = F.FILTERS[4], b"CTC"
    p = tmp_path / "forged.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    batch_bytes = 64 << 10
    hit = Q.query_reference(chunks, pattern)["hit"]
    fpass = F.filter_reference(chunks, f)["pass"]
    recs = T.fields(chunks)
    for pat, flt, t in ((pattern, f, T.ALL), (None, None, T.ALL), (pattern, None, T.TRAIL), (None, f, T.ADAPT_FIXED)):
        tref = T.trim_reference(chunks, t)
        want = tref["keep"] & (hit if pat is not None else True) & (fpass if flt is not None else True)
        assert 0 < want.sum() < want.size, (pat, flt, t)
        ref = S.select_reference(chunks, want)
        # (the trim's AND_MASK bit is ignored: with or without it the cursor does the same)
        cur = pp.Cursor(ix, str(p), batch_bytes=batch_bytes, device=device, pattern=pat,
                        filter=None if flt is None else _lib.PpgReadFilter(*flt), trim=T.struct_of(t, and_mask=pat is None))
        assert cur.batches > 1
        scanned = nbytes = nsel = 0
        totals = np.zeros(11, np.int64)
        for b in cur:
            sel, r = b.selected, b.trim_result
            assert b.text is None and b.desc is None and b.record_base == scanned
            assert (b.filter_result is None) == (flt is None)
            lo, hi = np.searchsorted(ref["recno"], [b.record_base, b.record_base + b.nrecords])
            assert sel.records == hi - lo and lo == nsel
            assert np.array_equal(sel.recno, ref["recno"][lo:hi])
            assert np.array_equal(sel.sel_off + nbytes, ref["sel_off"][lo:hi + 1])
            assert np.array_equal(sel.desc, ref["desc"][lo:hi])
            assert np.array_equal(sel.bytes, ref["bytes"][nbytes:nbytes + sel.nbytes])
            assert sel.trim.dtype == np.uint32 and sel.trim.shape == (sel.records, 2)
            assert np.array_equal(sel.trim, tref["rows"][ref["recno"][lo:hi]])
            for i in range(sel.records):
                _, s, q = recs[int(sel.recno[i])]
                ts, tq = sel.trimmed(i)
                assert (bytes(ts), bytes(tq)) == T.slices_of(sel.trim[i], s, q), int(sel.recno[i])
            in_batch = slice(b.record_base, b.record_base + b.nrecords)
            assert (r.records, r.kept) == (b.nrecords, int(tref["keep"][in_batch].sum()))
            assert r.bases_window == int(tref["rows"][in_batch, 1].sum())
            totals += np.array([r.records, r.kept, r.trimmed] + [r.cut[c] for c in pp.ReadTrimResult.CUTS] +
                               [r.bases, r.bases_window, r.bases_kept], np.int64)
            scanned += b.nrecords
            nbytes += sel.nbytes
            nsel += sel.records
        cur.close()
        assert scanned == tref["records"] and nsel == ref["records"] and nbytes == ref["nbytes"]
        assert totals.tolist() == ([tref["records"], tref["kept"], tref["trimmed"]] + tref["cut"].tolist() +
                                   [tref["bases"], tref["bases_window"], tref["bases_kept"]])
    # trim=None gives the batches of Cursor(pattern, filter), and no trim result
    got = []
    for kw in (dict(trim=None), dict()):
        cur = pp.Cursor(ix, str(p), batch_bytes=batch_bytes, device=device, pattern=pattern, filter=_lib.PpgReadFilter(*f), **kw)
        got.append([(b.record_base, b.nrecords, b.selected.recno.copy(), b.selected.bytes.copy(), b.selected.trim,
                     b.trim_result) for b in cur])
        res, ptr = _lib.PpgReadTrimResult(), C.c_void_p()
        assert _lib.lib.ppg_cursor_trim_result(cur._h, C.byref(res)) == _lib.PPG_ARG_ERROR
        assert _lib.lib.ppg_cursor_selected_trim(cur._h, C.byref(ptr)) == _lib.PPG_ARG_ERROR
        cur.close()
    assert len(got[0]) == len(got[1]) > 1
    for a, b in zip(*got):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] is None and a[5] is None
    assert np.array_equal(np.concatenate([a[2] for a in got[0]]), np.nonzero(hit & fpass)[0])
    # before the first batch there is no window to hand out
    cur = pp.Cursor(ix, str(p), batch_bytes=batch_bytes, device=device, trim=T.struct_of(T.ALL))
    res, ptr = _lib.PpgReadTrimResult(), C.c_void_p()
    assert _lib.lib.ppg_cursor_trim_result(cur._h, C.byref(res)) == _lib.PPG_ARG_ERROR
    assert _lib.lib.ppg_cursor_selected_trim(cur._h, C.byref(ptr)) == _lib.PPG_ARG_ERROR
    cur.close()
    with pytest.raises(ValueError):
        pp.Cursor(ix, str(p), device=device, packed=True, trim=T.struct_of(T.ALL))
    # BatchedFASTQ against the text enumerator trimmed on the host by the reference's rows
    b = pp.BatchedFASTQ(ix, str(p), device=device)
    b.batch_bytes = batch_bytes
    everything = [_fields(r) for r in b]
    tref = T.trim_reference(chunks, T.ALL)
    assert len(everything) == tref["records"]
    for pat, flt, keep in ((None, None, tref["keep"]), (pattern, f, tref["keep"] & hit & fpass)):
        got = list(b.Where(pat, None if flt is None else _lib.PpgReadFilter(*flt), T.struct_of(T.ALL)))
        assert [_fields(r) for r in got] == [e for e, ok in zip(everything, keep) if ok]
        for r, j in zip(got, np.nonzero(keep)[0]):
            assert (r.trimmed_sequence, r.trimmed_quality) == T.slices_of(tref["rows"][j], recs[j][1], recs[j][2])
            assert len(r.trimmed_sequence) >= T.ALL.min_len
    assert [_fields(r) for r in b.Where(pattern)] == [e for e, h in zip(everything, hit) if h]   # the paths before: unchanged
    for cap in (pp.BatchedFASTQ.query_out_capacity, 64 << 10):          # one batch; several batches
        b.query_out_capacity = cap
        r = b.CountTrimmed(T.struct_of(T.ALL))
        assert_totals(r, tref)
        assert np.array_equal(r.chunk_kept, tref["chunk_kept"]) and r.windows is None and r.keep_mask is None
        assert b.CountPattern(pattern) == int(hit.sum())                # the query hook still works beside it
        assert b.CountPassing(_lib.PpgReadFilter(*f)).passed == int(fpass.sum())
    r = b.CountTrimmed(pp.ReadTrim(head=T.HEAD, tail=T.TAIL, leading_quality=20, trailing_quality=20, window=(4, 20),
                                   adapter=T.TRUSEQ, min_overlap=5, max_error_rate=0.1, min_length=36))
    assert_totals(r, tref)
    b.Dispose()


# ---- 5. bad trims ----
def test_bad_trims_are_argument_errors(tmp_path, device):
    import torch
    gz, cs = R.load_input("one_record")
    sh = shard_of(gz, cs, device).run()
    assert sh.trim_reads(T.struct_of(T.ALL)).records == 1
    p = tmp_path / "one.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    mask = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", device.device))
    good = T.ALL
    for bad in (good._replace(ops=0x20), good._replace(head=-1), good._replace(tail=-1), good._replace(min_len=-1),
                good._replace(qual_base=256), good._replace(trail_q=224), good._replace(win_size=33),
                good._replace(min_overlap=34), good._replace(max_err_milli=1001), good._replace(adapter=b"AC\nGTAC")):
        for call in (lambda s: sh.trim_reads(s), lambda s: sh.trim_reads(s, mask=mask), lambda s: sh.set_readtrim(s),
                     lambda s: pp.Cursor(ix, str(p), device=device, trim=s),
                     lambda s: pp.Cursor(ix, str(p), device=device, pattern=b"A", trim=s)):
            with pytest.raises(pp.PpgError) as e:
                call(T.struct_of(bad))
            assert e.value.code == _lib.PPG_ARG_ERROR, bad
    with pytest.raises(ValueError):                     # CountTrimmed / Where take the same road
        pp.ReadTrim(window=(33, 20)).struct()
    # AND_MASK needs a mask
    with pytest.raises(pp.PpgError) as e:
        sh.set_readtrim(T.struct_of(good), None, and_mask=True)
    assert e.value.code == _lib.PPG_ARG_ERROR
    assert sh.run().readtrim is None                    # none of the refused calls attached anything
