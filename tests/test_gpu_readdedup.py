"""The read dedup on the GPU (ppg_readdedup.hip through the shard ABI and the Python layer) against the reference
of the semantics (tests/readdedup_ref.py): the result, the unique mask, the first-occurrence rows, the uniques
per chunk and the table as a sorted set of rows, all exact (integer work: no tolerance).  Inputs: every golden
case, the synthetic Illumina file, and a forged file of ~35 k short reads whose copy counts hit both edges of
every duplication level; tests/test_readdedup_cpu.py guards that they are what they claim."""
import ctypes as C
import functools
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
import readprofile_ref as P
import readdedup_ref as D

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


def host_words(t):
    import torch
    return t.reshape(-1).view(torch.int32).cpu().numpy().view(np.uint32)


def dev_words(words, device):
    import torch
    return torch.from_numpy(np.array(words, np.uint32).view(np.int32)).to(torch.device("cuda", device.device))   # (a copy)


def dirty_table(slots, device):
    """A table whose every value is garbage: the call has to make it empty."""
    import torch
    return torch.full((slots, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=torch.device("cuda", device.device))


def assert_equals_reference(r, ref, mask=True, first=True):
    assert r is not None
    assert [getattr(r, k) for k in D.TOTALS] == [ref[k] for k in D.TOTALS]
    assert r.overflow == 0
    assert np.array_equal(r.level_distinct, ref["level_distinct"]) and np.array_equal(r.level_reads, ref["level_reads"])
    assert r.level_distinct.sum() == r.unique and r.level_reads.sum() == r.participating
    assert r.chunk_unique.dtype == np.int64 and np.array_equal(r.chunk_unique, ref["chunk_unique"])
    n = ref["records"]
    if mask:
        got = host_words(r.unique_mask)
        assert np.array_equal(got[:ref["mask"].size], ref["mask"]), np.flatnonzero(got[:ref["mask"].size] != ref["mask"])[:8]
    if first:
        got = r.first.cpu().numpy()[:n]
        assert np.array_equal(got, ref["first"]), np.flatnonzero(got != ref["first"])[:8]
    rows, empty_ok = D.sorted_rows(r.table.cpu().numpy())
    assert empty_ok and rows.shape == ref["table"].shape and np.array_equal(rows, ref["table"])
    assert r.duplication_rate == (1 - ref["unique"] / ref["participating"] if ref["participating"] else 0.0)


@functools.lru_cache(maxsize=None)
def golden_inputs(name):
    """(random keep words two longer than the records need, content rows) of a seqpack_ref input."""
    ch = R.oracle_chunks(name)
    n = len(T.fields(ch))
    rng = np.random.default_rng(17)
    a, b = (rng.integers(0, 1 << 32, (n + 31) // 32 + 2, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    rows = D.content_rows(ch)
    for v in (a, rows):
        v.setflags(write=False)
    return a | b, rows


@functools.lru_cache(maxsize=None)
def golden_reference(name, d, with_mask, with_rows):
    if not with_mask and not with_rows:
        return D.reference(name, d)
    words, rows = golden_inputs(name)
    ch = R.oracle_chunks(name)
    keep = D.bits_of(words, len(T.fields(ch))) if with_mask else None
    return D.dedup_reference(ch, d, keep, rows if with_rows else None, words if with_mask else None)


def run_combinations(sh, device, ref_of, words, rows, slots_list):
    """max_bases x windows x AND_MASK x slots on one shard; the mask and the rows are unchanged when only read."""
    drows = dev_words(np.asarray(rows).reshape(-1), device)
    for slots in slots_list:
        for mb in D.MAX_BASES:
            d = D.dedup(mb)
            for with_rows in (False, True):
                for with_mask in (False, True):
                    ref = ref_of(d, with_mask, with_rows)
                    mask = dev_words(words, device) if with_mask else True
                    r = sh.dedup_reads(D.struct_of(d), mask=mask, windows=drows if with_rows else None, first=True,
                                       table=dirty_table(slots, device), and_mask=with_mask)
                    assert_equals_reference(r, ref)
                    assert r.table.shape[0] == slots
    assert np.array_equal(host_words(drows), np.asarray(rows, np.uint32).reshape(-1))


# ---- 1. parity ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_dedup_reads_matches_reference(name, device):
    sh = make_shard(name, device).run()
    words, rows = golden_inputs(name)
    slots = D.min_slots(sh.total_records)
    assert 2 * sh.total_records <= slots
    run_combinations(sh, device, lambda d, m, w: golden_reference(name, d, m, w), words, rows, (slots, 4 * slots))
    # the Python layer's defaults: no mask, no first, the smallest table
    r = sh.dedup_reads(pp.ReadDedup(50))
    assert_equals_reference(r, D.reference(name, D.dedup(50)), mask=False, first=False)
    assert r.unique_mask is None and r.first is None and r.table.shape == (slots, 3)
    assert sh.readdedup is None      # no hook was attached


# ---- 2. the forged input ----
def test_forged_input(device):
    """Copy counts on both edges of every level, a 10,000-fold hot key of 1-base reads, copies next to each other,
    in one chunk, across chunks and across the carry seam, lengths 0 .. 2,100, pairs that differ in one byte, in
    length or by a unit swap, three keys that share the table's last row as their home (the probe wraps); with
    a random mask that clears first occurrences and rows that are hostile or start off a dword."""
    sh = shard_of(D.forged_gz(), D.FORGED_CHUNK, device).run()
    n = sh.total_records
    slots = D.min_slots(n)
    assert n == len(D.forged_records()) and slots == 131072
    which = {(False, False): "plain", (True, False): "mask", (False, True): "rows", (True, True): "mask_rows"}
    run_combinations(sh, device, lambda d, m, w: D.forged_reference(d, which[(m, w)]), D.forged_random_mask(),
                     D.forged_rows(), (slots, 4 * slots))


# ---- 3. capacities and arguments ----
def _buffer(device, nbytes):
    """A buffer 4 KiB larger than asked for, every byte 0xA5."""
    import torch
    t = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", device.device))
    torch.cuda.synchronize(t.device)
    return t


def _dedup_reads(sh, d, mask, mask_cap, rows, rows_cap, first, first_cap, table, slots, shift=(0, 0, 0, 0)):
    res = _lib.PpgReadDedupResult()
    ptr = lambda t, s: C.c_void_p(t.data_ptr() + s) if t is not None else None   # noqa: E731
    rc = _lib.lib.ppg_shard_dedup_reads(sh.handle, C.byref(d), ptr(mask, shift[0]), mask_cap, ptr(rows, shift[1]), rows_cap,
                                        ptr(first, shift[2]), first_cap, ptr(table, shift[3]), slots, None, C.byref(res))
    return rc, res


def test_capacities(device):
    import torch
    name = R.SYNTH
    dd = D.dedup(0)
    ref = D.reference(name, dd)
    rec = ref["records"]
    cap = (rec + 31) // 32 * 32
    slots = D.min_slots(rec)
    assert cap - 32 < rec and slots // 2 >= 64 and rec > slots // 4
    both, none = D.struct_of(dd, True, True), D.struct_of(dd)
    wonly, monly = D.struct_of(dd, False, True), D.struct_of(dd, True, False)
    sh = make_shard(name, device)
    mask, rows, first, table = _buffer(device, cap // 8), _buffer(device, 8 * rec), _buffer(device, 8 * rec), _buffer(device, 24 * slots)
    A, B = _lib.PPG_ARG_ERROR, _lib.PPG_BUF_ERROR
    call = lambda d, *a, **kw: _dedup_reads(sh, d, *a, **kw)[0]   # noqa: E731
    assert call(both, mask, cap, rows, rec, first, rec, table, slots) == A                 # before any run
    sh.run()
    device.after_torch()
    untouched = lambda: all(bool((t == 0xA5).all()) for t in (mask, rows, first, table))   # noqa: E731
    assert call(both, mask, cap + 1, rows, rec, first, rec, table, slots) == A            # mask_cap no multiple of 32
    assert call(both, mask, cap - 32, rows, rec, first, rec, table, slots) == B           # one unit short
    assert call(both, mask, cap, rows, rec - 1, first, rec, table, slots) == B            # one row short
    assert call(both, mask, cap, rows, rec, first, rec - 1, table, slots) == B            # one first row short
    assert call(both, mask, cap, rows, rec, first, rec, table, slots // 2) == B           # the table one step too small
    assert call(none, None, 0, None, 0, None, 0, table, slots // 2) == B
    assert call(both, mask, cap, rows, rec, first, rec, table, slots, shift=(2, 0, 0, 0)) == A   # misaligned: mask
    assert call(both, mask, cap, rows, rec, first, rec, table, slots, shift=(0, 4, 0, 0)) == A   # ... rows
    assert call(both, mask, cap, rows, rec, first, rec, table, slots, shift=(0, 0, 4, 0)) == A   # ... first
    assert call(both, mask, cap, rows, rec, first, rec, table, slots, shift=(0, 0, 0, 4)) == A   # ... the table
    assert call(both, mask, cap, rows, -1, first, rec, table, slots) == A
    assert call(both, mask, cap, rows, rec, first, -1, table, slots) == A
    assert call(both, None, 0, rows, rec, first, rec, table, slots) == A                  # a flag without its buffer
    assert call(both, mask, cap, None, 0, first, rec, table, slots) == A
    assert call(monly, mask, cap, rows, rec, first, rec, table, slots) == A               # a buffer without its flag
    assert call(none, None, 32, None, 0, None, 0, table, slots) == A                      # a cap without its buffer
    assert call(none, None, 0, None, rec, None, 0, table, slots) == A
    assert call(none, None, 0, None, 0, None, rec, table, slots) == A
    assert call(none, None, 0, None, 0, None, 0, table, 3 * slots // 4) == A              # not a power of two
    assert call(none, None, 0, None, 0, None, 0, table, 32) == A                          # below 64
    assert call(none, None, 0, None, 0, None, 0, table, 0) == A
    assert call(none, None, 0, None, 0, None, 0, None, slots) == A                        # no table
    bad = D.struct_of(dd)
    bad.reserved[1] = 1
    assert call(bad, None, 0, None, 0, None, 0, table, slots) == A
    assert call(D.struct_of(D.dedup(-1)), None, 0, None, 0, None, 0, table, slots) == A
    assert call(D.struct_of(D.dedup(0, 1)), None, 0, None, 0, None, 0, table, slots) == A   # an unknown flag
    assert untouched()                                                                     # ... and nothing was written
    # exact caps: the 0xA5 mask lets bits 0, 2, 5, 7 of every byte participate; the rows (0xA5A5A5A5, 0xA5A5A5A5)
    # clamp to nothing, so every participant has the empty key and the first of them is the one unique record
    prior = np.full(cap // 32, 0xA5A5A5A5, np.uint32)
    keep = D.bits_of(prior, rec)
    want = D.dedup_reference(R.oracle_chunks(name), dd, keep, np.full((rec, 2), 0xA5A5A5A5, np.uint32), prior)
    rc, res = _dedup_reads(sh, both, mask, cap, rows, rec, first, rec, table, slots)
    assert rc == 0 and (res.records, res.participating, res.unique, res.bases) == (rec, int(keep.sum()), 1, 0)
    assert (res.max_count, res.max_first, res.overflow) == (want["max_count"], 0, 0) and want["max_first"] == 0
    torch.cuda.synchronize(mask.device)
    assert np.array_equal(mask[:cap // 8].cpu().numpy().view(np.uint32), want["mask"]) and bool((mask[cap // 8:] == 0xA5).all())
    assert bool((rows == 0xA5).all())                                                       # only read
    assert np.array_equal(first[:8 * rec].cpu().numpy().view(np.int64), want["first"]) and bool((first[8 * rec:] == 0xA5).all())
    got, empty_ok = D.sorted_rows(table[:24 * slots].cpu().numpy())
    assert empty_ok and np.array_equal(got, want["table"]) and bool((table[24 * slots:] == 0xA5).all())
    # without AND_MASK the words are written whole, pad bits 0, nothing past them
    mask[:] = 0xA5
    rc, res = _dedup_reads(sh, wonly, mask, cap, rows, rec, None, 0, table, slots)
    assert rc == 0 and (res.participating, res.unique) == (rec, 1)
    words = mask[:cap // 8].cpu().numpy().view(np.uint32)
    assert words[0] == 1 and not words[1:].any() and bool((mask[cap // 8:] == 0xA5).all())
    # a multi-batch shard has no resident output to deduplicate in one call
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    assert mb.batches > 1
    total = mb.total_records                 # (a failed run below resets it)
    assert _dedup_reads(mb, none, None, 0, None, 0, None, 0, table, slots)[0] == A
    # the hook checks its caps too, the table's load among them: the run fails, nothing is ready
    dev = mask.device
    ok_table = torch.zeros((D.min_slots(total), 3), dtype=torch.int64, device=dev)
    small_table = torch.zeros((D.min_slots(total) // 2, 3), dtype=torch.int64, device=dev)
    for kw in (dict(table=small_table), dict(table=ok_table, mask=torch.zeros(total // 32 - 1, dtype=torch.int32, device=dev)),
               dict(table=ok_table, first=torch.zeros(total - 1, dtype=torch.int64, device=dev))):
        with pytest.raises(pp.PpgError) as e:
            mb.set_readdedup(D.struct_of(dd), **kw).run()
        assert e.value.code == B and mb.readdedup is None
    with pytest.raises(ValueError):
        mb.set_readdedup(D.struct_of(dd))                                                   # no table
    assert mb.set_readdedup(D.struct_of(dd), table=ok_table).run().readdedup.unique == D.reference("memlevel1_c10", dd)["unique"]


# ---- 4. the hook ----
def _hook_inputs(which):
    if which == "forged":
        return D.forged_gz(), D.FORGED_CHUNK, D.forged_chunks()
    gz, cs = R.load_input(which)
    return gz, cs, R.oracle_chunks(which)


@pytest.mark.parametrize("which", ("forged", "memlevel1_c10"))
def test_multi_batch_hook(which, device):
    """The input through an output buffer that forces several batches, deduplicated batch by batch against one
    table: the same result as the one-shot call on one batch."""
    import torch
    gz, cs, chunks = _hook_inputs(which)
    dd = D.dedup(0 if which == "forged" else 4)
    ref = D.dedup_reference(chunks, dd)
    n = ref["records"]
    assert 0 < ref["unique"] < n
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    mref = D.dedup_reference(chunks, dd, D.bits_of(words, n), None, words)
    dev = torch.device("cuda", device.device)
    plain = shard_of(gz, cs, device, out_capacity=8192).run()
    one = shard_of(gz, cs, device).run()
    assert one.batches == 1
    sh = shard_of(gz, cs, device, out_capacity=8192)
    assert sh.batches > (100 if which == "forged" else 4) and sh.readdedup is None
    slots = D.min_slots(n)
    mask = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    first = torch.full((n,), -7, dtype=torch.int64, device=dev)
    table = dirty_table(slots, device)
    sh.set_readdedup(D.struct_of(dd), mask=mask, first=first, table=table)
    assert sh.readdedup is None                    # attached, not run yet
    for _ in range(2):                             # a second run makes the table empty again and starts from 0
        sh.run()
        assert_equals_reference(sh.readdedup, ref)
    # ... which is what the one-shot call gives on one batch
    o = one.dedup_reads(D.struct_of(dd), mask=True, first=True, table=dirty_table(slots, device))
    h = sh.readdedup
    assert [getattr(o, k) for k in D.TOTALS] == [getattr(h, k) for k in D.TOTALS]
    assert np.array_equal(host_words(o.unique_mask), host_words(h.unique_mask)) and torch.equal(o.first, h.first)
    assert np.array_equal(D.sorted_rows(o.table.cpu().numpy())[0], D.sorted_rows(h.table.cpu().numpy())[0])
    # ... and the run itself is the run without the hook
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    # AND_MASK on a mask at the shard's record numbers: cleared records do not participate, later copies become first
    m = dev_words(words, device)
    assert_equals_reference(sh.set_readdedup(D.struct_of(dd), mask=m, first=first, table=table, and_mask=True).run().readdedup, mref)
    # attached after the run: nothing is ready; off: the next run leaves nothing ready
    assert sh.set_readdedup(D.struct_of(dd), table=table).readdedup is None
    assert sh.set_readdedup(None).run().readdedup is None


# ---- 5. the chain ----
def test_query_filter_trim_dedup_profile_select_chain(device):
    """The six hooks on one mask tensor and one rows tensor: the dedup sees what query, filter and trim left and
    the trim's windows; the profile and the selection see first occurrences only."""
    import torch
    name, pattern, f, t = "memlevel1_c10", b"ACG", F.GOLDEN_FILTERS[2], T.ALL._replace(min_len=60)
    dd = D.dedup(3)
    ch = R.oracle_chunks(name)
    qref, fref, tref = Q.query_reference(ch, pattern), F.reference(name, f), T.reference(name, t)
    three = qref["hit"] & fref["pass"] & tref["keep"]
    dref = D.dedup_reference(ch, dd, three, tref["rows"])
    four = dref["unique_bits"]
    assert 0 < four.sum() < three.sum() < three.size and dref["participating"] == three.sum()
    sref = S.select_reference(ch, four)
    pr = P.profile(151)
    pref = P.profile_reference(ch, pr, four, tref["rows"])
    dev = torch.device("cuda", device.device)
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    rows = torch.full((tref["records"], 2), -1, dtype=torch.int32, device=dev)
    table = dirty_table(D.min_slots(tref["records"]), device)
    out = pp.SelectedRecords.empty(sref["records"], sref["nbytes"], device.device)
    sh.set_seqquery(pattern, mask).set_readfilter(_lib.PpgReadFilter(*f), mask, and_mask=True)
    sh.set_readtrim(T.struct_of(t), mask, rows, and_mask=True)
    sh.set_readdedup(D.struct_of(dd), mask=mask, windows=rows, table=table, and_mask=True)
    sh.set_readprofile(P.struct_of(pr), mask=mask, windows=rows).set_select(mask, out)
    for _ in range(2):
        sh.run()
        assert np.array_equal(host_words(mask), F.words_of(four))
        assert_equals_reference(sh.readdedup, dref, mask=False, first=False)
        r = sh.readprofile
        assert [getattr(r, k) for k in P.TOTALS] == [pref[k] for k in P.TOTALS]
        assert all(np.array_equal(r.table[k], pref["table"][k]) for k in P.ROW_DTYPE.names)
        h = sh.selected.to_host()
        assert r.profiled == h.records == sref["records"] == dref["unique"] and h.nbytes == sref["nbytes"]
        for key in ("recno", "sel_off", "desc", "bytes"):
            assert np.array_equal(getattr(h, key), sref[key]), key
        q, rf, tr = sh.seqquery, sh.readfilter, sh.readtrim
        assert (q.records, q.hits) == (qref["records"], qref["hits"]) and rf.passed == fref["passed"]
        assert (tr.kept, tr.bases_window) == (tref["kept"], tref["bases_window"])
        assert np.array_equal(tr.windows_host(), tref["rows"])                   # the rows were only read


# ---- 6. top(k) and BatchedFASTQ.Duplication ----
def test_top_and_batched_fastq_duplication(tmp_path, device):
    gz, cs, chunks = D.forged_gz(), D.FORGED_CHUNK, D.forged_chunks()
    sh = shard_of(gz, cs, device).run()
    plain = D.forged_reference(D.dedup(0))
    r = sh.dedup_reads(pp.ReadDedup())
    for k in (1, 5, 40, 2000):
        assert r.top(k) == D.top_of(plain, k), k
    assert r.top(0) == [] and len(r.top(10 ** 6)) == plain["unique"]
    assert r.top(1) == [(r.max_count, r.max_first)] == [(10000, plain["max_first"])]
    m = sh.dedup_reads(pp.ReadDedup(1), mask=dev_words(D.forged_random_mask(), device), and_mask=True)
    assert m.top(3) == D.top_of(D.forged_reference(D.dedup(1), "mask"), 3)
    # from the file, batch by batch
    p = tmp_path / "forged.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    pattern, f, t = b"GAT", F.Filter(F.LENGTH, 10, 8192, 0, 33, 0, 20, 0), T.FIXED._replace(min_len=5)
    hit = Q.query_reference(chunks, pattern)["hit"]
    fpass = F.filter_reference(chunks, f)["pass"]
    tref = T.trim_reference(chunks, t)
    keep = hit & fpass & tref["keep"]
    assert 0 < keep.sum() < keep.size and (tref["rows"][:, 0] % 4 != 0).any()
    b = pp.BatchedFASTQ(ix, str(p), device=device)
    fs, ts = _lib.PpgReadFilter(*f), T.struct_of(t)
    for cap in (pp.BatchedFASTQ.query_out_capacity, 64 << 10):          # one batch; several batches
        b.query_out_capacity = cap
        assert_equals_reference(b.Duplication(), plain, mask=False, first=False)
        assert_equals_reference(b.Duplication(pp.ReadDedup(50)), D.forged_reference(D.dedup(50)), mask=False, first=False)
        want = D.dedup_reference(chunks, D.dedup(32), keep, tref["rows"])
        got = b.Duplication(pp.ReadDedup(32), pattern, fs, ts)
        assert_equals_reference(got, want, mask=False, first=False)
        assert np.array_equal(host_words(got.unique_mask)[:want["mask"].size], want["mask"])
        assert b.CountUnique() == plain["unique"] and b.CountUnique(pp.ReadDedup(1), pattern=pattern) == \
            D.dedup_reference(chunks, D.dedup(1), hit)["unique"]
        # the profile of the first occurrences
        pr = P.profile(64)
        pref = P.profile_reference(chunks, pr, plain["unique_bits"])
        rp = b.Profile(pp.ReadProfile(64), dedup=pp.ReadDedup())
        assert [getattr(rp, k) for k in P.TOTALS] == [pref[k] for k in P.TOTALS] and rp.profiled == plain["unique"]
        # the other counts still work beside it, and it after them
        assert b.CountPattern(pattern) == int(hit.sum()) and b.CountPassing(fs).passed == int(fpass.sum())
        assert b._query_shard().readdedup is None
        assert b.Duplication().unique == plain["unique"]
    with pytest.raises(ValueError):
        b.Duplication(pp.ReadDedup(-1))
    b.Dispose()


# ---- 7. a failed run ----
def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_readtrim.test_failed_run_leaves_hook_unready builds it, with the hook attached."""
    import torch
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    sh.set_readdedup(pp.ReadDedup(), table=torch.zeros((1 << 16, 3), dtype=torch.int64, device=torch.device("cuda", device.device)))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert sh.readdedup is None


# ---- 8. the probe hook ----
def test_probe_hook(device):
    sh = shard_of(D.forged_gz(), D.FORGED_CHUNK, device)
    slots = D.min_slots(len(D.forged_records()))
    table = dirty_table(slots, device)
    sh.set_readdedup(pp.ReadDedup(), table=table).run()
    assert sh.batches == 1 and sh.readdedup is not None
    rows = dev_words(D.forged_rows().reshape(-1), device)
    device.after_torch()
    fn = _lib.lib.ppgx_readdedup_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    tptr, wptr, wcap = C.c_void_p(table.data_ptr()), C.c_void_p(rows.data_ptr()), rows.numel() // 2
    for s, args in ((D.struct_of(D.dedup(0)), (None, 0)), (D.struct_of(D.dedup(50), False, True), (wptr, wcap))):
        ms = (C.c_float * 5)(*[-1.0] * 5)
        assert fn(sh.handle, C.byref(s), *args, tptr, slots, 1, ms) == _lib.PPG_OK
        assert all(np.isfinite(v) and v >= 0 for v in ms), list(ms)
        assert fn(sh.handle, C.byref(s), *args, tptr, slots, 0, ms) == _lib.PPG_ARG_ERROR
        assert fn(sh.handle, C.byref(s), *args, tptr, slots // 2, 1, ms) == _lib.PPG_ARG_ERROR
    assert fn(sh.handle, C.byref(D.struct_of(D.dedup(0), True, False)), None, 0, tptr, slots, 1, ms) == _lib.PPG_ARG_ERROR
    assert sh.readdedup is None                     # the pinned outputs no longer belong to a run
    # the one-shot call afterwards is unharmed
    assert_equals_reference(sh.dedup_reads(D.struct_of(D.dedup(0)), mask=True, first=True, table=table),
                            D.forged_reference(D.dedup(0)))
