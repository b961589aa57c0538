"""The read profile on the GPU (ppg_readprofile.hip through the shard ABI and the Python layer) against the
reference of the semantics (tests/readprofile_ref.py): the table, the fixed result and the profiled records
per chunk, all exact (integer work: no tolerance).  Inputs: every golden case, the synthetic Illumina file,
and the read trim's forged file with records at the unit, wave and block boundaries of the kernels' unit map;
tests/test_readprofile_cpu.py guards that they are what they claim."""
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
import readprofile_ref as P

pytestmark = pytest.mark.gpu

POSITIONS = (1, 32, 33, 151, 1024)


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
    return torch.from_numpy(np.array(words, np.uint32).view(np.int32)).to(torch.device("cuda", device.device))   # (a copy)


def set_grid(sh, blocks):
    fn = _lib.lib.ppgx_readprofile_grid
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(sh.handle, blocks) == _lib.PPG_OK


def assert_equals_reference(r, ref):
    assert r is not None
    assert [getattr(r, k) for k in P.TOTALS] == [ref[k] for k in P.TOTALS]
    assert r.chunk_profiled.dtype == np.int64 and np.array_equal(r.chunk_profiled, ref["chunk_profiled"])
    assert np.array_equal(r.gc_hist, ref["gc_hist"]), (np.nonzero(r.gc_hist != ref["gc_hist"])[0])
    assert np.array_equal(r.meanq_hist, ref["meanq_hist"]), (np.nonzero(r.meanq_hist != ref["meanq_hist"])[0])
    assert r.table.shape == ref["table"].shape
    for f in P.ROW_DTYPE.names:
        bad = np.argwhere(r.table[f] != ref["table"][f])
        assert bad.size == 0, (f, bad[:8].tolist(), r.table[f][tuple(bad[0])], ref["table"][f][tuple(bad[0])])


# ---- 1. parity ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_profile_reads_matches_reference(name, device):
    sh = make_shard(name, device).run()
    for pos in POSITIONS:
        p = P.profile(pos)
        assert_equals_reference(sh.profile_reads(P.struct_of(p)), P.reference(name, p))
    assert_equals_reference(sh.profile_reads(pp.ReadProfile(151, 40)), P.reference(name, P.profile(151, 40)))
    assert sh.readprofile is None      # no hook was attached


# ---- 2. the forged input ----
@pytest.mark.parametrize("grid", (0, 1, 3))
@pytest.mark.parametrize("which", ("plain", "trim", "random", "hostile", "random_hostile"))
def test_forged_input(which, grid, device):
    """Records at the unit, wave and block boundaries, empty Sequences, Quality lines one short, 40 long and
    empty, records across the carry seam; with the trim's rows and keep mask, a random mask two words longer
    than the records, and rows that start past the read or run past its end.  One block loops over every
    tile, three get uneven shares; 1,024 positions go past the quality rows held in LDS."""
    sh = shard_of(T.forged_gz(), T.FORGED_CHUNK, device).run()
    n = sh.total_records
    mask = rows = None
    if which == "trim":
        t = sh.trim_reads(T.struct_of(T.ALL), mask=True, windows=True)
        assert t.kept == T.forged_reference(T.ALL)["kept"]
        mask, rows = t.keep_mask, t.windows
    if which in ("random", "random_hostile"):
        mask = dev_words(P.forged_random_mask(), device)
    if which in ("hostile", "random_hostile"):
        rows = dev_words(P.forged_hostile_rows().reshape(-1), device)
    before = (None if mask is None else mask_words(mask).copy(), None if rows is None else mask_words(rows.reshape(-1)).copy())
    set_grid(sh, grid)
    for pos in (1024, 33):
        p = P.profile(pos)
        assert_equals_reference(sh.profile_reads(P.struct_of(p), mask=mask, windows=rows), P.forged_reference(p, which))
    # the mask and the rows are only read
    assert mask is None or np.array_equal(mask_words(mask), before[0])
    assert rows is None or np.array_equal(mask_words(rows.reshape(-1)), before[1])
    assert n == P.forged_reference(P.profile(33))["records"]


# ---- 3. capacities and arguments ----
def _buffer(device, nbytes):
    """A buffer 4 KiB larger than asked for, every byte 0xA5."""
    import torch
    t = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", device.device))
    torch.cuda.synchronize(t.device)
    return t


def _profile_reads(sh, p, mask, mask_cap, rows, rows_cap, table=None, table_cap=0, shift=0, mshift=0):
    res = _lib.PpgReadProfileResult()
    rc = _lib.lib.ppg_shard_profile_reads(
        sh.handle, C.byref(p), C.c_void_p(mask.data_ptr() + mshift) if mask is not None else None, mask_cap,
        C.c_void_p(rows.data_ptr() + shift) if rows is not None else None, rows_cap, None, C.byref(res),
        table.ctypes.data_as(C.c_void_p) if table is not None else None, table_cap)
    return rc, res


def test_capacities(device):
    import torch
    name = R.SYNTH
    pr = P.profile(151)
    ref = P.reference(name, pr)
    rec = ref["records"]
    cap = (rec + 31) // 32 * 32
    assert cap - 32 < rec
    both, none = P.struct_of(pr, True, True), P.struct_of(pr)
    sh = make_shard(name, device)
    mask, rows = _buffer(device, cap // 8), _buffer(device, 8 * rec)
    table = np.full((151 + 1, 72), -7, np.int64)
    A, B = _lib.PPG_ARG_ERROR, _lib.PPG_BUF_ERROR
    assert _profile_reads(sh, both, mask, cap, rows, rec, table, 151)[0] == A              # before any run
    sh.run()
    device.after_torch()
    untouched = lambda: bool((mask == 0xA5).all()) and bool((rows == 0xA5).all()) and bool((table == -7).all())  # noqa: E731
    assert _profile_reads(sh, both, mask, cap + 1, rows, rec, table, 151)[0] == A          # mask_cap no multiple of 32
    assert _profile_reads(sh, both, mask, cap - 32, rows, rec, table, 151)[0] == B         # one unit short
    assert _profile_reads(sh, both, mask, cap, rows, rec - 1, table, 151)[0] == B          # one row short
    assert _profile_reads(sh, both, mask, cap, rows, rec, table, 150)[0] == B              # one table row short
    assert _profile_reads(sh, none, None, 0, None, 0, table, 150)[0] == B
    assert _profile_reads(sh, both, mask, cap, rows, rec, table, 151, shift=4)[0] == A     # rows not 8-byte aligned
    assert _profile_reads(sh, both, mask, cap, rows, rec, table, 151, mshift=2)[0] == A    # mask not 4-byte aligned
    assert _profile_reads(sh, both, mask, cap, rows, -1, table, 151)[0] == A
    assert _profile_reads(sh, both, None, 0, rows, rec, table, 151)[0] == A                # a flag without its buffer
    assert _profile_reads(sh, both, mask, cap, None, 0, table, 151)[0] == A
    assert _profile_reads(sh, none, mask, cap, None, 0, table, 151)[0] == A                # a buffer without its flag
    assert _profile_reads(sh, none, None, 0, rows, rec, table, 151)[0] == A
    assert _profile_reads(sh, none, None, 32, None, 0, table, 151)[0] == A                 # a cap without its buffer
    assert _profile_reads(sh, none, None, 0, None, rec, table, 151)[0] == A
    assert _profile_reads(sh, P.struct_of(pr._replace(max_pos=1025)), None, 0, None, 0, table, 151)[0] == A
    assert untouched()                                                                      # ... and nothing was written
    # exact caps: the 0xA5 mask selects bits 0, 2, 5, 7 of every byte; the rows (0xA5A5A5A5, 0xA5A5A5A5) clamp to nothing
    keep = P.bits_of(np.full(cap // 32, 0xA5A5A5A5, np.uint32), rec)
    want = P.profile_reference(R.oracle_chunks(name), pr, keep, np.full((rec, 2), 0xA5A5A5A5, np.uint32))
    rc, res = _profile_reads(sh, both, mask, cap, rows, rec, table, 151)
    assert rc == 0 and (res.records, res.profiled, res.bases) == (rec, want["profiled"], 0) and want["profiled"] == keep.sum()
    assert table[0, 7] == want["profiled"] and (table[151] == -7).all() and table[:151].sum() == want["profiled"]
    assert bool((mask == 0xA5).all()) and bool((rows == 0xA5).all())                        # only read
    rc, res = _profile_reads(sh, none, None, 0, None, 0, None, 0)                           # no table asked for
    assert rc == 0 and (res.records, res.profiled, res.bases) == (rec, rec, ref["bases"])
    # a multi-batch shard has no resident output to profile in one call
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    assert mb.batches > 1
    total = mb.total_records                 # (a failed run below resets it)
    assert _profile_reads(mb, none, None, 0, None, 0, table, 151)[0] == A
    # the hook checks its caps too: the run fails, nothing is ready
    small = torch.zeros(total // 32 - 1, dtype=torch.int32, device=mask.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_readprofile(P.struct_of(pr), mask=small).run()
    assert e.value.code == B and mb.readprofile is None
    few = torch.zeros(2 * (total - 1), dtype=torch.int32, device=mask.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_readprofile(P.struct_of(pr), windows=few).run()
    assert e.value.code == B and mb.readprofile is None
    # ... and _ready refuses a table that is too small, then fills one that fits
    mb.set_readprofile(P.struct_of(pr)).run()
    res = _lib.PpgReadProfileResult()
    ready = _lib.lib.ppg_shard_readprofile_ready
    table[:] = -7
    assert ready(mb.handle, None, C.byref(res), table.ctypes.data_as(C.c_void_p), 150) == B and (table == -7).all()
    assert ready(mb.handle, None, C.byref(res), table.ctypes.data_as(C.c_void_p), 151) == 1
    assert np.array_equal(table[:151].view(P.ROW_DTYPE).reshape(-1)["base"], P.reference("memlevel1_c10", pr)["table"]["base"])


# ---- 4. the hook ----
def _hook_inputs(which):
    if which == "forged":
        return T.forged_gz(), T.FORGED_CHUNK, T.forged_chunks(), 64 << 10
    gz, cs = R.load_input(which)
    return gz, cs, R.oracle_chunks(which), 8192


@pytest.mark.parametrize("which", ("forged", "memlevel1_c10"))
def test_multi_batch_hook(which, device):
    """The input through an output buffer that forces several batches, profiled batch by batch."""
    gz, cs, chunks, cap = _hook_inputs(which)
    pr = P.profile(151)
    ref = P.profile_reference(chunks, pr)
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, (ref["records"] + 31) // 32, dtype=np.uint64).astype(np.uint32)
    mref = P.profile_reference(chunks, pr, P.bits_of(words, ref["records"]))
    plain = shard_of(gz, cs, device, out_capacity=cap).run()
    sh = shard_of(gz, cs, device, out_capacity=cap)
    assert sh.batches > (4 if which == "memlevel1_c10" else 2) and sh.readprofile is None
    sh.set_readprofile(P.struct_of(pr))
    assert sh.readprofile is None                  # attached, not run yet
    for _ in range(2):                             # a second run starts its accumulators from 0 again
        sh.run()
        assert_equals_reference(sh.readprofile, ref)
    # ... and the run itself is the run without the hook
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    for k in range(sh.n):
        assert np.array_equal(plain.chunk_records(k), sh.chunk_records(k)), k
    # a mask at the shard's record numbers, through one block per batch
    set_grid(sh, 1)
    assert_equals_reference(sh.set_readprofile(P.struct_of(pr), mask=dev_words(words, device)).run().readprofile, mref)
    set_grid(sh, 0)
    # attached after the run: nothing is ready; off: the next run leaves nothing ready
    assert sh.set_readprofile(P.struct_of(pr)).readprofile is None
    assert sh.set_readprofile(None).run().readprofile is None


# ---- 5. the chain ----
def test_query_filter_trim_profile_select_chain(device):
    """The five hooks on one mask tensor and one rows tensor: the profile reads what query, filter and trim
    left, which is what the selection hands over; every other stage's result is its own."""
    import torch
    name, pattern, f, t = "memlevel1_c10", b"GATTAC", F.GOLDEN_FILTERS[2], T.ALL._replace(min_len=60)
    ch = R.oracle_chunks(name)
    qref, fref, tref = Q.reference(name, pattern), F.reference(name, f), T.reference(name, t)
    three = qref["hit"] & fref["pass"] & tref["keep"]
    assert 0 < three.sum() < three.size
    sref = S.select_reference(ch, three)
    pr = P.profile(151)
    pref = P.profile_reference(ch, pr, three, tref["rows"])
    dev = torch.device("cuda", device.device)
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    rows = torch.full((tref["records"], 2), -1, dtype=torch.int32, device=dev)
    out = pp.SelectedRecords.empty(sref["records"], sref["nbytes"], device.device)
    sh.set_seqquery(pattern, mask).set_readfilter(_lib.PpgReadFilter(*f), mask, and_mask=True)
    sh.set_readtrim(T.struct_of(t), mask, rows, and_mask=True).set_readprofile(P.struct_of(pr), mask=mask, windows=rows)
    sh.set_select(mask, out)
    for _ in range(2):
        sh.run()
        assert np.array_equal(mask_words(mask), F.words_of(three))
        assert_equals_reference(sh.readprofile, pref)
        h = sh.selected.to_host()
        assert sh.readprofile.profiled == h.records == sref["records"] and h.nbytes == sref["nbytes"]
        for key in ("recno", "sel_off", "desc", "bytes"):
            assert np.array_equal(getattr(h, key), sref[key]), key
        q, r, tr = sh.seqquery, sh.readfilter, sh.readtrim
        assert (q.records, q.hits, q.bases) == (qref["records"], qref["hits"], qref["bases"])
        assert [q.counts[c] for c in pp.SeqQuery.CLASSES] == qref["counts"].tolist()
        assert np.array_equal(q.chunk_hits, qref["chunk_hits"])
        assert (r.records, r.passed, r.bases) == (fref["records"], fref["passed"], fref["bases"])
        assert np.array_equal(r.chunk_passed, fref["chunk_passed"]) and np.array_equal(r.qual_count, fref["qual_count"])
        assert (tr.records, tr.kept, tr.trimmed, tr.bases_window) == (tref["records"], tref["kept"], tref["trimmed"], tref["bases_window"])
        assert np.array_equal(tr.chunk_kept, tref["chunk_kept"]) and np.array_equal(tr.windows_host(), tref["rows"])


# ---- 6. BatchedFASTQ.Profile ----
def test_batched_fastq_profile(tmp_path, device):
    gz, cs, chunks = T.forged_gz(), T.FORGED_CHUNK, T.forged_chunks()
    f, pattern = F.FILTERS[4], b"CTC"
    p = tmp_path / "forged.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    hit = Q.query_reference(chunks, pattern)["hit"]
    fpass = F.filter_reference(chunks, f)["pass"]
    tref = T.trim_reference(chunks, T.ALL)
    pr = P.profile(160)
    b = pp.BatchedFASTQ(ix, str(p), device=device)
    fs, ts = _lib.PpgReadFilter(*f), T.struct_of(T.ALL)
    for cap in (pp.BatchedFASTQ.query_out_capacity, 64 << 10):          # one batch; several batches
        b.query_out_capacity = cap
        assert_equals_reference(b.Profile(pp.ReadProfile(160)), P.profile_reference(chunks, pr))
        assert_equals_reference(b.Profile(), P.profile_reference(chunks, P.profile(256)))
        keep = hit & fpass & tref["keep"]
        assert 0 < keep.sum() < keep.size
        assert_equals_reference(b.Profile(pp.ReadProfile(160), pattern, fs, ts), P.profile_reference(chunks, pr, keep, tref["rows"]))
        assert_equals_reference(b.Profile(pp.ReadProfile(160), pattern=pattern), P.profile_reference(chunks, pr, hit))
        assert_equals_reference(b.Profile(pp.ReadProfile(160), filter=fs), P.profile_reference(chunks, pr, fpass))
        assert_equals_reference(b.Profile(pp.ReadProfile(160), trim=ts), P.profile_reference(chunks, pr, tref["keep"], tref["rows"]))
        # the other counts still work beside it, and it after them
        assert b.CountPattern(pattern) == int(hit.sum())
        assert b.CountPassing(fs).passed == int(fpass.sum())
        assert b.CountTrimmed(ts).kept == tref["kept"]
        assert b._query_shard().readprofile is None
        assert_equals_reference(b.Profile(pp.ReadProfile(160)), P.profile_reference(chunks, pr))
    with pytest.raises(ValueError):
        b.Profile(pp.ReadProfile(2000))
    b.Dispose()


# ---- 7. a failed run ----
def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_readtrim.test_failed_run_leaves_hook_unready builds it, with the hook attached."""
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    sh.set_readprofile(pp.ReadProfile(151))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert sh.readprofile is None


# ---- 8. the probe hook ----
def test_probe_hook(device):
    chunks = T.forged_chunks()
    sh = shard_of(T.forged_gz(), T.FORGED_CHUNK, device)
    sh.set_readprofile(pp.ReadProfile(160)).run()
    assert sh.batches == 1 and sh.readprofile is not None
    t = sh.trim_reads(T.struct_of(T.ALL), mask=True, windows=True)
    device.after_torch()
    fn = _lib.lib.ppgx_readprofile_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    mptr, mcap = C.c_void_p(t.keep_mask.data_ptr()), 32 * t.keep_mask.numel()
    wptr, wcap = C.c_void_p(t.windows.data_ptr()), t.windows.shape[0]
    for pos in (160, 1024):
        for s, args in ((P.struct_of(P.profile(pos)), (None, 0, None, 0)),
                        (P.struct_of(P.profile(pos), True, True), (mptr, mcap, wptr, wcap))):
            ms = (C.c_float * 3)(-1.0, -1.0, -1.0)
            assert fn(sh.handle, C.byref(s), *args, 1, ms) == _lib.PPG_OK
            assert all(np.isfinite(v) and v >= 0 for v in ms), list(ms)
            assert fn(sh.handle, C.byref(s), *args, 0, ms) == _lib.PPG_ARG_ERROR
    assert fn(sh.handle, C.byref(P.struct_of(P.profile(160), True, False)), None, 0, None, 0, 1, ms) == _lib.PPG_ARG_ERROR
    assert sh.readprofile is None                   # the pinned outputs no longer belong to a run
    # the one-shot call afterwards is unharmed
    pr = P.profile(160)
    assert_equals_reference(sh.profile_reads(P.struct_of(pr)), P.profile_reference(chunks, pr))
    assert_equals_reference(sh.profile_reads(P.struct_of(pr), mask=t.keep_mask, windows=t.windows),
                            P.forged_reference(pr, "trim"))
