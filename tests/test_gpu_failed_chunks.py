"""Shards with failed chunks beside good ones (tests/mixed_ref.py has the inputs and the reference).

A run over such a shard goes through every batch and every hook and then returns the first failed chunk's status;
the header says what a failed chunk contributes to each stage: nothing, or no rows.  Pinned here: the run's results
(the oracle's code and 0 records for a failed chunk, the oracle's records for every other), the one-shot stage
calls on a one-batch shard after the failing run against the mixed reference, exactly -- record numbers, unit
layout, masks, rows, the table as a sorted set of rows, the selected bytes, per-chunk counts, canaries --, the
hooks of a multi-batch run (the run raises, every stage is unready, no canary is touched, the pair check refuses
the shard), and the same shard object run again on clean bytes, after which nothing of the failed run is left."""
import ctypes as C

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib, paired
import mixed_ref as M
import seqpack_ref as R
import readfilter_ref as F
import readtrim_ref as T
import readprofile_ref as P
import readdedup_ref as D
from stage_rig import CANARY, DD, FLT, PATTERN, PRF, TRM, Rig, assert_twins, references

pytestmark = pytest.mark.gpu

# (id, golden case, the shard's chunks or None for all, failed chunks)
INPUTS = [("l6_first", M.L6, None, (0,)), ("l6_last", M.L6, None, (7,)), ("l6_middle_two", M.L6, None, (3, 4)),
          ("memlevel1_five", M.MEM, None, (0, 73, 74, 75, 147)), ("l6_all_three", M.ALL_FAIL[0], M.ALL_FAIL[1], M.ALL_FAIL[2]),
          ("l6_cut_16", M.CUT[0], M.CUT[1], None)]
IDS = [i[0] for i in INPUTS]


def files_of(inp):
    """The Rig's files of one input, its failed chunks' codes, the mixed reference chunks and the clean ones."""
    _, name, n, failed = inp
    clean_gz, cs = R.load_input(name)
    if failed is None:                                   # the compressed range cut short
        part, cs, codes, mixed = M.cut_input()
        oi_lo = M.comp_bounds(M.O.build_index(clean_gz, cs), 0, n)[0]
        gz = clean_gz[:oi_lo] + part                     # (the Rig slices [lo, hi) of it: hi is past its end)
    else:
        gz, cs, codes, mixed, _ = M.mixed_input(name, tuple(failed))
    clean = R.oracle_chunks(name)
    if n is not None:
        mixed, clean = mixed[:n], clean[:n]
    return {"gz": [gz], "index_gz": [clean_gz], "cs": [cs], "ch": [clean]}, codes, mixed, clean


def assert_failing_run(sh, codes, mixed, clean):
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == codes[min(codes)]
    r = sh.results()
    want = np.array([len(c[2]) for c in mixed], np.int64)
    for k in range(sh.n):
        if k in codes:
            assert (r["status"][k], r["records"][k]) == (codes[k], 0), k
        else:
            assert (r["status"][k], r["records"][k]) == (0, len(clean[k][2])), k
    assert sh.total_records == want.sum()
    assert np.array_equal(sh.record_base(), np.concatenate([[0], np.cumsum(want)[:-1]]))


@pytest.mark.parametrize("inp", INPUTS, ids=IDS)
def test_run_reports_failed_chunks(inp, device):
    files, codes, mixed, clean = files_of(inp)
    rig = Rig(files, 0, device, which=(), keys=False, n=inp[2])
    sh = rig.sh
    assert sh.batches == 1 and sh.n == len(mixed) and all(k < sh.n for k in codes)
    assert_failing_run(sh, codes, mixed, clean)
    for k in range(sh.n):                                # the good chunks' text and descriptors are the oracle's
        if k not in codes:
            assert sh.chunk_bytes(k).tobytes() == M.chunks_text(clean)[k], k
            assert np.array_equal(sh.chunk_records(k), clean[k][2]), k


class Buffers:
    """Caller buffers with 4 KiB of 0xA5 behind each (and 0xA5 in them)."""

    def __init__(self, device):
        import torch
        self.dev = torch.device("cuda", device.device)
        self.whole = {}

    def add(self, name, nbytes):
        import torch
        self.whole[name] = (torch.full((nbytes + CANARY,), 0xA5, dtype=torch.uint8, device=self.dev), nbytes)
        return C.c_void_p(self.whole[name][0].data_ptr())

    def host(self, name, dtype):
        whole, nbytes = self.whole[name]
        return whole[:nbytes].cpu().numpy().view(dtype)

    def assert_canaries(self):
        for name, (whole, nbytes) in self.whole.items():
            assert bool((whole[nbytes:] == 0xA5).all()), name


@pytest.mark.parametrize("inp", INPUTS, ids=IDS)
def test_one_shot_stages_after_failing_run(inp, device):
    """pack, query, filter, trim, dedup, profile and selection, one call each on the one-batch shard whose run
    returned an error, chained on one mask and one rows buffer as the hooks chain: OK, and the mixed reference."""
    import torch
    files, codes, mixed, clean = files_of(inp)
    sh = Rig(files, 0, device, which=(), keys=False, n=inp[2]).sh
    assert_failing_run(sh, codes, mixed, clean)
    ref = references(mixed, strict=False)
    n, nch = sh.total_records, sh.n
    assert n == ref["query"]["records"]
    lib, h, ok = _lib.lib, sh.handle, _lib.PPG_OK
    b = Buffers(device)
    words = (n + 31) // 32
    cap = 32 * words
    nbases = int(ref["pack"]["seq_off"][-1])
    slots = D.min_slots(n)
    nbytes = sum(len(c[1]) for c in mixed)
    mask, rows = b.add("mask", 4 * words), b.add("rows", 8 * n)
    seq_off, seq_len, bases, nmask = b.add("seq_off", 8 * (n + 1)), b.add("seq_len", 4 * n), b.add("bases", nbases // 4), b.add("nmask", nbases // 8)
    metrics, first, table = b.add("metrics", 24 * n), b.add("first", 8 * n), b.add("table", 24 * slots)
    recno, sel_off, desc, sbytes = b.add("recno", 8 * n), b.add("sel_off", 8 * (n + 1)), b.add("desc", 16 * n), b.add("sel_bytes", nbytes)
    torch.cuda.synchronize(b.dev)
    device.after_torch()
    ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    failed = sorted(codes)
    counts = lambda: np.full(nch, -1, np.int64)   # noqa: E731
    mask_is = lambda bits: np.array_equal(b.host("mask", np.uint32), F.words_of(bits))   # noqa: E731
    # pack
    tot = C.c_int64(-1)
    assert lib.ppg_shard_pack_seq(h, seq_off, seq_len, n, bases, nmask, None, nbases, C.byref(tot)) == ok
    assert tot.value == nbases
    for name, key, dt in (("seq_off", "seq_off", np.int64), ("seq_len", "seq_len", np.uint32), ("bases", "bases", np.uint32),
                          ("nmask", "mask", np.uint32)):
        assert np.array_equal(b.host(name, dt), ref["pack"][key]), name
    # query
    res, ch, qref = _lib.PpgSeqQueryResult(), counts(), ref["query"]
    assert lib.ppg_shard_query_seq(h, *pp._pattern_arg(PATTERN), mask, cap, ptr(ch), C.byref(res)) == ok
    assert (res.records, res.hits, res.bases, list(res.count)) == (qref["records"], qref["hits"], qref["bases"], qref["counts"].tolist())
    assert np.array_equal(ch, qref["chunk_hits"]) and not ch[failed].any() and mask_is(qref["hit"])
    # filter, AND_MASK
    flt = _lib.PpgReadFilter(*FLT)
    flt.criteria |= _lib.PPG_FILTER_AND_MASK
    res, ch, fref = _lib.PpgReadFilterResult(), counts(), ref["filter"]
    assert lib.ppg_shard_filter_reads(h, C.byref(flt), mask, cap, metrics, n, ptr(ch), C.byref(res)) == ok
    assert (res.records, res.passed, list(res.failed)) == (fref["records"], fref["passed"], fref["failed"].tolist())
    assert (res.bases, res.other, res.qual_bytes) == (fref["bases"], fref["other"], fref["qual_bytes"])
    assert np.array_equal(np.array(res.qual_count), fref["qual_count"])
    assert np.array_equal(ch, fref["chunk_passed"]) and not ch[failed].any()
    assert np.array_equal(b.host("metrics", F.METRICS_DTYPE), fref["metrics"]) and mask_is(qref["hit"] & fref["pass"])
    # trim, AND_MASK
    res, ch, tref = _lib.PpgReadTrimResult(), counts(), ref["trim"]
    assert lib.ppg_shard_trim_reads(h, C.byref(T.struct_of(TRM, and_mask=True)), mask, cap, rows, n, ptr(ch), C.byref(res)) == ok
    assert (res.records, res.kept, res.trimmed, list(res.cut)) == (tref["records"], tref["kept"], tref["trimmed"], tref["cut"].tolist())
    assert (res.bases, res.bases_window, res.bases_kept) == (tref["bases"], tref["bases_window"], tref["bases_kept"])
    assert np.array_equal(ch, tref["chunk_kept"]) and not ch[failed].any()
    assert np.array_equal(b.host("rows", np.uint32).reshape(-1, 2), tref["rows"])
    assert mask_is(qref["hit"] & fref["pass"] & tref["keep"])
    # dedup, AND_MASK on the three, inside the trim's windows
    res, ch, dref = _lib.PpgReadDedupResult(), counts(), ref["dedup"]
    assert lib.ppg_shard_dedup_reads(h, C.byref(D.struct_of(DD, True, True)), mask, cap, rows, n, first, n, table, slots, ptr(ch),
                                     C.byref(res)) == ok
    assert [getattr(res, k) for k in D.TOTALS] == [dref[k] for k in D.TOTALS]
    assert list(res.level_distinct) == dref["level_distinct"].tolist() and list(res.level_reads) == dref["level_reads"].tolist()
    assert np.array_equal(ch, dref["chunk_unique"]) and not ch[failed].any()
    assert np.array_equal(b.host("first", np.int64), dref["first"]) and mask_is(ref["bits"])
    got, empty_ok = D.sorted_rows(b.host("table", np.int64).reshape(-1, 3))
    assert empty_ok and np.array_equal(got, dref["table"])
    # profile over the mask and the rows
    res, ch, tab, pref = _lib.PpgReadProfileResult(), counts(), np.full((PRF.max_pos, 72), -1, np.int64), ref["profile"]
    assert lib.ppg_shard_profile_reads(h, C.byref(P.struct_of(PRF, True, True)), mask, cap, rows, n, ptr(ch), C.byref(res), ptr(tab),
                                       tab.shape[0]) == ok
    assert [getattr(res, k) for k in P.TOTALS] == [pref[k] for k in P.TOTALS]
    assert list(res.gc_hist) == pref["gc_hist"].tolist() and list(res.meanq_hist) == pref["meanq_hist"].tolist()
    assert tab.tobytes() == pref["table"].tobytes()
    assert np.array_equal(ch, pref["chunk_profiled"]) and not ch[failed].any()
    # the selection of what is left
    srec, snb, sref = C.c_int64(-1), C.c_int64(-1), ref["select"]
    assert lib.ppg_shard_select_records(h, mask, cap, recno, sel_off, desc, n, sbytes, nbytes, C.byref(srec), C.byref(snb)) == ok
    S_, B_ = sref["records"], sref["nbytes"]
    assert (srec.value, snb.value) == (S_, B_)
    assert np.array_equal(b.host("recno", np.int64)[:S_], sref["recno"]) and np.array_equal(b.host("sel_off", np.int64)[:S_ + 1], sref["sel_off"])
    assert np.array_equal(b.host("desc", np.uint32).reshape(-1, 4)[:S_], sref["desc"])
    assert np.array_equal(b.host("sel_bytes", np.uint8)[:B_], sref["bytes"])
    assert (b.host("recno", np.uint8)[8 * S_:] == 0xA5).all() and (b.host("sel_bytes", np.uint8)[B_:] == 0xA5).all()
    # nothing but the mask, the table, first and the selection was written by the later calls
    assert np.array_equal(b.host("rows", np.uint32).reshape(-1, 2), tref["rows"]) and mask_is(ref["bits"])
    b.assert_canaries()


MULTI = [(INPUTS[3], 8192, 5), (INPUTS[2], 48 << 10, 5)]   # (input, out_capacity, at least this many batches)


@pytest.mark.parametrize("inp,cap,least", MULTI, ids=["memlevel1_five", "l6_middle_two"])
def test_hooks_of_a_failing_multi_batch_run(inp, cap, least, device):
    """Keys and the seven stages attached, several batches, failed chunks among them: the run raises the lowest
    failed chunk's status after every batch and every hook ran, every stage is unready, no canary is touched and
    the pair check refuses the shard.  Then the same shard object runs on the clean bytes: the hooks' results are
    the clean references and bit for bit those of a twin that never saw the corrupt bytes."""
    files, codes, mixed, clean = files_of(inp)
    rig = Rig(files, 0, device, cap=cap, on_device=True)
    assert rig.sh.batches >= least
    assert_failing_run(rig.sh, codes, mixed, clean)
    rig.assert_ready(0, "failed run")
    assert rig.answers()["keys"] == 0
    rig.assert_canaries()
    pr = paired.Pairs()
    with pytest.raises(pp.PpgError) as e:
        pr.check(rig.sh, rig.sh)
    assert e.value.code == _lib.PPG_ARG_ERROR
    # recovery: the clean bytes into the same shard object
    clean_files = dict(files, gz=files["index_gz"])
    rig.load(clean_files["gz"][0][rig.lo:rig.hi])
    rig.sh.run()
    rig.assert_ready(1, "clean run")
    assert rig.answers()["keys"] == 1
    rig.assert_reference(references(clean))
    twin = Rig(clean_files, 0, device, cap=cap)
    twin.sh.run()
    assert_twins([rig], [twin], "the clean run after the failed one")
    assert pr.check(rig.sh, twin.sh)["mismatches"] == 0


def test_range_lengths(device):
    """What ppg_shard_create takes for comp_len: the index's, or less down to 8 bytes into the last chunk's own
    bytes (that chunk then fails with the oracle's status on the same slice, the others are exact); a byte more
    than the index's, or a range that ends before that, is PPG_ARG_ERROR."""
    name, n = M.CUT[0], M.CUT[1]
    gz, cs = R.load_input(name)
    oi = M.O.build_index(gz, cs)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    clean = R.oracle_chunks(name)[:n]
    lo, hi = M.comp_bounds(oi, 0, n)
    least = oi.point(n - 1)[1] - oi.point(0)[1] + 8
    make = lambda length: pp.Shard(ix, np.frombuffer(gz[lo:lo + length], np.uint8), 0, n, device=device)   # noqa: E731
    for length in (hi - lo + 1, least - 1, 0):
        with pytest.raises(pp.PpgError) as e:
            make(length)
        assert e.value.code == _lib.PPG_ARG_ERROR, length
    assert make(hi - lo).run().total_records == sum(len(c[2]) for c in clean)
    sh = make(least)
    with pytest.raises(M.O.OracleError) as oe:
        M.extract_until(gz, oi, n - 1, lo + least)
    assert_failing_run(sh, {n - 1: oe.value.code}, M.mixed_chunks(clean, {n - 1}), clean)


def test_failing_fused_emission_leaves_stages_unready(device):
    """ppg_pairs_emit_run over a good shard and one with failed chunks, all hooks attached: the emission ends with
    the failed chunk's status when that shard's last batch has run, and no stage of either shard is ready."""
    files, codes, mixed, clean = files_of(INPUTS[2])
    good = Rig(dict(files, gz=files["index_gz"]), 0, device, cap=48 << 10)
    bad = Rig(files, 0, device, cap=48 << 10)
    assert good.sh.batches >= 5 and bad.sh.batches >= 5
    good.sh.run()                                    # (ready before: the emission has to take that back)
    good.assert_ready(1, "plain run")
    pr = paired.Pairs()
    with pytest.raises(pp.PpgError) as e:
        for _ in pr.emit_run(good.sh, bad.sh, 500):
            pass
    assert e.value.code == codes[min(codes)]
    for r in (good, bad):
        r.assert_ready(0, "failed fused run")
        r.assert_canaries()
    assert bad.answers()["keys"] == 0
