"""What the GPU tests of what lies between the record stages share (tests/test_gpu_pair_emission_stages.py,
tests/test_gpu_failed_chunks.py): the seven stages chained on one mask and one rows tensor with the structs of
test_gpu_readdedup.test_query_filter_trim_dedup_profile_select_chain, their Python references chained the same
way, and Rig: one shard with keys and stages attached, every caller buffer followed by 4 KiB of 0xA5, whose
*_ready answers, results and buffers can be taken as a snapshot and compared bit for bit."""
import ctypes as C

import numpy as np

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import seqpack_ref as R
import seqquery_ref as Q
import seqselect_ref as S
import readfilter_ref as F
import readtrim_ref as T
import readprofile_ref as P
import readdedup_ref as D

KEYS = 8192
PATTERN, FLT, TRM, DD, PRF = b"ACG", F.GOLDEN_FILTERS[2], T.ALL._replace(min_len=60), D.dedup(3), P.profile(151)
STAGES = ("pack", "query", "filter", "trim", "dedup", "profile", "select")
CANARY = 4096


def references(ch, strict=True):
    """The stages' references of one file's oracle chunks, chained as the hooks chain on one mask (strict:
    every stage of the chain must take something away and leave something)."""
    qref, fref, tref = Q.query_reference(ch, PATTERN), F.filter_reference(ch, FLT), T.trim_reference(ch, TRM)
    three = qref["hit"] & fref["pass"] & tref["keep"]
    dref = D.dedup_reference(ch, DD, three, tref["rows"])
    four = dref["unique_bits"]
    assert not strict or 0 < four.sum() < three.sum() < three.size
    pack = R.pack_reference([c[1] for c in ch], [c[2] for c in ch], quality=False)
    return {"pack": pack, "query": qref, "filter": fref, "trim": tref, "dedup": dref, "bits": four,
            "select": S.select_reference(ch, four), "profile": P.profile_reference(ch, PRF, four, tref["rows"])}


class Rig:
    """One shard with keys and the stages of `which` attached, 4 KiB of 0xA5 behind every caller buffer (and
    0xA5 in it: the table and the mask start as garbage)."""

    def __init__(self, files, f, device, which=STAGES, keys=True, cap=0, n=None, on_device=False):
        """files: {"gz", "cs", "ch"} lists indexed by f (the bytes, the chunk size, the oracle chunks that size
        the buffers) and optionally "index_gz" (the bytes the index is built from when gz is corrupt); n: the
        shard's chunks (all); cap: out_capacity; on_device: the compressed range lives in a tensor of this
        rig, so load() can replace its bytes between runs."""
        import torch
        gz, cs, ch = files["gz"][f], files["cs"][f], files["ch"][f]
        self.dev = torch.device("cuda", device.device)
        ix = pp.Core.BuildDeflateIndex(files.get("index_gz", files["gz"])[f], cs)
        n = ix.Count - 1 if n is None else n
        self.lo, self.hi = ix.point_fields(0)[1] - 1, ix.point_fields(n)[1]
        comp = gz[self.lo:self.hi]
        if on_device:
            self.comp = torch.zeros(len(comp) + 64, dtype=torch.uint8, device=self.dev)
            self.load(comp)
            sh = pp.Shard(ix, self.comp.data_ptr(), 0, n, device=device, comp_on_device=True, comp_len=len(comp), out_capacity=cap)
        else:
            sh = pp.Shard(ix, np.frombuffer(comp, np.uint8), 0, n, device=device, out_capacity=cap)
        self.sh = sh
        fields = T.fields(ch)
        nrec = self.nrec = len(fields)
        nbases = sum((len(s) + 31) // 32 * 32 for _, s, _ in fields)
        nbytes = sum(len(c[1]) for c in ch)
        self.whole = {}
        words = (nrec + 31) // 32
        mask = self.buf("mask", 4 * words, torch.int32)
        rows = self.buf("rows", 8 * nrec, torch.int32).view(-1, 2)
        if keys:
            sh.set_keys(self.buf("keys", 8 * KEYS, torch.int64))
        if "pack" in which:
            self.packed = pp.PackedReads(self.buf("seq_off", 8 * (nrec + 1), torch.int64), self.buf("seq_len", 4 * nrec, torch.int32),
                                         self.buf("bases", nbases // 4, torch.int32), self.buf("nmask", nbases // 8, torch.int32))
            sh.set_seqpack(self.packed)
        if "query" in which:
            sh.set_seqquery(PATTERN, mask)
        if "filter" in which:
            sh.set_readfilter(_lib.PpgReadFilter(*FLT), mask, metrics=self.buf("metrics", 24 * nrec, torch.uint8), and_mask=True)
        if "trim" in which:
            sh.set_readtrim(T.struct_of(TRM), mask, rows, and_mask=True)
        if "dedup" in which:
            slots = D.min_slots(nrec)
            sh.set_readdedup(D.struct_of(DD), mask=mask, windows=rows, first=self.buf("first", 8 * nrec, torch.int64),
                             table=self.buf("table", 24 * slots, torch.int64).view(-1, 3), and_mask=True)
        if "profile" in which:
            sh.set_readprofile(P.struct_of(PRF), mask=mask, windows=rows)
        if "select" in which:
            self.out = pp.SelectedRecords(self.buf("sel_bytes", nbytes, torch.uint8), self.buf("sel_off", 8 * (nrec + 1), torch.int64),
                                          self.buf("sel_desc", 16 * nrec, torch.int32).view(-1, 4),
                                          self.buf("sel_recno", 8 * nrec, torch.int64), 0, 0)
            sh.set_select(mask, self.out)
        self.which = which
        torch.cuda.synchronize(self.dev)   # the buffers' fills are done before the library's stream writes them
        device.after_torch()

    def load(self, comp):
        """Replace the compressed range's bytes (on_device rigs): the next run decodes these."""
        import torch
        assert len(comp) + 64 == self.comp.numel()
        self.comp[:len(comp)].copy_(torch.from_numpy(np.frombuffer(comp, np.uint8).copy()))
        torch.cuda.synchronize(self.dev)

    def buf(self, name, nbytes, dtype):
        import torch
        whole = torch.full((nbytes + CANARY,), 0xA5, dtype=torch.uint8, device=self.dev)
        self.whole[name] = (whole, nbytes)
        return whole[:nbytes].view(dtype)

    def ready(self):
        """What the *_ready entry points answer, raw: per stage (the answer, the result's bytes, the chunk counts)."""
        lib, h, n = _lib.lib, self.sh.handle, self.sh.n
        ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        out = {"keys": lib.ppg_shard_keys_ready(h)}
        tot = C.c_int64(-1)
        out["pack"] = (lib.ppg_shard_seqpack_ready(h, C.byref(tot)), tot.value)
        for name, fn, res in (("query", lib.ppg_shard_seqquery_ready, _lib.PpgSeqQueryResult()),
                              ("filter", lib.ppg_shard_readfilter_ready, _lib.PpgReadFilterResult()),
                              ("trim", lib.ppg_shard_readtrim_ready, _lib.PpgReadTrimResult()),
                              ("dedup", lib.ppg_shard_readdedup_ready, _lib.PpgReadDedupResult())):
            ch = np.full(n, -1, np.int64)
            rc = fn(h, ptr(ch), C.byref(res))
            out[name] = (rc, bytes(res), ch.tobytes())
        res, ch, table = _lib.PpgReadProfileResult(), np.full(n, -1, np.int64), np.full((PRF.max_pos, 72), -1, np.int64)
        rc = lib.ppg_shard_readprofile_ready(h, ptr(ch), C.byref(res), ptr(table), table.shape[0])
        out["profile"] = (rc, bytes(res), ch.tobytes(), table.tobytes())
        rec, nb = C.c_int64(-1), C.c_int64(-1)
        out["select"] = (lib.ppg_shard_select_ready(h, C.byref(rec), C.byref(nb)), rec.value, nb.value)
        return out

    def answers(self):
        r = self.ready()
        return {k: (v if k == "keys" else v[0]) for k, v in r.items()}

    def snapshot(self):
        """Every ready answer and result, and every caller buffer whole (its canary with it)."""
        import torch
        torch.cuda.synchronize(self.dev)
        snap = {"ready": self.ready(), "results": {k: v.tobytes() for k, v in self.sh.results().items()},
                "total": self.sh.total_records}
        for name, (whole, nbytes) in self.whole.items():
            snap["buf:" + name] = whole.cpu().numpy().tobytes()
        return snap

    def assert_canaries(self):
        for name, (whole, nbytes) in self.whole.items():
            assert bool((whole[nbytes:] == 0xA5).all()), name

    def assert_same(self, snap, where):
        now = self.snapshot()
        assert now.keys() == snap.keys()
        for key in snap:
            if key == "ready":
                for stage in snap[key]:
                    assert now[key][stage] == snap[key][stage], (where, "ready", stage)
            else:
                assert now[key] == snap[key], (where, key)
        self.assert_canaries()

    def assert_ready(self, want, where):
        """Every attached stage answers `want` (1 ready, 0 unready); a stage that is not attached is never ready.
        (The keys are not a stage: a fused emission marks them written when their file's last batch has run.)"""
        for stage, rc in self.answers().items():
            if stage != "keys":
                assert rc == (want if stage in self.which else 0), (where, stage, rc)

    def assert_reference(self, ref):
        """Query, filter, trim, dedup, profile and selection against the Python references, exactly."""
        sh, n = self.sh, self.nrec
        assert n == ref["query"]["records"] == sh.total_records
        host = lambda name: self.whole[name][0][:self.whole[name][1]].cpu().numpy()   # noqa: E731
        assert np.array_equal(host("mask").view(np.uint32), F.words_of(ref["bits"]))
        q, qref = sh.seqquery, ref["query"]
        assert (q.records, q.hits, q.bases) == (qref["records"], qref["hits"], qref["bases"])
        assert np.array_equal(q.chunk_hits, qref["chunk_hits"]) and list(q.counts.values()) == qref["counts"].tolist()
        rf, fref = sh.readfilter, ref["filter"]
        assert (rf.records, rf.passed) == (fref["records"], fref["passed"]) and np.array_equal(rf.chunk_passed, fref["chunk_passed"])
        assert np.array_equal(host("metrics").view(F.METRICS_DTYPE), fref["metrics"])
        tr, tref = sh.readtrim, ref["trim"]
        assert (tr.records, tr.kept, tr.bases_window) == (tref["records"], tref["kept"], tref["bases_window"])
        assert np.array_equal(tr.chunk_kept, tref["chunk_kept"])
        assert np.array_equal(host("rows").view(np.uint32).reshape(-1, 2), tref["rows"])
        r, dref = sh.readdedup, ref["dedup"]
        assert [getattr(r, k) for k in D.TOTALS] == [dref[k] for k in D.TOTALS]
        assert np.array_equal(r.level_distinct, dref["level_distinct"]) and np.array_equal(r.level_reads, dref["level_reads"])
        assert np.array_equal(r.chunk_unique, dref["chunk_unique"])
        assert np.array_equal(host("first").view(np.int64), dref["first"])
        rows, empty_ok = D.sorted_rows(host("table").view(np.int64).reshape(-1, 3))
        assert empty_ok and np.array_equal(rows, dref["table"])
        rp, pref = sh.readprofile, ref["profile"]
        assert [getattr(rp, k) for k in P.TOTALS] == [pref[k] for k in P.TOTALS]
        assert all(np.array_equal(rp.table[k], pref["table"][k]) for k in P.ROW_DTYPE.names)
        assert np.array_equal(rp.chunk_profiled, pref["chunk_profiled"])
        h, sref = sh.selected.to_host(), ref["select"]
        assert h.records == sref["records"] == dref["unique"] and h.nbytes == sref["nbytes"]
        for key in ("recno", "sel_off", "desc", "bytes"):
            assert np.array_equal(getattr(h, key), sref[key]), key
        assert sh.seqpack_ready
        got, kref = self.packed.to_host(), ref["pack"]
        assert got.records == n and got.total_bases == int(kref["seq_off"][-1])
        for key in ("seq_off", "seq_len", "bases", "mask"):
            assert np.array_equal(getattr(got, key), kref[key]), key
        self.assert_canaries()


def assert_twins(rg, twins, where):
    """Shards against twins that came to the same state another way (a fused emission against a plain run, a
    run after a failed one against a first run): the same answers, results and buffers."""
    for r, t in zip(rg, twins):
        a, b = r.snapshot(), t.snapshot()
        assert a.keys() == b.keys()
        _, rec, nb = a["ready"]["select"]
        used = {"buf:sel_bytes": nb, "buf:sel_off": 8 * (rec + 1), "buf:sel_desc": 16 * rec, "buf:sel_recno": 8 * rec}
        for key in a:
            if key == "ready":
                for stage in a[key]:
                    assert a[key][stage] == b[key][stage], (where, "ready", stage)
            elif key == "buf:table":   # the rows' places depend on the insertion order of equal homes: as a set
                ra, rb = (D.sorted_rows(np.frombuffer(x, np.uint8)[:-CANARY].view(np.int64).reshape(-1, 3)) for x in (a[key], b[key]))
                assert ra[1] and rb[1] and np.array_equal(ra[0], rb[0]), (where, key)
            elif key in used:          # the selection's buffers over what is in use: what lies behind is no result
                assert a[key][:used[key]] == b[key][:used[key]], (where, key)
            else:
                assert a[key] == b[key], (where, key)
        r.assert_canaries()
