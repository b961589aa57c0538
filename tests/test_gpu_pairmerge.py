"""The pair merge on the GPU (ppg_pairmerge.hip through the C ABI and the Python layer) against the reference of
the semantics (tests/pairmerge_ref.py): the merged set's planes word for word, pair_of, the counters and the merged
reads as strings, all exact (integer work: no tolerance).  Inputs: the forge of read pairs with forged qualities
under every parameter set and map (tests/test_pairmerge_cpu.py guards that it is what it claims), hostile rows, and
a forged R1 / R2 pair of .gz files through PairedFASTQ."""
import ctypes as C

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib, paired
import pairmerge_ref as M
import pairoverlap_ref as V
import readtrim_ref as T

pytestmark = pytest.mark.gpu

A, B = _lib.PPG_ARG_ERROR, _lib.PPG_BUF_ERROR
GUARD = 4096          # canary bytes past every buffer
I32 = np.iinfo(np.int32)


def tdev(device):
    import torch
    return torch.device("cuda", device.device)


def to_device(reads, quals, device):
    """Lists of reads and qualities as a PackedReads of CUDA tensors, packed by the reference of the format."""
    import torch
    h = M.pack_strings(reads, quals)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).to(tdev(device))  # noqa: E731
    return pp.PackedReads(t(h["seq_off"]), t(h["seq_len"]), t(h["bases"]), t(h["mask"]), t(h["qual"]), len(reads),
                          int(h["seq_off"][-1]))


_sets = {}


def forge_on_device(which, device):
    """(packed1, packed2, rec1, rec2 as CUDA tensors or None) of the forge with its qualities under a map; made once."""
    import torch
    if which not in _sets:
        set1, qual1, set2, qual2, rec1, rec2 = M.forge_sets(which)
        m = lambda r: None if r is None else torch.from_numpy(r.copy()).to(tdev(device))   # noqa: E731
        _sets[which] = (to_device(set1, qual1, device), to_device(set2, qual2, device), m(rec1), m(rec2))
    return _sets[which]


def rows_on_device(rows, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, np.int32).copy()).to(tdev(device))


def assert_planes(host, ref, quality=True):
    """A host PackedReads cut to its records against the reference's planes, word for word."""
    n, nb = ref["merged"], ref["padded_bases"]
    assert host.records == n and host.total_bases == nb
    assert np.array_equal(host.seq_off, ref["seq_off"]) and np.array_equal(host.seq_len, ref["seq_len"])
    for name in ("bases", "mask") + (("qual",) if quality else ()):
        got, want = getattr(host, name), ref[name]
        assert got.shape == want.shape, name
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert quality or host.qual is None


def assert_equals_reference(r, ref, quality=True, pair_of=True, strings=True):
    assert [getattr(r, k) for k in M.TOTALS] == [ref[k] for k in M.TOTALS], [(k, getattr(r, k), ref[k]) for k in M.TOTALS]
    assert r.corrected == ref["corrected"]
    assert r.agree == ref["overlap_bases"] - ref["disagree"] - ref["n_filled"] - ref["n_both"]
    host = r.reads.to_host()
    assert_planes(host, ref, quality)
    if pair_of:
        assert np.array_equal(r.pair_of.cpu().numpy(), ref["pair_of"])
    else:
        assert r.pair_of is None
    if strings:
        for j, (s, q) in enumerate(zip(ref["seqs"], ref["quals"])):
            assert host.sequence(j) == s, j
            if quality:
                assert host.quality(j) == q, j


def set_grid(device, blocks):
    fn = _lib.lib.ppgx_pairmerge_grid
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(device.handle, blocks) == _lib.PPG_OK


# ---- 1. parity on the forge ----
@pytest.mark.parametrize("which", ["identity", "permutation", "holes"])
@pytest.mark.parametrize("pname", ["defaults", "exact", "always"])
def test_forge_matches_reference(pname, which, device):
    p1, p2, rec1, rec2 = forge_on_device(which, device)
    ov = V.forge_reference(pname, which, windows=False)
    ref = M.forge_reference(pname, which)
    rows = rows_on_device(ov["rows"], device)
    r = pp.pair_merge(p1, p2, rows, pp.PairMerge(), rec1, rec2, device=device)
    assert_equals_reference(r, ref)
    assert r.merged == ov["found"] > 0 and r.overlap_bases == ov["overlap_bases"]      # the identities with the overlap
    assert r.disagree + r.n_filled + r.n_both == ov["mismatches"]
    assert r.reads.rec_cap == ref["merged"] and r.reads.base_cap == ref["padded_bases"]   # sized exactly
    # without the output's quality plane and pair_of: the same choice
    r = pp.pair_merge(p1, p2, rows, None, rec1, rec2, quality=False, pair_of=False, device=device)
    assert_equals_reference(r, ref, quality=False, pair_of=False, strings=False)
    # the rows the overlap kernel writes are the reference's: merging them is the same
    o = pp.pair_overlap(p1, p2, pp.PairOverlap(*V.PARAM_SETS[pname]), rec1, rec2, found_mask=False, device=device)
    assert np.array_equal(o.rows.cpu().numpy(), ov["rows"])
    assert_equals_reference(pp.pair_merge(p1, p2, o.rows, None, rec1, rec2, device=device), ref, strings=False)


def test_other_thresholds(device):
    """qual_hi / qual_lo change corrected and nothing else."""
    p1, p2, _, _ = forge_on_device("identity", device)
    rows = rows_on_device(V.forge_reference("always", "identity", windows=False)["rows"], device)
    base = M.forge_reference("always")
    for m in (M.Merge(70, 40), M.Merge(255, 0), M.Merge(1, 0), M.Merge(36, 35)):
        ref = M.forge_reference("always", "identity", m)
        assert ref["corrected"] != base["corrected"] and ref["seqs"] == base["seqs"]
        assert_equals_reference(pp.pair_merge(p1, p2, rows, pp.PairMerge(*m), device=device), ref, strings=False)


# ---- 2. grids agree ----
def test_grids_agree(device):
    """The default grid, one block (which loops over every unit) and three blocks (uneven shares)."""
    p1, p2, rec1, rec2 = forge_on_device("holes", device)
    ref = M.forge_reference("defaults", "holes")
    rows = rows_on_device(V.forge_reference("defaults", "holes", windows=False)["rows"], device)
    try:
        for blocks in (0, 1, 3):
            set_grid(device, blocks)
            assert_equals_reference(pp.pair_merge(p1, p2, rows, None, rec1, rec2, device=device), ref, strings=False)
    finally:
        set_grid(device, 0)
    fn = _lib.lib.ppgx_pairmerge_grid
    assert fn(device.handle, -1) == A and fn(None, 1) == A


# ---- 3 / 4. the C entry points: hostile rows, capacities, arguments ----
class Call:
    """The buffers of one ppg_pairs_merge call on the forge, each filled with 0xA5 and with GUARD bytes behind it,
    and the call with any argument replaced.  rec_cap / base_cap: the output's capacities."""

    def __init__(self, device, rows, rec_cap, base_cap, rec1=None):
        import torch
        self.device = device
        self.p1, self.p2, _, _ = forge_on_device("identity", device)
        self.n = self.p1.records
        self.rec_cap, self.base_cap = rec_cap, base_cap
        self.rows = rows_on_device(rows, device)
        self.rec1 = None if rec1 is None else torch.from_numpy(rec1.copy()).to(tdev(device))
        self.sizes = {"seq_off": 8 * (rec_cap + 1), "seq_len": 4 * rec_cap, "bases": base_cap // 4, "mask": base_cap // 8,
                      "qual": base_cap, "pair_of": 8 * rec_cap}
        self.buf = {k: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device=tdev(device)) for k, v in self.sizes.items()}
        self.views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                         p.qual.data_ptr(), p.records) for p in (self.p1, self.p2)]
        self.res = _lib.PpgPairMergeResult()
        self.m = M.struct_of(M.DEFAULT)
        device.after_torch()

    def ptr(self, k, shift=0):
        return C.c_void_p(self.buf[k].data_ptr() + shift)

    def inputs(self, **kw):
        a = dict(ctx=self.device.handle, m=C.byref(self.m), s1=C.byref(self.views[0]), s2=C.byref(self.views[1]),
                 rec1=None if self.rec1 is None else C.c_void_p(self.rec1.data_ptr()), rec2=None, npairs=self.n,
                 rows=C.c_void_p(self.rows.data_ptr()), row_cap=self.n)
        a.update(kw)
        return a

    def __call__(self, **kw):
        a = self.inputs()
        a.update(seq_off=self.ptr("seq_off"), seq_len=self.ptr("seq_len"), rec_cap=self.rec_cap, bases=self.ptr("bases"),
                 mask=self.ptr("mask"), qual=self.ptr("qual"), base_cap=self.base_cap, pair_of=self.ptr("pair_of"),
                 res=C.byref(self.res))
        a.update(kw)
        return _lib.lib.ppg_pairs_merge(*a.values())

    def size(self, **kw):
        a = self.inputs(**kw)
        del a["m"]
        n, b = C.c_int64(-1), C.c_int64(-1)
        return _lib.lib.ppg_pairs_merge_size(*a.values(), C.byref(n), C.byref(b)), n.value, b.value

    def untouched(self):
        return all(bool((b == 0xA5).all()) for b in self.buf.values())

    def got(self, k, dtype, n):
        """The first n values of a buffer, and whether every byte after them is still 0xA5."""
        a = self.buf[k].cpu().numpy()
        nb = n * np.dtype(dtype).itemsize
        return a[:nb].view(dtype), bool((a[nb:] == 0xA5).all())

    def assert_output(self, ref):
        """Everything up to seq_off[merged] is the reference's; everything after it, and every canary, is untouched."""
        n, nb = ref["merged"], ref["padded_bases"]
        for k, dtype, cnt, want in (("seq_off", np.int64, n + 1, ref["seq_off"]), ("seq_len", np.uint32, n, ref["seq_len"]),
                                    ("bases", np.uint32, nb // 16, ref["bases"]), ("mask", np.uint32, nb // 32, ref["mask"]),
                                    ("qual", np.uint8, nb, ref["qual"]), ("pair_of", np.int64, n, ref["pair_of"])):
            got, rest = self.got(k, dtype, cnt)
            assert np.array_equal(got, want), k
            assert rest, k
        assert [getattr(self.res, k) for k in M.TOTALS] == [ref[k] for k in M.TOTALS] and tuple(self.res.corrected) == ref["corrected"]


def hostile_rows():
    """(rows, rec1, expected class per touched pair): the reference overlap's rows of the forge with rows that do not
    fit their pairs, and valid-looking rows on pairs that are unmapped or too long."""
    pairs = V.forge()
    rows = V.forge_reference("defaults", "identity", windows=False)["rows"].copy()
    rec1 = np.arange(len(pairs), dtype=np.int64)
    found = [i for i in np.nonzero(rows[:, 3])[0] if i % 3 == 0]
    want = {}
    it = iter(found)
    L = lambda i: (len(pairs[i].r1), len(pairs[i].r2))   # noqa: E731
    for kind in range(16):
        for _ in range(3):
            i = int(next(it))
            L1, L2 = L(i)
            d, ov, mis, I = (int(x) for x in rows[i])
            cls = "stale"
            if kind == 0:
                row = (d, ov, mis, I + 1)                      # I != L2 + d
            elif kind == 1:
                row = (d + 1, ov, mis, I)
            elif kind == 2:
                row = (L1, ov, mis, L2 + L1)                   # d = L1
            elif kind == 3:
                row = (-L2, ov, mis, 1)                        # d = -L2 (its I would be 0: unmerged)
            elif kind == 4:
                row = (d, ov, mis, -I)                         # I < 0
            elif kind == 5:
                row = (-L2 - 5, ov, mis, -5)                   # I == L2 + d, both out of range
            elif kind == 6:
                row = (I32.min,) * 4
            elif kind == 7:
                row = (I32.max,) * 4
            elif kind < 16:
                f, v = (kind - 8) // 2, (I32.min, I32.max)[kind & 1]
                row = tuple(v if k == f else x for k, x in enumerate((d, ov, mis, I)))
                cls = "merged" if f in (1, 2) else "stale"     # ov and mis are not read
            rows[i] = row
            want[i] = cls
    # valid-looking rows where the pair is not analysed
    for i, p in enumerate(pairs):
        if max(L(i)) > V.MAX_LEN:
            rows[i] = (0, 100, 0, len(p.r2))
            want[i] = "too_long"
    for i in found[-40::4]:
        rec1[i] = (-1, len(pairs), 1 << 40, -(1 << 40))[i % 4]
        want[int(i)] = "unmapped"
    return rows, rec1, want


def test_hostile_rows(device):
    rows, rec1, want = hostile_rows()
    set1, qual1, set2, qual2, _, _ = M.forge_sets("identity")
    ref = M.merge_reference(set1, qual1, set2, qual2, rows, rec1=rec1)
    merged = set(ref["pair_of"].tolist())
    for i, cls in want.items():
        assert (i in merged) == (cls == "merged"), (i, cls)
        if cls in ("stale", "merged"):
            assert M.classify(len(set1[i]), len(set2[i]), rows[i]) == cls, (i, rows[i])
    assert ref["stale"] == sum(c == "stale" for c in want.values()) >= 36 and ref["unmapped"] == 10 and ref["too_long"] >= 4
    # caps with room to spare: what is past seq_off[merged] stays as it was
    c = Call(device, rows, ref["merged"] + 7, ref["padded_bases"] + 96, rec1)
    assert c() == 0
    c.assert_output(ref)
    assert c.size() == (0, ref["merged"], ref["padded_bases"])


def test_capacities_and_arguments(device):
    ref = M.forge_reference("defaults")
    rows = V.forge_reference("defaults", "identity", windows=False)["rows"]
    n, nm, nb = ref["pairs"], ref["merged"], ref["padded_bases"]
    c = Call(device, rows, nm, nb)
    v = c.views[0]
    view = lambda w=0, **kw: C.byref(_lib.PpgPackedView(**{**{f: getattr(c.views[w], f) for f, _ in v._fields_}, **kw}))   # noqa: E731
    bad_m = M.struct_of(M.Merge(47, 47))
    for kw, rc in ((dict(row_cap=n - 1), B), (dict(rec_cap=nm - 1), B), (dict(base_cap=nb - 32), B), (dict(rec_cap=0), B),
                   (dict(base_cap=0), B),
                   (dict(ctx=None), A), (dict(m=None), A), (dict(m=C.byref(bad_m)), A), (dict(s1=None), A), (dict(s2=None), A),
                   (dict(s1=view(bases=None)), A), (dict(s2=view(1, qual=None)), A), (dict(s1=view(qual=None)), A),
                   (dict(s1=view(seq_off=v.seq_off + 4)), A), (dict(s2=view(1, qual=c.views[1].qual + 8)), A), (dict(s1=view(records=-1)), A),
                   (dict(npairs=-1), A), (dict(npairs=n + 1, row_cap=n + 1), A),          # the identity map's limit
                   (dict(row_cap=-1), A), (dict(rec_cap=-1), A), (dict(base_cap=-32), A), (dict(base_cap=nb + 1), A),
                   (dict(rows=None), A), (dict(rows=C.c_void_p(c.rows.data_ptr() + 8)), A),
                   (dict(rec1=c.ptr("pair_of", 4)), A), (dict(rec2=c.ptr("pair_of", 4)), A),
                   (dict(seq_off=None), A), (dict(seq_off=c.ptr("seq_off", 4)), A), (dict(seq_len=None), A),
                   (dict(seq_len=c.ptr("seq_len", 2)), A), (dict(bases=None), A), (dict(bases=c.ptr("bases", 4)), A),
                   (dict(mask=None), A), (dict(mask=c.ptr("mask", 2)), A), (dict(qual=c.ptr("qual", 8)), A),
                   (dict(pair_of=c.ptr("pair_of", 4)), A)):
        assert c(**kw) == rc, kw
    assert c.untouched()                                                   # ... and nothing was written
    # the size entry: the merge's caps; it reads no quality plane
    assert c.size() == (0, nm, nb) and c.size(s1=view(qual=None), s2=view(1, qual=None)) == (0, nm, nb)
    assert c.size(row_cap=n - 1)[0] == B and c.size(ctx=None)[0] == A and c.size(npairs=-1)[0] == A
    assert c.size(rows=C.c_void_p(c.rows.data_ptr() + 8))[0] == A and c.size(s1=view(mask=None))[0] == A
    # exact caps: everything is written up to its cap and nothing past it
    assert c() == 0
    c.assert_output(ref)
    # optional outputs absent: the other planes are the same
    for k in ("qual", "pair_of"):
        c.buf[k].fill_(0xA5)
    assert c(qual=None, pair_of=None, res=None) == 0 and bool((c.buf["qual"] == 0xA5).all()) and bool((c.buf["pair_of"] == 0xA5).all())
    assert np.array_equal(c.got("bases", np.uint32, nb // 16)[0], ref["bases"]) and np.array_equal(c.got("mask", np.uint32, nb // 32)[0], ref["mask"])
    # fewer pairs than records
    k = 32 * 9 + 5
    set1, qual1, set2, qual2, _, _ = M.forge_sets("identity")
    part = M.merge_reference(set1, qual1, set2, qual2, rows, npairs=k)
    for b in c.buf.values():
        b.fill_(0xA5)
    assert c(npairs=k, row_cap=k) == 0 and 0 < part["merged"] < nm
    c.assert_output(part)
    # no pairs at all, and rows that are all zero: seq_off[0] = 0 and nothing else
    zero = rows_on_device(np.zeros_like(rows), device)
    nothing = dict(rec_cap=0, base_cap=0, seq_len=None, bases=None, mask=None, qual=None, pair_of=None)   # NULL at capacity 0
    for kw in (dict(npairs=0), dict(npairs=0, rows=None, row_cap=0, rec_cap=0, base_cap=0), dict(rows=C.c_void_p(zero.data_ptr())),
               dict(rows=C.c_void_p(zero.data_ptr()), **nothing), dict(npairs=0, rows=None, row_cap=0, **nothing)):
        for b in c.buf.values():
            b.fill_(0xA5)
        c.device.after_torch()
        assert c(**kw) == 0, kw
        got, rest = c.got("seq_off", np.int64, 1)
        assert got[0] == 0 and rest and all(bool((c.buf[x] == 0xA5).all()) for x in c.buf if x != "seq_off")
        assert c.res.merged == 0 and c.res.padded_bases == 0 and c.res.pairs == kw.get("npairs", n) == c.res.unmerged + c.res.too_long


    # ... but a NULL plane with room for something stays an error
    assert c(seq_len=None, rec_cap=1) == A and c(bases=None, base_cap=32) == A and c(mask=None, base_cap=32) == A
    assert c(**dict(nothing, seq_off=None)) == A


# ---- 5. the Python layer ----
@pytest.mark.parametrize("how", ["zero rows", "no pairs", "out of nothing"])
def test_nothing_merged(how, device):
    """No pair merges: an empty result, not an error, although a tensor of no elements has no address."""
    import torch
    p1, p2, _, _ = forge_on_device("identity", device)
    n = p1.records
    if how == "no pairs":
        none = torch.zeros(0, dtype=torch.int64, device=tdev(device))
        r = pp.pair_merge(p1, p2, torch.zeros((0, 4), dtype=torch.int32, device=tdev(device)), rec1=none, rec2=none, device=device)
        n = 0
    else:
        rows = torch.zeros((n, 4), dtype=torch.int32, device=tdev(device))
        out = pp.PackedReads.empty(0, 0, True, tdev(device)) if how == "out of nothing" else None
        r = pp.pair_merge(p1, p2, rows, out=out, device=device)
        assert out is None or r.reads is out
    assert r.merged == 0 and r.pairs == n == r.unmerged + r.too_long and r.merged_bases == r.padded_bases == r.overlap_bases == 0
    assert r.reads.records == 0 and r.reads.total_bases == 0 and r.pair_of.numel() == 0 and r.corrected == (0, 0)
    host = r.reads.to_host()
    assert host.seq_off.tolist() == [0] and host.seq_len.size == host.bases.size == host.mask.size == host.qual.size == 0


def test_python_layer_refuses_bad_tensors(device):
    import torch
    p1, p2, _, _ = forge_on_device("identity", device)
    dev = tdev(device)
    ref = M.forge_reference("defaults")
    rows = rows_on_device(V.forge_reference("defaults", "identity", windows=False)["rows"], device)
    noq = pp.PackedReads(p1.seq_off, p1.seq_len, p1.bases, p1.mask, None, p1.records, p1.total_bases)
    for kw in (dict(rows=rows.to(torch.int64)), dict(rows=rows.cpu()), dict(rows=rows.reshape(-1)[:-1]),
               dict(rec1=torch.zeros(4, dtype=torch.int32, device=dev)),
               dict(rec1=torch.zeros(4, dtype=torch.int64, device=dev), rec2=torch.zeros(5, dtype=torch.int64, device=dev)),
               dict(packed1=noq), dict(packed2=noq), dict(packed1=p1.to_host()), dict(merge=pp.PairMerge(47, 47)),
               dict(merge=pp.PairMerge(256, 0)), dict(merge=pp.PairOverlap()), dict(out=p1.to_host()), dict(out=rows),
               dict(pair_of=torch.zeros(ref["merged"], dtype=torch.int32, device=dev)),
               dict(pair_of=torch.zeros(ref["merged"] - 1, dtype=torch.int64, device=dev))):
        a = dict(packed1=p1, packed2=p2, rows=rows, device=device)
        a.update(kw)
        with pytest.raises(ValueError):
            pp.pair_merge(**a)
    with pytest.raises(pp.PpgError) as e:       # rows one short: the library's own check
        pp.pair_merge(p1, p2, rows[:-1].contiguous(), device=device)
    assert e.value.code == B
    small = pp.PackedReads.empty(ref["merged"] - 1, ref["padded_bases"], True, dev)
    with pytest.raises(pp.PpgError) as e:
        pp.pair_merge(p1, p2, rows, out=small, device=device)
    assert e.value.code == B and not bool(small.seq_off.any()) and not bool(small.qual.any())
    # planes of the caller's, larger than needed, and a pair_of of the caller's
    out = pp.PackedReads.empty(ref["merged"] + 5, ref["padded_bases"] + 320, True, dev)
    po = torch.full((ref["merged"] + 9,), -3, dtype=torch.int64, device=dev)
    r = pp.pair_merge(p1, p2, rows, out=out, pair_of=po, device=device)
    assert r.reads is out and out.records == ref["merged"] and out.total_bases == ref["padded_bases"]
    assert_equals_reference(r, ref, strings=False)
    assert bool((po[ref["merged"]:] == -3).all())


# ---- 6. PairedFASTQ.Merge over a forged R1 / R2 pair of files ----
@pytest.fixture(scope="module")
def pair_files(tmp_path_factory):
    idx = [i for i, p in enumerate(V.forge()) if i % 6 == 0 and len(p.r1) and len(p.r2)]
    pairs = [V.forge()[i] for i in idx]
    q1s, q2s = M.forge_quals()
    d = tmp_path_factory.mktemp("pairmerge")
    files = []
    for mate, flush, cs, qs in ((1, 37, 20, q1s), (2, 53, 30, q2s)):
        quals = [M.file_quals(qs[i]) for i in idx]
        gz = M.mate_file(pairs, quals, mate, flush)
        path = d / f"m{mate}.fastq.gz"
        path.write_bytes(gz)
        chunks, dup = M.oracle_chunks(gz, cs)
        recs = T.fields(chunks)
        reads, rq = [S for _, S, _ in recs], [Q for _, _, Q in recs]
        assert [reads[j] for j in np.nonzero(~dup)[0]] == [p.r1 if mate == 1 else p.r2 for p in pairs]
        assert [rq[j] for j in np.nonzero(~dup)[0]] == quals
        files.append((str(path), gz, cs, dup, reads, rq))
    assert files[0][3].sum() > 5
    return pairs, files


@pytest.mark.parametrize("cap", [0, 32 << 10])
def test_paired_fastq_merge(pair_files, cap, device):
    pairs, files = pair_files
    ix = [pp.Core.BuildDeflateIndex(f[1], f[2]) for f in files]
    pf = paired.PairedFASTQ(ix[0], files[0][0], ix[1], files[1][0], pair_chunk=100, device=device, out_capacity=cap)
    assert pf.Count() == len(pairs) and [sh.batches > 1 for sh in pf.shards] == [cap > 0] * 2
    # the reference on the shards' records: the twice-parsed ones are in no pair
    maps = [np.nonzero(~f[3])[0].astype(np.int64) for f in files]
    sets, quals = [f[4] for f in files], [f[5] for f in files]
    for prm, mrg in ((None, None), (pp.PairOverlap(*V.EXACT), pp.PairMerge(70, 40))):
        p = V.DEFAULTS if prm is None else V.Params(prm.min_overlap, prm.max_diff, prm.max_err_milli)
        ov = V.overlap_reference(sets[0], sets[1], p, maps[0], maps[1])
        ref = M.merge_reference(sets[0], quals[0], sets[1], quals[1], ov["rows"], M.DEFAULT if mrg is None else M.Merge(70, 40),
                                maps[0], maps[1])
        r = pf.Merge(prm, mrg)
        assert_equals_reference(r, ref)
        assert r.merged > 50 and r.unmapped == 0 and r.stale == 0
        assert r.overlap.found == r.merged and np.array_equal(r.overlap.rows.cpu().numpy(), ov["rows"])
        assert r.overlap.overlap_bases == r.overlap_bases and r.overlap.mismatches == r.disagree + r.n_filled + r.n_both
    # the pair chunks and the overlap are still there after the re-runs
    assert sum(len(a) for _, a, _ in pf.pair_chunks()) == len(pairs)
    o = pf.Overlap()
    ov = V.overlap_reference(sets[0], sets[1], V.DEFAULTS, maps[0], maps[1])
    assert [getattr(o, k) for k in V.TOTALS] == [ov[k] for k in V.TOTALS] and np.array_equal(o.rows.cpu().numpy(), ov["rows"])
    assert np.array_equal(M.words(o.found_mask), ov["mask"]) and o.windows1 is None


# ---- 7. the merged set is a packed set ----
def test_merged_set_feeds_the_overlap(device):
    import torch
    p1, p2, _, _ = forge_on_device("identity", device)
    ref = M.forge_reference("defaults")
    r = pp.pair_merge(p1, p2, rows_on_device(V.forge_reference("defaults", "identity", windows=False)["rows"], device), device=device)
    # merged read j against merged read j + 1, every 5th, any number of mismatches allowed: the first candidate of
    # 30 bases is accepted, and its mismatch count depends on every base and N bit of both reads
    a = np.arange(0, ref["merged"] - 1, 5, dtype=np.int64)
    prm = V.ALWAYS
    want = V.overlap_reference(ref["seqs"], ref["seqs"], prm, a, a + 1, windows1=V.whole_rows(ref["seqs"]))
    rec = [torch.from_numpy(x).to(tdev(device)) for x in (a, a + 1)]
    got = pp.pair_overlap(r.reads, r.reads, pp.PairOverlap(*prm), rec[0], rec[1], windows1=True, device=device)
    assert [getattr(got, k) for k in V.TOTALS] == [want[k] for k in V.TOTALS] and 100 < want["found"] < want["pairs"] and want["mismatches"] > 10000
    assert np.array_equal(got.rows.cpu().numpy(), want["rows"]) and np.array_equal(got.insert_hist, want["hist"])
    assert np.array_equal(M.words(got.windows1).reshape(-1, 2), want["windows1"])


# ---- 8. the probe hook ----
def test_probe_hook(device):
    p1, p2, _, _ = forge_on_device("identity", device)
    ref = M.forge_reference("defaults")
    rows = rows_on_device(V.forge_reference("defaults", "identity", windows=False)["rows"], device)
    fn = _lib.lib.ppgx_pairmerge_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float),
                   C.POINTER(C.c_int64)]
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                p.qual.data_ptr(), p.records) for p in (p1, p2)]
    m, ms, sizes = M.struct_of(M.DEFAULT), (C.c_float * 4)(-1.0, -1.0, -1.0, -1.0), (C.c_int64 * 2)(-1, -1)
    rp = C.c_void_p(rows.data_ptr())
    device.after_torch()
    a = (device.handle, C.byref(m), C.byref(views[0]), C.byref(views[1]), p1.records, rp)
    assert fn(*a, 2, ms, sizes) == _lib.PPG_OK
    assert all(np.isfinite(x) and x >= 0 for x in ms) and list(sizes) == [ref["merged"], ref["padded_bases"]]
    assert fn(*a, 0, ms, sizes) == A and fn(*a, 1, None, sizes) == A and fn(*a, 1, ms, None) == A
    assert fn(*a[:4], p1.records + 1, rp, 1, ms, sizes) == A and fn(None, *a[1:], 1, ms, sizes) == A
    assert fn(a[0], None, *a[2:], 1, ms, sizes) == A
    # the call afterwards is unharmed
    assert_equals_reference(pp.pair_merge(p1, p2, rows, device=device), ref, strings=False)
