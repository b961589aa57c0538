"""The pair overlap on the GPU (ppg_pairoverlap.hip through the C ABI and the Python layer) against the reference
of the semantics (tests/pairoverlap_ref.py): rows, found mask, both windows planes, totals and the insert-size
histogram, all exact (integer work: no tolerance).  Inputs: the forge of read pairs under every parameter set and
map (tests/test_pairoverlap_cpu.py guards that it is what it claims), and a forged R1 / R2 pair of .gz files
through PairedFASTQ."""
import ctypes as C
import zlib

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib, paired
from oracle import oracle as O
import pairoverlap_ref as V
import readprofile_ref as P
import readtrim_ref as T

pytestmark = pytest.mark.gpu

A, B = _lib.PPG_ARG_ERROR, _lib.PPG_BUF_ERROR
GUARD = 4096          # canary bytes past every buffer


def to_device(reads, device):
    """A list of reads as a PackedReads of CUDA tensors, packed by the reference of the format."""
    import torch
    h = V.pack_strings(reads)
    dev = torch.device("cuda", device.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).to(dev)  # noqa: E731
    return pp.PackedReads(t(h["seq_off"]), t(h["seq_len"]), t(h["bases"]), t(h["mask"]), None, len(reads), int(h["seq_off"][-1]))


_sets = {}


def forge_on_device(which, device):
    """(packed1, packed2, rec1, rec2 as CUDA tensors or None) of the forge under a map; made once."""
    import torch
    if which not in _sets:
        set1, set2, rec1, rec2 = V.forge_sets(which)
        dev = torch.device("cuda", device.device)
        m = lambda r: None if r is None else torch.from_numpy(r.copy()).to(dev)   # noqa: E731
        _sets[which] = (to_device(set1, device), to_device(set2, device), m(rec1), m(rec2))
    return _sets[which]


def words(t):
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def assert_equals_reference(r, ref, windows=True):
    assert [getattr(r, k) for k in V.TOTALS] == [ref[k] for k in V.TOTALS] and r.clipped == ref["clipped"]
    assert np.array_equal(r.insert_hist, ref["hist"]), np.nonzero(r.insert_hist != ref["hist"])[0][:8]
    if r.rows is not None:
        got = r.rows.cpu().numpy()
        bad = np.nonzero((got != ref["rows"]).any(axis=1))[0]
        assert bad.size == 0, (bad[:8].tolist(), got[bad[0]].tolist(), ref["rows"][bad[0]].tolist())
    if r.found_mask is not None:
        assert np.array_equal(words(r.found_mask), ref["mask"])
    if windows:
        for got, want in ((r.windows1, ref["windows1"]), (r.windows2, ref["windows2"])):
            got = words(got).reshape(-1, 2)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (bad[:8].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


def set_grid(device, blocks):
    fn = _lib.lib.ppgx_pairoverlap_grid
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(device.handle, blocks) == _lib.PPG_OK


# ---- 1. parity on the forge ----
@pytest.mark.parametrize("which", ["identity", "permutation", "holes"])
@pytest.mark.parametrize("pname", sorted(V.PARAM_SETS))
def test_forge_matches_reference(pname, which, device):
    p1, p2, rec1, rec2 = forge_on_device(which, device)
    p = V.PARAM_SETS[pname]
    r = pp.pair_overlap(p1, p2, pp.PairOverlap(*p), rec1, rec2, windows1=True, windows2=True, device=device)
    ref = V.forge_reference(pname, which)
    assert_equals_reference(r, ref)
    med = np.repeat(np.arange(V.HIST), ref["hist"])
    assert r.median_insert == (int(med[(med.size - 1) // 2]) if med.size else None)
    assert r.found > 0 and r.rows.shape == (ref["pairs"], 4) and r.found_mask.numel() == (ref["pairs"] + 31) // 32


def test_grids_agree(device):
    """The default grid, one block (which loops over every pair) and three blocks (uneven shares)."""
    p1, p2, rec1, rec2 = forge_on_device("holes", device)
    ref = V.forge_reference("defaults", "holes")
    try:
        for blocks in (0, 1, 3):
            set_grid(device, blocks)
            assert_equals_reference(pp.pair_overlap(p1, p2, pp.PairOverlap(), rec1, rec2, windows1=True, windows2=True,
                                                    device=device), ref)
    finally:
        set_grid(device, 0)
    fn = _lib.lib.ppgx_pairoverlap_grid
    assert fn(device.handle, -1) == A and fn(None, 1) == A


# ---- 2. prior windows rows: a trim's rows are clipped, every other row stays bit-identical ----
def test_prior_rows_and_untouched_rows(device):
    import torch
    p1, p2, rec1, rec2 = forge_on_device("holes", device)
    set1, set2, h1, h2 = V.forge_sets("holes")
    rng = np.random.default_rng(5)
    prior = []
    for s in (set1, set2):
        L = np.array([len(x) for x in s], np.int64)
        rows = np.stack([rng.integers(0, L + 3), rng.integers(0, L + 3)], axis=1).astype(np.uint32)
        rows[::17] = (0xFFFFFFFF, 0xFFFFFFFF)          # hostile rows: past the read, and lengths that wrap when added
        rows[5::19, 1] = 0xFFFFFFFF
        rows[7::23] = (0, 0)
        prior.append(rows)
    ref = V.overlap_reference(set1, set2, V.DEFAULTS, h1, h2, windows1=prior[0], windows2=prior[1])
    dev = torch.device("cuda", device.device)
    w = [torch.from_numpy(x.view(np.int32).copy()).to(dev) for x in prior]
    r = pp.pair_overlap(p1, p2, pp.PairOverlap(), rec1, rec2, windows1=w[0], windows2=w[1], device=device)
    assert r.windows1 is w[0] and r.windows2 is w[1]
    assert_equals_reference(r, ref)
    # the records of found pairs, by set; every other row is the prior row
    n = len(set1)
    for m, (recs, rows) in enumerate(((h1, prior[0]), (h2, prior[1]))):
        ok = (h1 >= 0) & (h1 < n) & (h2 >= 0) & (h2 < n) & ref["found_bits"]
        touched = np.zeros(n, bool)
        touched[recs[ok]] = True
        got = words(w[m]).reshape(-1, 2)
        assert 100 < touched.sum() < n - 100 and np.array_equal(got[~touched], rows[~touched])
        assert (got[touched] != rows[touched]).any()


# ---- 3. the C entry point: optional outputs, capacities, arguments ----
class Call:
    """The buffers of one ppg_pairs_overlap call on the forge (identity map), each with GUARD bytes of 0xA5 behind
    it, and the call with any argument replaced."""

    def __init__(self, device):
        import torch
        self.device = device
        self.p1, self.p2, _, _ = forge_on_device("identity", device)
        self.n = n = self.p1.records
        dev = torch.device("cuda", device.device)
        self.words = (n + 31) // 32
        self.sizes = {"rows": 16 * n, "mask": 4 * self.words, "win1": 8 * n, "win2": 8 * n}
        self.buf = {k: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for k, v in self.sizes.items()}
        self.views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                         None, p.records) for p in (self.p1, self.p2)]
        self.res, self.hist = _lib.PpgPairOverlapResult(), np.full(V.HIST + 8, -7, np.int64)
        self.o = V.struct_of(V.DEFAULTS)
        device.after_torch()

    def ptr(self, k, shift=0):
        return C.c_void_p(self.buf[k].data_ptr() + shift)

    def __call__(self, **kw):
        n = self.n
        a = dict(ctx=self.device.handle, o=C.byref(self.o), s1=C.byref(self.views[0]), s2=C.byref(self.views[1]), rec1=None,
                 rec2=None, npairs=n, rows=self.ptr("rows"), row_cap=n, mask=self.ptr("mask"), mask_cap=32 * self.words,
                 win1=self.ptr("win1"), cap1=n, win2=self.ptr("win2"), cap2=n, res=C.byref(self.res),
                 hist=self.hist.ctypes.data_as(C.c_void_p), hist_cap=V.HIST)
        a.update(kw)
        return _lib.lib.ppg_pairs_overlap(*a.values())

    def untouched(self):
        return all(bool((b == 0xA5).all()) for b in self.buf.values()) and bool((self.hist == -7).all())

    def guards_intact(self):
        return all(bool((self.buf[k][v:] == 0xA5).all()) for k, v in self.sizes.items()) and bool((self.hist[V.HIST:] == -7).all())

    def fill_windows(self):
        """Whole-read rows in both planes (the guards stay)."""
        import torch
        for k, p in (("win1", self.p1), ("win2", self.p2)):
            rows = torch.stack([torch.zeros_like(p.seq_len), p.seq_len], dim=1).contiguous().view(torch.uint8).reshape(-1)
            self.buf[k][:rows.numel()] = rows

    def got(self, k, dtype):
        return self.buf[k][:self.sizes[k]].cpu().numpy().view(dtype)


def test_capacities_and_arguments(device):
    c = Call(device)
    n, W = c.n, c.words
    bad_view = _lib.PpgPackedView(c.views[0].seq_off, c.views[0].seq_len, None, c.views[0].mask, None, n)
    odd_view = _lib.PpgPackedView(c.views[0].seq_off + 4, c.views[0].seq_len, c.views[0].bases, c.views[0].mask, None, n)
    neg_view = _lib.PpgPackedView(c.views[0].seq_off, c.views[0].seq_len, c.views[0].bases, c.views[0].mask, None, -1)
    bad_o = V.struct_of(V.Params(0, 5, 200))
    for kw, rc in ((dict(row_cap=n - 1), B), (dict(mask_cap=32 * W - 32), B), (dict(cap1=n - 1), B), (dict(cap2=n - 1), B),
                   (dict(hist_cap=V.HIST - 1), B), (dict(hist_cap=0), B),
                   (dict(ctx=None), A), (dict(o=None), A), (dict(o=C.byref(bad_o)), A), (dict(s1=None), A), (dict(s2=None), A),
                   (dict(s1=C.byref(bad_view)), A), (dict(s2=C.byref(odd_view)), A), (dict(s1=C.byref(neg_view)), A),
                   (dict(npairs=-1), A), (dict(npairs=n + 1, row_cap=n + 1, mask_cap=32 * W + 32), A),   # the identity map's limit
                   (dict(mask_cap=32 * W + 1), A), (dict(row_cap=-1), A), (dict(cap1=-1), A), (dict(hist_cap=-1), A),
                   (dict(rows=c.ptr("rows", 8)), A), (dict(mask=c.ptr("mask", 2)), A), (dict(win1=c.ptr("win1", 4)), A),
                   (dict(win2=c.ptr("win2", 4)), A), (dict(rec1=c.ptr("rows", 4)), A), (dict(rec2=c.ptr("rows", 4)), A)):
        assert c(**kw) == rc, kw
    assert c.untouched()                                                   # ... and nothing was written
    # exact caps: everything is written up to its cap and nothing past it
    c.fill_windows()
    assert c() == 0 and c.guards_intact()
    ref = V.forge_reference("defaults", "identity")
    assert [getattr(c.res, k) for k in V.TOTALS] == [ref[k] for k in V.TOTALS] and tuple(c.res.clipped) == ref["clipped"]
    assert np.array_equal(c.hist[:V.HIST], ref["hist"])
    assert np.array_equal(c.got("rows", np.int32).reshape(-1, 4), ref["rows"]) and np.array_equal(c.got("mask", np.uint32), ref["mask"])
    assert np.array_equal(c.got("win1", np.uint32).reshape(-1, 2), ref["windows1"])
    assert np.array_equal(c.got("win2", np.uint32).reshape(-1, 2), ref["windows2"])
    # fewer pairs than records: the mask's words below ceil(npairs / 32) whole, none after; rows past npairs stay
    c.buf["rows"].fill_(0xA5)
    c.buf["mask"].fill_(0xA5)
    k = 32 * 5 + 3
    assert c(npairs=k, row_cap=k, mask_cap=32 * 6, win1=None, cap1=0, win2=None, cap2=0, hist=None, hist_cap=0) == 0
    assert np.array_equal(c.got("rows", np.int32).reshape(-1, 4)[:k], ref["rows"][:k]) and bool((c.buf["rows"][16 * k:] == 0xA5).all())
    assert np.array_equal(c.got("mask", np.uint32)[:6], V.mask_words(ref["found_bits"][:k])) and bool((c.buf["mask"][24:] == 0xA5).all())
    assert c.res.pairs == k and c.res.found == int(ref["found_bits"][:k].sum())
    # no pairs at all
    assert c(npairs=0) == 0 and c.res.pairs == 0 and c.res.found == 0 and not c.hist[:V.HIST].any()


@pytest.mark.parametrize("absent", ["rows", "mask", "win1", "win2", "res", "hist", "all"])
def test_optional_outputs_absent(absent, device):
    c = Call(device)
    c.fill_windows()
    ref = V.forge_reference("defaults", "identity")
    off = {"rows": dict(rows=None, row_cap=0), "mask": dict(mask=None, mask_cap=0), "win1": dict(win1=None, cap1=0),
           "win2": dict(win2=None, cap2=0), "res": dict(res=None), "hist": dict(hist=None, hist_cap=0)}
    kw = {}
    for k, v in off.items():
        if absent in (k, "all"):
            kw.update(v)
    before = {k: c.buf[k].clone() for k in c.buf}
    assert c(**kw) == 0 and c.guards_intact()
    gone = lambda k: absent in (k, "all")   # noqa: E731
    for k in ("rows", "mask", "win1", "win2"):
        if gone(k):
            assert bool((c.buf[k] == before[k]).all()), k
    if not gone("rows"):
        assert np.array_equal(c.got("rows", np.int32).reshape(-1, 4), ref["rows"])
    if not gone("mask"):
        assert np.array_equal(c.got("mask", np.uint32), ref["mask"])
    if not gone("win1"):
        assert np.array_equal(c.got("win1", np.uint32).reshape(-1, 2), ref["windows1"])
    if not gone("win2"):
        assert np.array_equal(c.got("win2", np.uint32).reshape(-1, 2), ref["windows2"])
    if not gone("res"):
        assert [getattr(c.res, k) for k in V.TOTALS] == [ref[k] for k in V.TOTALS]
    assert np.array_equal(c.hist[:V.HIST], ref["hist"]) if not gone("hist") else bool((c.hist == -7).all())


def test_python_layer_refuses_bad_tensors(device):
    import torch
    p1, p2, _, _ = forge_on_device("identity", device)
    dev = torch.device("cuda", device.device)
    with pytest.raises(ValueError):
        pp.pair_overlap(p1, p2, pp.PairOverlap(), rec1=torch.zeros(4, dtype=torch.int32, device=dev), device=device)
    with pytest.raises(ValueError):
        pp.pair_overlap(p1, p2, pp.PairOverlap(), rec1=torch.zeros(4, dtype=torch.int64, device=dev),
                        rec2=torch.zeros(5, dtype=torch.int64, device=dev), device=device)
    with pytest.raises(ValueError):
        pp.pair_overlap(p1, p2, pp.PairOverlap(), rows=torch.zeros((p1.records, 4), dtype=torch.int64, device=dev), device=device)
    with pytest.raises(ValueError):
        pp.pair_overlap(p1, p2, pp.PairOverlap(), windows1=torch.zeros((p1.records, 2), dtype=torch.int32), device=device)
    with pytest.raises(ValueError):
        pp.pair_overlap(p1, p2, pp.PairOverlap(0), device=device)
    with pytest.raises(pp.PpgError) as e:       # rows one short: the library's own check
        pp.pair_overlap(p1, p2, pp.PairOverlap(), rows=torch.zeros((p1.records - 1, 4), dtype=torch.int32, device=dev), device=device)
    assert e.value.code == B
    r = pp.pair_overlap(p1, p2, pp.PairOverlap(), rows=False, found_mask=False, device=device)
    assert r.rows is None and r.found_mask is None and r.windows1 is None and r.found == V.forge_reference("defaults", "identity")["found"]


# ---- 4. PairedFASTQ.Overlap over a forged R1 / R2 pair of files ----
def mate_file(pairs, mate, flush_every):
    """The mate's FASTQ as one gzip member, a full flush after every flush_every records: Points fall on record
    starts, so the reference parses some records twice."""
    recs = []
    for i, p in enumerate(pairs):
        s = p.r1 if mate == 1 else p.r2
        recs.append(b"@SRR9.%d.%d\n%s\n+\n%s\n" % (i + 1, mate, s, b"I" * len(s)))
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = []
    for g in range(0, len(recs), flush_every):
        out.append(co.compress(b"".join(recs[g:g + flush_every])))
        out.append(co.flush(zlib.Z_FULL_FLUSH))
    out.append(co.flush())
    return b"".join(out)


def oracle_chunks(gz, cs):
    """Per chunk, from the oracle: (offset_k, raw_k, descriptors), and per shard record whether it is a Q1 duplicate."""
    oi = O.build_index(gz, cs)
    chunks, dup = [], []
    for k in range(oi.count - 1):
        off = oi.point(k)[4]
        desc = np.asarray(O.parse(off, O.extract(gz, oi, k)), np.uint32).reshape(-1, 4)
        chunks.append((off, off + O.extract(gz, oi, k), desc))
        dup += [j == 0 and int(d[3]) < len(off) for j, d in enumerate(desc)]
    return chunks, np.array(dup, bool)


@pytest.fixture(scope="module")
def pair_files(tmp_path_factory):
    pairs = [p for p in V.forge()[::6] if len(p.r1) and len(p.r2)]
    d = tmp_path_factory.mktemp("pairoverlap")
    files = []
    for mate, flush, cs in ((1, 37, 20), (2, 53, 30)):
        gz = mate_file(pairs, mate, flush)
        path = d / f"m{mate}.fastq.gz"
        path.write_bytes(gz)
        chunks, dup = oracle_chunks(gz, cs)
        reads = [S for _, S, _ in T.fields(chunks)]
        assert [reads[j] for j in np.nonzero(~dup)[0]] == [p.r1 if mate == 1 else p.r2 for p in pairs]
        files.append((str(path), gz, cs, chunks, dup, reads))
    assert files[0][4].sum() > 5 and len(files[0][3]) > 5 and len(files[1][3]) > 2
    return pairs, files


@pytest.mark.parametrize("cap", [0, 32 << 10])
def test_paired_fastq_overlap(pair_files, cap, device):
    pairs, files = pair_files
    ix = [pp.Core.BuildDeflateIndex(f[1], f[2]) for f in files]
    pf = paired.PairedFASTQ(ix[0], files[0][0], ix[1], files[1][0], pair_chunk=100, device=device, out_capacity=cap)
    assert pf.Count() == len(pairs) and [sh.batches > 1 for sh in pf.shards] == [cap > 0] * 2
    # the reference on the shards' records: the twice-parsed ones are in no pair
    maps = [np.nonzero(~f[4])[0].astype(np.int64) for f in files]
    sets = [f[5] for f in files]
    for prm, windows in ((None, True), (pp.PairOverlap(*V.EXACT), False), (pp.PairOverlap(*V.RATE), True)):
        p = V.DEFAULTS if prm is None else V.Params(prm.min_overlap, prm.max_diff, prm.max_err_milli)
        ref = V.overlap_reference(sets[0], sets[1], p, maps[0], maps[1],
                                  windows1=V.whole_rows(sets[0]) if windows else None,
                                  windows2=V.whole_rows(sets[1]) if windows else None)
        r = pf.Overlap(prm, windows=windows)
        assert_equals_reference(r, ref, windows)
        assert (r.windows1 is None) == (not windows) and r.found > 50 and r.unmapped == 0
    # the pair chunks are still there after the re-runs
    assert sum(len(a) for _, a, _ in pf.pair_chunks()) == len(pairs)
    if cap:
        return
    # the clipped rows go into each file's own profile as they are
    r = pf.Overlap(windows=True)
    pr = P.profile(1024)
    for f, sh, w in zip(files, pf.shards, (r.windows1, r.windows2)):
        rows = words(w).reshape(-1, 2)
        assert (rows[f[4]] == V.whole_rows([f[5][j] for j in np.nonzero(f[4])[0]])).all()     # duplicates: whole reads
        got, want = sh.profile_reads(pp.ReadProfile(1024), windows=w), P.profile_reference(f[3], pr, None, rows)
        assert [getattr(got, k) for k in P.TOTALS] == [want[k] for k in P.TOTALS]
        for name in P.ROW_DTYPE.names:
            assert np.array_equal(got.table[name], want["table"][name]), name
        assert got.bases < sum(len(s) for s in f[5])


# ---- 5. the probe hook ----
def test_probe_hook(device):
    p1, p2, _, _ = forge_on_device("identity", device)
    fn = _lib.lib.ppgx_pairoverlap_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(), None, p.records)
             for p in (p1, p2)]
    o, ms = V.struct_of(V.DEFAULTS), (C.c_float * 1)(-1.0)
    device.after_torch()
    assert fn(device.handle, C.byref(o), C.byref(views[0]), C.byref(views[1]), p1.records, 2, ms) == _lib.PPG_OK
    assert np.isfinite(ms[0]) and ms[0] >= 0
    assert fn(device.handle, C.byref(o), C.byref(views[0]), C.byref(views[1]), p1.records, 0, ms) == A
    assert fn(device.handle, C.byref(o), C.byref(views[0]), C.byref(views[1]), p1.records + 1, 1, ms) == A
    assert fn(None, C.byref(o), C.byref(views[0]), C.byref(views[1]), p1.records, 1, ms) == A
    # the call afterwards is unharmed
    assert_equals_reference(pp.pair_overlap(p1, p2, pp.PairOverlap(), device=device), V.forge_reference("defaults", "identity"), False)
