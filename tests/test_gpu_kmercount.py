"""The k-mer counts on the GPU (ppg_kmercount.hip through the C ABI and the Python layer) against the reference of
the semantics (tests/kmercount_ref.py): the table's rows, the totals and the spectrum, all exact (integer work: no
tolerance).  Inputs: the forge of reads under every tested k and both canonical settings
(tests/test_kmercount_cpu.py guards that it is what it claims), and forged .gz files through
BatchedFASTQ.CountKmers and PairedFASTQ.CountKmers."""
import ctypes as C
import zlib

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib, paired
from oracle import oracle as O
import kmercount_ref as K
import readdedup_ref as D
import readfilter_ref as F
import readtrim_ref as T
import seqquery_ref as Q

pytestmark = pytest.mark.gpu

A, B = _lib.PPG_ARG_ERROR, _lib.PPG_BUF_ERROR
GUARD = 4096          # canary bytes past every buffer
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def tdev(device):
    import torch
    return torch.device("cuda", device.device)


def to_device(reads, device):
    """A list of reads as a PackedReads of CUDA tensors, packed by the reference of the format."""
    import torch
    h = K.pack_strings(reads)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).to(tdev(device))  # noqa: E731
    return pp.PackedReads(t(h["seq_off"]), t(h["seq_len"]), t(h["bases"]), t(h["mask"]), None, len(reads), int(h["seq_off"][-1]))


_forge = {}


def forge_on_device(device):
    if "p" not in _forge:
        _forge["p"] = to_device(K.forge_reads(), device)
    return _forge["p"]


def words_tensor(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(tdev(device))


def host(t):
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def table_rows(table):
    """(keys, counts) of the non-empty rows of a device table sorted by key; every other row must be {~0, 0}."""
    t = table.cpu().numpy().view(np.uint64).reshape(-1, 2)
    used = t[:, 0] != EMPTY
    assert not t[~used, 1].any()
    rows = t[used]
    order = np.argsort(rows[:, 0])
    return rows[order, 0], rows[order, 1].astype(np.int64)


def assert_equals_reference(r, ref, call_totals=True):
    names = K.TOTALS if call_totals else K.TABLE_TOTALS
    assert [getattr(r, k) for k in names] == [ref[k] for k in names], [(k, getattr(r, k), ref[k]) for k in names if getattr(r, k) != ref[k]]
    assert r.overflow == 0
    assert np.array_equal(r.spectrum, ref["spectrum"]), np.nonzero(r.spectrum != ref["spectrum"])[0][:8]
    keys, counts = table_rows(r.table)
    assert np.array_equal(keys, ref["keys"]) and np.array_equal(counts, ref["counts"])


def slots_for(ref):
    return pp.KmerCount.min_slots(ref["distinct"])


def set_grid(device, blocks):
    fn = _lib.lib.ppgx_kmercount_grid
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(device.handle, blocks) == _lib.PPG_OK


# ---- 1. parity on the forge ----
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_forge_matches_reference(k, canonical, device):
    p = forge_on_device(device)
    ref = K.forge_reference(k, canonical)
    r = pp.count_kmers(p, pp.KmerCount(k, canonical), slots=slots_for(ref), device=device)
    assert_equals_reference(r, ref)
    assert r.retries == 0 and r.slots == slots_for(ref) and r.kmers == r.total_count and r.spectrum[K.SPECTRUM - 1] > 0


# ---- 2. mask and windows ----
def hostile_rows(reads, rng):
    L = np.array([len(x) for x in reads], np.int64)
    rows = np.stack([rng.integers(0, L + 3), rng.integers(0, L + 3)], axis=1).astype(np.uint32)
    rows[::17] = (0xFFFFFFFF, 0xFFFFFFFF)          # past the read, and lengths that wrap when added
    rows[5::19, 1] = 0xFFFFFFFF
    rows[7::23] = (0, 0)
    rows[3::29] = (0, 0xFFFFFFFF)                  # the whole read
    return rows


@pytest.mark.parametrize("k,canonical", [(21, True), (16, False), (1, True)])
def test_mask_and_windows(k, canonical, device):
    reads = K.forge_reads()
    p = forge_on_device(device)
    rng = np.random.default_rng(5)
    bits = rng.random(len(reads)) < 0.6
    rows = hostile_rows(reads, rng)
    mwords = np.concatenate([K.mask_words(bits), np.array([0xFFFFFFFF], np.uint32)])   # (a word more than the records need)
    dm, dw = words_tensor(mwords, device), words_tensor(rows, device)
    kc = pp.KmerCount(k, canonical)
    for m, w in ((dm, None), (None, dw), (dm, dw)):
        ref = K.reference(reads, k, canonical, bits if m is not None else None, rows if w is not None else None)
        r = pp.count_kmers(p, kc, mask=m, windows=w, slots=slots_for(K.forge_reference(k, canonical)), device=device)
        assert_equals_reference(r, ref)
        assert 0 < ref["kmers"] < K.forge_reference(k, canonical)["kmers"]
    assert np.array_equal(host(dm), mwords) and np.array_equal(host(dw).reshape(-1, 2), rows)        # only read
    h = K.pack_strings(reads)
    assert np.array_equal(host(p.bases), h["bases"]) and np.array_equal(host(p.mask), h["mask"])


# ---- 3. grids ----
def test_grids_agree(device):
    """The default grid, one block (which loops over every tile) and three blocks (uneven shares)."""
    p = forge_on_device(device)
    try:
        for blocks in (0, 1, 3):
            set_grid(device, blocks)
            for k, canonical in ((21, True), (31, False)):
                ref = K.forge_reference(k, canonical)
                assert_equals_reference(pp.count_kmers(p, pp.KmerCount(k, canonical), slots=slots_for(ref), device=device), ref)
    finally:
        set_grid(device, 0)
    fn = _lib.lib.ppgx_kmercount_grid
    assert fn(device.handle, -1) == A and fn(None, 1) == A


# ---- 4 / 7. the C entry point: capacity, optional outputs, arguments ----
class Call:
    """The buffers of one ppg_kmers_count call on the forge, each device buffer with GUARD bytes of 0xA5 behind it,
    and the call with any argument replaced."""

    def __init__(self, device, slots, k=21, flags=K.CANONICAL, reads=None):
        import torch
        self.device = device
        self.p = forge_on_device(device) if reads is None else to_device(reads, device)
        self.n = n = self.p.records
        self.slots = slots
        self.mwords = (n + 31) // 32
        self.sizes = {"table": 16 * slots, "mask": 4 * self.mwords, "win": 8 * n}
        self.buf = {k_: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device=tdev(device)) for k_, v in self.sizes.items()}
        self.view = _lib.PpgPackedView(self.p.seq_off.data_ptr(), self.p.seq_len.data_ptr(), self.p.bases.data_ptr(),
                                       self.p.mask.data_ptr(), None, n)
        self.res = _lib.PpgKmerCountResult()
        self.spec = np.full(K.SPECTRUM + 8, -7, np.int64)
        self.o = K.struct_of(k, flags)
        device.after_torch()

    def ptr(self, k, shift=0):
        return C.c_void_p(self.buf[k].data_ptr() + shift)

    def __call__(self, **kw):
        a = dict(ctx=self.device.handle, o=C.byref(self.o), s=C.byref(self.view), mask=None, mask_cap=0, win=None, win_cap=0,
                 table=self.ptr("table"), slots=self.slots, res=C.byref(self.res), spec=self.spec.ctypes.data_as(C.c_void_p),
                 spec_cap=K.SPECTRUM)
        a.update(kw)
        self.device.after_torch()
        return _lib.lib.ppg_kmers_count(*a.values())

    def untouched(self):
        return all(bool((b == 0xA5).all()) for b in self.buf.values()) and bool((self.spec == -7).all())

    def guards_intact(self):
        return all(bool((self.buf[k][v:] == 0xA5).all()) for k, v in self.sizes.items()) and bool((self.spec[K.SPECTRUM:] == -7).all())

    def rows(self):
        import torch
        return table_rows(self.buf["table"][:self.sizes["table"]].view(torch.int64))


def test_capacity_fails_fast_and_recovers(device):
    ref = K.forge_reference(21, True)
    S = slots_for(ref)
    assert ref["distinct"] > S // 4
    c = Call(device, S)                     # the buffer is sized for S; smaller tables use its front
    for slots, rc in ((S // 2, B), (64, B), (S, 0), (64, B), (S, 0)):
        c.buf["table"].fill_(0xA5)
        c.spec[:] = -7
        assert c(slots=slots) == rc, slots
        assert bool((c.buf["table"][16 * slots:] == 0xA5).all()) and c.guards_intact()
        if rc:
            assert bool((c.spec == -7).all())          # nothing outside the table is written
        else:
            keys, counts = c.rows()
            assert np.array_equal(keys, ref["keys"]) and np.array_equal(counts, ref["counts"])
            assert [getattr(c.res, k) for k in K.TOTALS] == [ref[k] for k in K.TOTALS] and c.res.overflow == 0
            assert np.array_equal(c.spec[:K.SPECTRUM], ref["spectrum"])


def test_exactly_half_full_is_ok(device):
    """distinct == slots / 2 is PPG_OK, one more is PPG_BUF_ERROR: k = 3, every 3-mer (64) and a table of 128 / 64."""
    import itertools
    words = ["".join(w) for w in itertools.product("ACGT", repeat=3)]
    reads = [("T" + w).encode() for w in words] + [b"ACGTTGCAAC" * 5]
    ref = K.reference(reads, 3, False)
    assert ref["distinct"] == 64
    c = Call(device, 128, k=3, flags=0, reads=reads)
    assert c() == 0 and c.res.distinct == 64 and np.array_equal(c.rows()[1], ref["counts"]) and c.guards_intact()
    assert c(slots=64) == B
    ref4 = K.reference(reads, 4, False)                                    # one key more than half of 128 rows
    assert ref4["distinct"] > 64 and Call(device, 128, k=4, flags=0, reads=reads)() == B


def test_arguments_and_optional_outputs(device):
    import torch
    ref = K.forge_reference(21, True)
    S = slots_for(ref)
    c = Call(device, S)
    n, W = c.n, c.mwords
    v = c.view
    bad_view = _lib.PpgPackedView(v.seq_off, v.seq_len, None, v.mask, None, n)
    odd_view = _lib.PpgPackedView(v.seq_off + 4, v.seq_len, v.bases, v.mask, None, n)
    neg_view = _lib.PpgPackedView(v.seq_off, v.seq_len, v.bases, v.mask, None, -1)
    m, w = K.struct_of(21, K.CANONICAL | K.USE_MASK), K.struct_of(21, K.CANONICAL | K.USE_WINDOWS)
    with_m, with_w = dict(o=C.byref(m), mask=c.ptr("mask"), mask_cap=32 * W), dict(o=C.byref(w), win=c.ptr("win"), win_cap=n)
    cases = [(dict(ctx=None), A), (dict(o=None), A), (dict(o=C.byref(K.struct_of(32, 1))), A), (dict(o=C.byref(K.struct_of(21, 16))), A),
             (dict(s=None), A), (dict(s=C.byref(bad_view)), A), (dict(s=C.byref(odd_view)), A), (dict(s=C.byref(neg_view)), A),
             (dict(table=None), A), (dict(table=c.ptr("table", 8)), A), (dict(slots=S - 1), A), (dict(slots=32), A), (dict(slots=0), A),
             (dict(slots=-64), A), (dict(spec_cap=-1), A), (dict(mask_cap=-32), A), (dict(win_cap=-1), A),
             (dict(mask=c.ptr("mask"), mask_cap=32 * W), A), (dict(win=c.ptr("win"), win_cap=n), A),        # a buffer without its flag
             (dict(o=C.byref(m)), A), (dict(o=C.byref(w)), A),                                                # a flag without its buffer
             (dict(with_m, mask_cap=32 * W + 1), A), (dict(with_m, mask=c.ptr("mask", 2)), A), (dict(with_w, win=c.ptr("win", 4)), A),
             (dict(with_m, mask_cap=32 * W - 32), B), (dict(with_w, win_cap=n - 1), B), (dict(spec_cap=K.SPECTRUM - 1), B),
             (dict(spec_cap=0), B)]
    for kw, rc in cases:
        assert c(**kw) == rc, kw
    assert c.untouched()                                                   # ... and nothing was written
    # each optional output absent
    for kw in (dict(res=None), dict(spec=None, spec_cap=0), dict(res=None, spec=None, spec_cap=0)):
        c.buf["table"].fill_(0xA5)
        c.spec[:] = -7
        c.res = _lib.PpgKmerCountResult()
        assert c(**kw) == 0 and c.guards_intact()
        keys, counts = c.rows()
        assert np.array_equal(keys, ref["keys"]) and np.array_equal(counts, ref["counts"])
        assert c.res.kmers == (0 if "res" in kw else ref["kmers"])
        assert np.array_equal(c.spec[:K.SPECTRUM], ref["spectrum"]) if "spec" not in kw else bool((c.spec == -7).all())
    # mask and windows at their exact caps, through the C call
    bits = np.arange(n) % 3 != 0
    rows = hostile_rows(K.forge_reads(), np.random.default_rng(2))
    c.buf["mask"][:4 * W] = torch.from_numpy(K.mask_words(bits).view(np.uint8).copy()).to(c.buf["mask"].device)
    c.buf["win"][:8 * n] = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(c.buf["win"].device)
    before = {k: c.buf[k].clone() for k in ("mask", "win")}
    both = K.struct_of(21, K.CANONICAL | K.USE_MASK | K.USE_WINDOWS)
    assert c(o=C.byref(both), mask=c.ptr("mask"), mask_cap=32 * W, win=c.ptr("win"), win_cap=n) == 0 and c.guards_intact()
    want = K.reference(K.forge_reads(), 21, True, bits, rows)
    assert [getattr(c.res, k) for k in K.TOTALS] == [want[k] for k in K.TOTALS] and np.array_equal(c.rows()[0], want["keys"])
    assert all(bool((c.buf[k] == before[k]).all()) for k in before)
    # zero records (the planes of the forge, none of them read)
    z = Call(device, 64)
    z.view.records = 0
    assert z() == 0 and z.guards_intact() and z.rows()[0].size == 0
    assert [getattr(z.res, k) for k in K.TOTALS] == [0] * 10 + [-1, 0] and not z.spec[:K.SPECTRUM].any()
    # no read long enough
    z = Call(device, 64, reads=[b"", b"ACGTN", b""])
    assert z() == 0 and (z.res.records, z.res.participating, z.res.short_reads, z.res.bases, z.res.max_key) == (3, 3, 3, 5, -1)


# ---- 5. accumulate ----
@pytest.mark.parametrize("k,canonical", [(21, True), (2, False)])
def test_accumulate(k, canonical, device):
    reads = K.forge_reads()
    a, b = reads[:500], reads[500:]
    pa, pb = to_device(a, device), to_device(b, device)
    whole, ra, rb = K.forge_reference(k, canonical), K.reference(a, k, canonical), K.reference(b, k, canonical)
    union = K.reference(b, k, canonical, prior=(ra["keys"], ra["counts"]))
    assert np.array_equal(union["keys"], whole["keys"]) and np.array_equal(union["counts"], whole["counts"])
    kc = pp.KmerCount(k, canonical)
    r1 = pp.count_kmers(pa, kc, slots=slots_for(whole), device=device)
    assert_equals_reference(r1, ra)
    r2 = pp.count_kmers(pb, kc, table=r1.table, accumulate=True, device=device)
    assert r2.table is r1.table
    assert_equals_reference(r2, union)                                   # the call's totals are B's, the table's the union's
    assert [getattr(r2, n) for n in K.CALL_TOTALS] == [rb[n] for n in K.CALL_TOTALS] and r2.total_count == whole["kmers"]
    r3 = pp.count_kmers(pb, kc, table=r1.table, device=device)           # without the flag the call forgets A
    assert_equals_reference(r3, rb)
    with pytest.raises(ValueError):
        pp.count_kmers(pb, kc, accumulate=True, device=device)


# ---- 6. select and lookup ----
def test_select_lookup_and_top(device):
    import torch
    p = forge_on_device(device)
    k = 21
    kc = pp.KmerCount(k, True)
    ref = K.forge_reference(k, True)
    r = pp.count_kmers(p, kc, slots=slots_for(ref), device=device)
    tp, slots = C.c_void_p(r.table.data_ptr()), r.slots
    sel = _lib.lib.ppg_kmers_select
    for mc in (1, 2, ref["max_count"], ref["max_count"] + 1):
        want = ref["counts"] >= mc
        n = int(want.sum())
        found = C.c_int64(-1)
        assert sel(device.handle, tp, slots, mc, None, 0, C.byref(found)) == 0 and found.value == n        # count only
        for cap in (n, n - 1):
            if cap < 0:
                continue
            out = torch.full((16 * cap + GUARD,), 0xA5, dtype=torch.uint8, device=tdev(device))
            device.after_torch()
            found = C.c_int64(-1)
            rc = sel(device.handle, tp, slots, mc, C.c_void_p(out.data_ptr()), cap, C.byref(found))
            assert rc == (0 if cap == n else B) and found.value == n and bool((out[16 * cap:] == 0xA5).all())
            if cap == n:
                rows = out[:16 * n].cpu().numpy().view(np.uint64).reshape(-1, 2)
                order = np.argsort(rows[:, 0])
                assert np.array_equal(rows[order, 0], ref["keys"][want]) and np.array_equal(rows[order, 1].astype(np.int64), ref["counts"][want])
        got = r.select(mc)
        assert got.shape == (n, 2) and set(got[:, 0].tolist()) == set(ref["keys"][want].tolist())
    assert sel(device.handle, tp, slots, 0, None, 0, None) == A and sel(device.handle, tp, slots + 1, 1, None, 0, None) == A
    assert sel(None, tp, slots, 1, None, 0, None) == A and sel(device.handle, tp, slots, 1, None, 5, None) == A
    assert sel(device.handle, tp, slots, 1, None, -1, None) == A and sel(device.handle, tp, slots, 1, None, 0, None) == 0
    # top(n), ties by key
    for n in (0, 1, 2, 10, 300, ref["distinct"], ref["distinct"] + 5):
        assert r.top(n) == [(K.word_of(key, k), c) for key, c in K.top(ref, n)], n
    assert r.top(1) == [(kc.word(r.max_key), r.max_count)] == [("A" * k, ref["max_count"])]
    # lookup: every present key, absent keys and the empty marker
    present = ref["keys"]
    absent = np.setdiff1d(np.random.default_rng(1).integers(0, 4 ** k, size=2000, dtype=np.uint64), present)
    keys = np.concatenate([present, absent, np.array([EMPTY, EMPTY - np.uint64(1)], np.uint64)])
    want = np.concatenate([ref["counts"], np.zeros(absent.size + 2, np.int64)])
    assert np.array_equal(r.lookup([int(x) for x in keys]), want) and absent.size > 1000
    # words are canonicalised, keys are looked up as given
    w = K.word_of(int(present[len(present) // 2]), k)
    rc = K.revcomp(w.encode()).decode()
    c = int(ref["counts"][len(present) // 2])
    assert r.lookup([w, rc, rc.encode()]).tolist() == [c, c, c] and r.lookup([]).size == 0
    assert r.lookup([pp.KmerCount(k, False).key(rc)]).tolist() == [c if rc == w else 0]
    look = _lib.lib.ppg_kmers_lookup
    dk = torch.zeros(4, dtype=torch.int64, device=tdev(device))
    assert look(None, tp, slots, C.c_void_p(dk.data_ptr()), 4, C.c_void_p(dk.data_ptr())) == A
    assert look(device.handle, tp, slots, C.c_void_p(dk.data_ptr() + 4), 2, C.c_void_p(dk.data_ptr())) == A
    assert look(device.handle, tp, slots, None, 2, C.c_void_p(dk.data_ptr())) == A and look(device.handle, tp, 63, None, 0, None) == A
    assert look(device.handle, tp, slots, None, 0, None) == 0 and look(device.handle, tp, slots, C.c_void_p(dk.data_ptr()), -1, None) == A


def test_python_layer_refuses_bad_tensors(device):
    import torch
    p = forge_on_device(device)
    dev = tdev(device)
    kc = pp.KmerCount(21)
    for kw in (dict(mask=torch.zeros(64, dtype=torch.int64, device=dev)), dict(windows=torch.zeros((p.records, 2), dtype=torch.int64, device=dev)),
               dict(windows=torch.zeros((p.records, 2), dtype=torch.int32)), dict(table=torch.zeros((128, 2), dtype=torch.int32, device=dev)),
               dict(table=torch.zeros(129, dtype=torch.int64, device=dev)), dict(windows=torch.zeros(3, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            pp.count_kmers(p, kc, device=device, **kw)
    with pytest.raises(ValueError):
        pp.count_kmers(p, pp.KmerCount(32), slots=64, device=device)
    with pytest.raises(ValueError):
        pp.count_kmers(p.to_host(), kc, device=device)
    with pytest.raises(pp.PpgError) as e:       # a table of 96 rows: the library's own check
        pp.count_kmers(p, kc, table=torch.zeros((96, 2), dtype=torch.int64, device=dev), device=device)
    assert e.value.code == A
    with pytest.raises(pp.PpgError) as e:       # a fixed size that is too small is the caller's error
        pp.count_kmers(p, kc, slots=64, device=device)
    assert e.value.code == B


# ---- 8. from files ----
def fastq_gz(reads, tag, flush_every):
    """The reads' FASTQ as one gzip member, a full flush after every flush_every records: Points fall on record
    starts, so the reference parses some records twice."""
    recs = [b"@SRR9.%d.%d\n%s\n+\n%s\n" % (i + 1, tag, s, b"I" * len(s)) for i, s in enumerate(reads)]
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = []
    for g in range(0, len(recs), flush_every):
        out.append(co.compress(b"".join(recs[g:g + flush_every])))
        out.append(co.flush(zlib.Z_FULL_FLUSH))
    out.append(co.flush())
    return b"".join(out)


def oracle_chunks(gz, cs):
    """Per chunk, from the oracle: (offset_k, raw_k, descriptors)."""
    oi = O.build_index(gz, cs)
    chunks = []
    for k in range(oi.count - 1):
        off = oi.point(k)[4]
        raw = O.extract(gz, oi, k)
        chunks.append((off, off + raw, np.asarray(O.parse(off, raw), np.uint32).reshape(-1, 4)))
    return chunks


def file_reads(which):
    """Reads a FASTQ line can hold (no '\\r', which would end up in the Sequence all the same, but no empty line
    games either): every forged read of one base or more."""
    reads = [r for r in K.forge_reads() if len(r) and b"\r" not in r]
    return reads[::2] if which == 1 else [K.revcomp(r) for r in reads[1::2]]


@pytest.fixture(scope="module")
def kmer_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmercount")
    files = []
    for which, flush, cs in ((1, 37, 20), (2, 53, 30)):
        reads = file_reads(which)
        n = min(len(file_reads(1)), len(file_reads(2)))
        gz = fastq_gz(reads[:n], which, flush)
        path = d / f"m{which}.fastq.gz"
        path.write_bytes(gz)
        chunks = oracle_chunks(gz, cs)
        seqs = [S for _, S, _ in T.fields(chunks)]
        assert len(seqs) > n + 5 and len(chunks) > 5                       # some records are parsed twice
        files.append((str(path), gz, cs, chunks, seqs))
    return files


@pytest.mark.parametrize("cap", [None, 32 << 10])
def test_batched_fastq_count_kmers(kmer_files, cap, device):
    path, gz, cs, chunks, seqs = kmer_files[0]
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    b = pp.BatchedFASTQ(ix, path, device=device)
    if cap:
        b.query_out_capacity = cap
    kc = pp.KmerCount(21, True)
    plain = K.reference(seqs, 21, True)                                    # twice-parsed records count twice
    r = b.CountKmers(kc)
    assert (b._query_shard().batches > 1) == bool(cap)
    assert_equals_reference(r, plain)
    assert r.retries >= 1 and r.slots >= 2 * plain["distinct"]             # sized by doubling
    assert_equals_reference(b.CountKmers(pp.KmerCount(16, False), slots=slots_for(K.reference(seqs, 16, False))),
                            K.reference(seqs, 16, False))
    # trim + filter + dedup chained onto one mask and one rows tensor
    pattern, f, t = b"GAT", F.Filter(F.LENGTH, 40, 8192, 0, 33, 0, 20, 0), T.FIXED._replace(min_len=25)
    keep = Q.query_reference(chunks, pattern)["hit"] & F.filter_reference(chunks, f)["pass"]
    tref = T.trim_reference(chunks, t)
    keep &= tref["keep"]
    first = D.dedup_reference(chunks, D.dedup(0), keep, tref["rows"])["unique_bits"]
    assert 0 < first.sum() < keep.sum() < keep.size
    want = K.reference(seqs, 21, True, first, tref["rows"])
    got = b.CountKmers(kc, pattern=pattern, filter=_lib.PpgReadFilter(*f), trim=T.struct_of(t), dedup=pp.ReadDedup())
    assert_equals_reference(got, want)
    assert 0 < want["kmers"] < plain["kmers"]
    # the other counts still work beside it
    assert b.CountPattern(pattern) == int(Q.query_reference(chunks, pattern)["hit"].sum())
    assert_equals_reference(b.CountKmers(kc), plain)
    b.Dispose()


@pytest.mark.parametrize("cap", [0, 32 << 10])
def test_paired_fastq_count_kmers(kmer_files, cap, device):
    ix = [pp.Core.BuildDeflateIndex(f[1], f[2]) for f in kmer_files]
    pf = paired.PairedFASTQ(ix[0], kmer_files[0][0], ix[1], kmer_files[1][0], pair_chunk=100, device=device, out_capacity=cap)
    assert [sh.batches > 1 for sh in pf.shards] == [cap > 0] * 2
    for k, canonical in ((21, True), (17, False)):
        r1, r2 = (K.reference(f[4], k, canonical) for f in kmer_files)
        union = K.reference(kmer_files[1][4], k, canonical, prior=(r1["keys"], r1["counts"]))
        r = pf.CountKmers(pp.KmerCount(k, canonical))
        assert_equals_reference(r, union)                                  # the call's totals are R2's
        assert r.records == r2["records"] and r.total_count == r1["kmers"] + r2["kmers"]
    assert r.retries >= 1
    assert sum(len(a) for _, a, _ in pf.pair_chunks()) == pf.Count()      # the pair chunks are still there after the re-runs


# ---- 9. the probe hook ----
def test_probe_hook(device):
    import torch
    p = forge_on_device(device)
    ref = K.forge_reference(21, True)
    S = slots_for(ref)
    fn = _lib.lib.ppgx_kmercount_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    view = _lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(), None, p.records)
    table = torch.zeros((S, 2), dtype=torch.int64, device=tdev(device))
    o, ms, sizes = K.struct_of(21, K.CANONICAL), (C.c_float * 6)(*[-1.0] * 6), (C.c_int64 * 4)()
    device.after_torch()
    tp = C.c_void_p(table.data_ptr())
    assert fn(device.handle, C.byref(o), C.byref(view), tp, S, 2, ms, sizes) == _lib.PPG_OK
    assert all(np.isfinite(x) for x in ms) and min(ms[0], ms[1], ms[3], ms[4], ms[5]) >= 0
    assert list(sizes) == [ref["kmers"], ref["distinct"], int((ref["counts"] >= 2).sum()), 0]
    assert fn(device.handle, C.byref(o), C.byref(view), tp, S, 0, ms, sizes) == A
    assert fn(device.handle, C.byref(K.struct_of(21, K.CANONICAL | K.ACCUMULATE)), C.byref(view), tp, S, 1, ms, sizes) == A
    assert fn(None, C.byref(o), C.byref(view), tp, S, 1, ms, sizes) == A and fn(device.handle, C.byref(o), C.byref(view), tp, S + 1, 1, ms, sizes) == A
    assert fn(device.handle, C.byref(o), C.byref(view), tp, 64, 1, ms, sizes) == _lib.PPG_OK and sizes[3] > 0     # undersized: reported
    # the call afterwards is unharmed
    assert_equals_reference(pp.count_kmers(p, pp.KmerCount(21, True), table=table, device=device), ref)
