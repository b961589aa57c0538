"""Record selection on the GPU (ppg_seqselect.hip through the shard ABI, the select cursor and the
Python layer) against the reference of the semantics (tests/seqselect_ref.py): record numbers,
offsets, rebased descriptors and bytes, all exact.  Inputs: every golden case and the synthetic
Illumina file under the query tests' patterns, and the shared masks on the inputs that reach the
offset carry, the duplicates and malformed text, on a forged file whose record lengths cover every
alignment of the copy kernel, on one of very short records and on one of records longer than the copy
kernel's span; tests/test_seqselect_cpu.py guards
that they are what they claim."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
from conftest import GOLDEN, load_case
import seqpack_ref as R
import seqquery_ref as Q
import seqselect_ref as S

pytestmark = pytest.mark.gpu

ARRAYS = ("recno", "sel_off", "desc", "bytes")


def comp_range(gz, index, first, n):
    _, i0, _, _ = index.point_fields(first)
    _, i1, _, _ = index.point_fields(first + n)
    return np.frombuffer(gz[i0 - 1:i1], np.uint8)


def make_shard(name, device, **kw):
    gz, cs = S.load_input(name)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    n = ix.Count - 1
    return pp.Shard(ix, comp_range(gz, ix, 0, n), 0, n, device=device, **kw)


def dev_mask(words, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(torch.device("cuda", device.device))


def assert_equals_reference(sel, ref):
    h = sel.to_host()
    assert (sel.records, sel.nbytes) == (h.records, h.nbytes) == (ref["records"], ref["nbytes"])
    assert h.recno.dtype == np.int64 and h.sel_off.dtype == np.int64 and h.desc.dtype == np.uint32
    for key in ARRAYS:
        assert np.array_equal(getattr(h, key), ref[key]), key


# ---- 1. a query's hits, selected ----
@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_select_query_hits_matches_reference(name, device):
    sh = make_shard(name, device).run()
    for pattern in Q.PATTERNS:
        ref = S.pattern_reference(name, pattern)
        q = sh.query_sequences(pattern, mask=True)
        assert sh.select_size(q) == (ref["records"], ref["nbytes"])
        assert_equals_reference(sh.select_records(q), ref)
    assert sh.selected is None      # no hook was attached


# ---- 2. the shared masks ----
@pytest.mark.parametrize("name", ("memlevel1_c10", "stored_c50", "malformed_c40", S.FORGED, S.TINY, S.LONG))
def test_shared_masks(name, device):
    sh = make_shard(name, device).run()
    for which in S.MASKS:
        ref = S.reference(name, which)
        m = dev_mask(S.mask_words(S.mask_bool(name, which)), device)
        assert sh.select_size(m) == (ref["records"], ref["nbytes"]), which
        assert_equals_reference(sh.select_records(m), ref)
    every = S.reference(name, "all")
    assert sh.select_size() == sh.select_size(None) == (every["records"], every["nbytes"])
    assert_equals_reference(sh.select_records(), every)                  # the NULL mask is the all-ones mask
    garbage = dev_mask(S.mask_words(S.mask_bool(name, "all"), garbage_words=1), device)
    assert_equals_reference(sh.select_records(garbage), every)           # bits past the records change nothing
    half = S.mask_words(S.mask_bool(name, "half"))
    pad = every["records"] % 32
    if pad:
        half = half.copy()
        half[-1] |= np.uint32((0xFFFFFFFF << pad) & 0xFFFFFFFF)
    assert_equals_reference(sh.select_records(dev_mask(half, device)), S.reference(name, "half"))


@pytest.mark.parametrize("name", S.WHOLE_TEXT)
def test_select_all_is_the_decompressed_text(name, device):
    """GPU against GPU and zlib, no reference module in between."""
    gz, _ = R.load_input(name)
    text = zlib.decompress(gz, 31)
    sh = make_shard(name, device).run()
    sel = sh.select_records().to_host()
    assert sel.nbytes == len(text) and sel.bytes.tobytes() == text
    assert np.array_equal(sel.bytes, sh.copy_output(0, len(text)))
    assert sel.recno.tolist() == list(range(sh.total_records))


# ---- 3. capacities ----
class Bufs:
    """Output buffers with 4 KiB of slack each, every byte 0xA5."""

    def __init__(self, device, sel_cap, byte_cap):
        import torch
        dev = torch.device("cuda", device.device)
        mk = lambda n: torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device=dev)   # noqa: E731
        self.recno, self.off, self.desc, self.bytes = mk(8 * sel_cap), mk(8 * (sel_cap + 1)), mk(16 * sel_cap), mk(byte_cap)
        self.sel_cap, self.byte_cap = sel_cap, byte_cap
        torch.cuda.synchronize(dev)

    def all(self):
        return (self.recno, self.off, self.desc, self.bytes)

    def untouched(self):
        return all(bool((t == 0xA5).all()) for t in self.all())


def _select(sh, mask, mask_cap, b, desc_shift=0, bytes_shift=0):
    rec, nb = C.c_int64(-1), C.c_int64(-1)
    rc = _lib.lib.ppg_shard_select_records(
        sh.handle, C.c_void_p(mask.data_ptr()) if mask is not None else None, mask_cap, C.c_void_p(b.recno.data_ptr()),
        C.c_void_p(b.off.data_ptr()), C.c_void_p(b.desc.data_ptr() + desc_shift), b.sel_cap,
        C.c_void_p(b.bytes.data_ptr() + bytes_shift), b.byte_cap, C.byref(rec), C.byref(nb))
    return rc, rec.value, nb.value


def test_capacities(device):
    name = S.FORGED
    ref = S.reference(name, "half")
    Sn, nbytes, total = ref["records"], ref["nbytes"], S.reference(name, "all")["records"]
    cap = (total + 31) // 32 * 32
    assert cap - 32 < total
    mask = dev_mask(S.mask_words(S.mask_bool(name, "half")), device)
    sh = make_shard(name, device)
    exact = Bufs(device, Sn, nbytes)
    assert _select(sh, mask, cap, exact)[0] == _lib.PPG_ARG_ERROR             # before any run
    sh.run()
    device.after_torch()
    assert _select(sh, mask, cap + 1, exact)[0] == _lib.PPG_ARG_ERROR         # mask_cap no multiple of 32
    assert _select(sh, mask, cap - 32, exact)[0] == _lib.PPG_BUF_ERROR        # one unit short
    short = Bufs(device, Sn - 1, nbytes)
    assert _select(sh, mask, cap, short) == (_lib.PPG_BUF_ERROR, Sn, nbytes) and short.untouched()
    short = Bufs(device, Sn, nbytes - 1)
    assert _select(sh, mask, cap, short) == (_lib.PPG_BUF_ERROR, Sn, nbytes) and short.untouched()
    assert _select(sh, mask, cap, exact, desc_shift=8)[0] == _lib.PPG_ARG_ERROR    # misaligned desc
    assert _select(sh, mask, cap, exact, bytes_shift=4)[0] == _lib.PPG_ARG_ERROR   # misaligned bytes
    assert exact.untouched()
    assert _select(sh, mask, cap, exact) == (0, Sn, nbytes)                   # exact caps
    got = [t.cpu().numpy() for t in exact.all()]
    assert np.array_equal(got[0][:8 * Sn].view(np.int64), ref["recno"])
    assert np.array_equal(got[1][:8 * (Sn + 1)].view(np.int64), ref["sel_off"])
    assert np.array_equal(got[2][:16 * Sn].view(np.uint32).reshape(-1, 4), ref["desc"])
    assert np.array_equal(got[3][:nbytes], ref["bytes"])
    for g, used in zip(got, (8 * Sn, 8 * (Sn + 1), 16 * Sn, nbytes)):
        assert (g[used:] == 0xA5).all()                                       # nothing past what is in use
    # a multi-batch shard has no resident output to select from in one call; its sizes are still known
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    assert mb.batches > 1
    assert _select(mb, None, 0, Bufs(device, 1024, 1 << 20))[0] == _lib.PPG_ARG_ERROR
    every = S.reference("memlevel1_c10", "all")
    assert mb.select_size() == (every["records"], every["nbytes"])
    hm = S.reference("memlevel1_c10", "half")
    assert mb.select_size(dev_mask(S.mask_words(S.mask_bool("memlevel1_c10", "half")), device)) == (hm["records"], hm["nbytes"])


# ---- 4. the hook ----
def test_multi_batch_hook(device):
    """memlevel1_c10 through an 8 KiB output buffer (more than 4 batches): queried and selected batch by
    batch through the same mask tensor."""
    import torch
    name, pattern = "memlevel1_c10", b"GATTAC"
    ref = S.pattern_reference(name, pattern)
    qref = Q.reference(name, pattern)
    dev = torch.device("cuda", device.device)
    plain = make_shard(name, device, out_capacity=8192).run()
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4 and sh.selected is None
    mask = torch.full((qref["mask"].size,), -1, dtype=torch.int32, device=dev)
    out = pp.SelectedRecords.empty(ref["records"], ref["nbytes"], device.device)
    sh.set_seqquery(pattern, mask).set_select(mask, out)
    assert sh.selected is None                  # attached, not run yet
    for _ in range(2):                          # a second run starts from 0 again
        sh.run()
        assert sh.selected is out
        assert_equals_reference(sh.selected, ref)
        assert sh.seqquery.hits == ref["records"]
    # ... which is the one-batch result, and the run itself is the run without the hooks
    one = make_shard(name, device).run()
    assert_equals_reference(one.select_records(one.query_sequences(pattern, mask=True)), ref)
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    for k in range(sh.n):
        assert np.array_equal(plain.chunk_records(k), sh.chunk_records(k)), k
    # caps one short: the run fails, nothing is ready
    for sel_cap, byte_cap in ((ref["records"] - 1, ref["nbytes"]), (ref["records"], ref["nbytes"] - 1)):
        with pytest.raises(pp.PpgError) as e:
            sh.set_select(mask, pp.SelectedRecords.empty(sel_cap, byte_cap, device.device)).run()
        assert e.value.code == _lib.PPG_BUF_ERROR and sh.selected is None
    # off: the next run leaves nothing ready
    assert sh.set_select(None).run().selected is None
    # a mask computed beforehand, no query hook; and no mask at all
    sh.set_seqquery(None)
    half = S.reference(name, "half")
    hm = dev_mask(S.mask_words(S.mask_bool(name, "half")), device)
    assert_equals_reference(sh.set_select(hm, pp.SelectedRecords.empty(half["records"], half["nbytes"], device.device)).run().selected,
                            half)
    every = S.reference(name, "all")
    assert_equals_reference(sh.set_select(None, pp.SelectedRecords.empty(every["records"], every["nbytes"], device.device)).run().selected,
                            every)


# ---- 5. a failed run ----
def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_seqquery.test_failed_run_leaves_hook_unready builds it, with the hook attached."""
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    sh.set_select(None, pp.SelectedRecords.empty(1 << 12, 1 << 20, device.device))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert sh.selected is None


# ---- 6. the cursor ----
def _fields(r):
    return (r.identifier, r.sequence, r.other, r.quality)


@pytest.mark.parametrize("name", ("l6_c20", "memlevel1_c10", S.FORGED, S.TINY))
def test_select_cursor_and_where(name, tmp_path, device):
    """S.TINY: a batch holds more records than a slot is sized for at open and b"A" hits more of them
    than its pinned side starts with, so the slot's device and pinned buffers both grow."""
    gz, cs = S.load_input(name)
    p = tmp_path / (name + ".fastq.gz")
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    total = S.reference(name, "all")["records"]
    batch_bytes = 64 << 10
    pattern = b"A" if name == S.TINY else b"GATTAC"
    for pat, ref in ((pattern, S.pattern_reference(name, pattern)), (b"", S.reference(name, "all"))):
        cur = pp.Cursor(ix, str(p), batch_bytes=batch_bytes, device=device, pattern=pat)
        assert cur.batches > 1
        got = {k: [] for k in ARRAYS}
        scanned = nbytes = 0
        for b in cur:
            sel = b.selected
            assert b.text is None and b.desc is None and b.record_base == scanned
            assert sel.sel_off[0] == 0 and sel.sel_off[-1] == sel.nbytes == sel.bytes.size
            assert ((sel.recno >= b.record_base) & (sel.recno < b.record_base + b.nrecords)).all()
            got["recno"].append(sel.recno.copy())
            got["sel_off"].append(sel.sel_off[:-1] + nbytes)      # batch-relative -> file-relative
            got["desc"].append(sel.desc.copy())
            got["bytes"].append(sel.bytes.copy())
            scanned += b.nrecords
            nbytes += sel.nbytes
        cur.close()
        assert scanned == total and nbytes == ref["nbytes"]
        assert np.array_equal(np.concatenate(got["recno"]), ref["recno"])
        assert np.array_equal(np.concatenate(got["sel_off"] + [np.array([nbytes])]), ref["sel_off"])
        assert np.array_equal(np.concatenate(got["desc"]).reshape(-1, 4), ref["desc"])
        assert np.array_equal(np.concatenate(got["bytes"]), ref["bytes"])
    # BatchedFASTQ.Where against the text enumerator filtered on the host
    b = pp.BatchedFASTQ(ix, str(p), device=device)
    b.batch_bytes = batch_bytes
    everything = [_fields(r) for r in b]
    want = [f for f in everything if pattern in f[1]]
    assert [_fields(r) for r in b.Where(pattern)] == want
    assert len(want) == b.CountPattern(pattern)
    assert [_fields(r) for r in b.Where(None)] == everything
    shares = []
    for rank in range(2):
        rb = pp.BatchedFASTQ(ix, str(p), device=device, rank=rank, world=2)
        rb.batch_bytes = batch_bytes
        shares += [_fields(r) for r in rb.Where(pattern)]
    assert shares == want
