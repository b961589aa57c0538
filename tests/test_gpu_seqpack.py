"""Packed reads on the GPU (ppg_seqpack.hip through the shard ABI, the cursor ABI and the Python
layer) against the numpy reference of the format (tests/seqpack_ref.py): whole arrays, bit for bit
(integer / byte work: no tolerance).  Inputs: every golden case and a 1 MB synthetic Illumina file;
tests/test_seqpack_cpu.py guards that they reach every path of the pack kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
from conftest import GOLDEN, load_case
import seqpack_ref as R

pytestmark = pytest.mark.gpu


def comp_range(gz, index, first, n):
    _, i0, _, _ = index.point_fields(first)
    _, i1, _, _ = index.point_fields(first + n)
    return np.frombuffer(gz[i0 - 1:i1], np.uint8)


def make_shard(name, device, **kw):
    gz, cs = R.load_input(name)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    n = ix.Count - 1
    return pp.Shard(ix, comp_range(gz, ix, 0, n), 0, n, device=device, **kw)


def assert_equals_reference(h, ref, quality=True):
    for key in ("seq_off", "seq_len", "bases", "mask"):
        got = getattr(h, key)
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key]), key
    if quality:
        assert np.array_equal(h.qual, ref["qual"]), "qual"
    else:
        assert h.qual is None


@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_pack_sequences_matches_reference(name, device):
    ref = R.reference(name)
    sh = make_shard(name, device).run()
    tot, rec = sh.seq_bases()
    assert (tot, rec) == (int(ref["seq_off"][-1]), ref["seq_len"].size)
    pk = sh.pack_sequences(quality=True)
    assert pk.on_device and (pk.total_bases, pk.records) == (tot, rec)
    assert_equals_reference(pk.to_host(), ref)


@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_pack_sequences_without_quality(name, device):
    ref = R.reference(name)
    sh = make_shard(name, device).run()
    pk = sh.pack_sequences(quality=False)
    assert pk.qual is None
    assert_equals_reference(pk.to_host(), ref, quality=False)


def test_multi_batch_hook(device):
    """memlevel1_c10 through an 8 KiB output buffer (more than 4 batches), packed batch by batch."""
    name = "memlevel1_c10"
    ref = R.reference(name)
    plain = make_shard(name, device, out_capacity=8192).run()
    sh = make_shard(name, device, out_capacity=8192)
    assert sh.batches > 4
    pk = pp.PackedReads.empty(ref["seq_len"].size, int(ref["seq_off"][-1]), True, device.device)
    assert not sh.seqpack_ready
    sh.set_seqpack(pk).run()
    assert sh.seqpack_ready
    assert (pk.total_bases, pk.records) == (int(ref["seq_off"][-1]), ref["seq_len"].size)
    assert sh.seq_bases() == (pk.total_bases, pk.records)
    assert_equals_reference(pk.to_host(), ref)
    # ... which is the one-batch result, and the run itself is the run without the hook
    one = make_shard(name, device).run().pack_sequences().to_host()
    assert_equals_reference(one, ref)
    ra, rb = plain.results(), sh.results()
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    for k in range(sh.n):
        assert np.array_equal(plain.chunk_records(k), sh.chunk_records(k)), k
    sh.set_seqpack(None).run()
    assert not sh.seqpack_ready


def _planes(device, rec, tot):
    """Planes 4 KiB larger than rec records / tot bases need, every byte 0xA5."""
    import torch
    dev = torch.device("cuda", device.device)
    mk = lambda nbytes: torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)   # noqa: E731
    t = {"off": mk(8 * (rec + 1)), "len": mk(4 * rec), "bases": mk(tot // 4), "mask": mk(tot // 8), "qual": mk(tot)}
    torch.cuda.synchronize(dev)
    return t


def _pack_seq(sh, t, rec_cap, base_cap):
    tot = C.c_int64()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    return _lib.lib.ppg_shard_pack_seq(sh.handle, p(t["off"]), p(t["len"]), rec_cap, p(t["bases"]), p(t["mask"]),
                                       p(t["qual"]), base_cap, C.byref(tot))


def test_capacities(device):
    name = R.SYNTH
    sh = make_shard(name, device)
    t = _planes(device, 8, 256)
    assert _pack_seq(sh, t, 8, 256) == _lib.PPG_ARG_ERROR            # before any run
    sh.run()
    tot, rec = sh.seq_bases()
    assert _pack_seq(sh, t, rec, tot + 1) == _lib.PPG_ARG_ERROR      # base_cap no multiple of 32
    for rec_cap, base_cap in ((rec, tot - 32), (rec - 1, tot)):
        t = _planes(device, rec, tot)
        device.after_torch()
        assert _pack_seq(sh, t, rec_cap, base_cap) == _lib.PPG_BUF_ERROR
        # nothing at or past a cap is written
        assert bool((t["off"][8 * (rec_cap + 1):] == 0xA5).all()) and bool((t["len"][4 * rec_cap:] == 0xA5).all())
        assert bool((t["bases"][base_cap // 4:] == 0xA5).all()) and bool((t["mask"][base_cap // 8:] == 0xA5).all())
        assert bool((t["qual"][base_cap:] == 0xA5).all())
    # exact capacities succeed, and the 4 KiB past them stay untouched
    t = _planes(device, rec, tot)
    device.after_torch()
    assert _pack_seq(sh, t, rec, tot) == 0
    ref = R.reference(name)
    assert np.array_equal(t["qual"][:tot].cpu().numpy(), ref["qual"])
    assert np.array_equal(t["bases"][:tot // 4].cpu().numpy().view(np.uint32), ref["bases"])
    for key, used in (("off", 8 * (rec + 1)), ("len", 4 * rec), ("bases", tot // 4), ("mask", tot // 8), ("qual", tot)):
        assert bool((t[key][used:] == 0xA5).all()), key
    # a multi-batch shard has no resident output to pack from
    mb = make_shard("memlevel1_c10", device, out_capacity=8192).run()
    tot, rec = mb.seq_bases()
    assert _pack_seq(mb, _planes(device, rec, tot), rec, tot) == _lib.PPG_ARG_ERROR
    # the hook checks its caps too: the run fails, nothing is ready
    small = pp.PackedReads.empty(rec, tot - 32, True, device.device)
    with pytest.raises(pp.PpgError) as e:
        mb.set_seqpack(small).run()
    assert e.value.code == _lib.PPG_BUF_ERROR and not mb.seqpack_ready


def test_failed_run_leaves_hook_unready(device):
    """corrupt_err as test_gpu_parity.test_corrupt_streams builds it, with the hook attached."""
    meta, gz = load_case("corrupt_err")
    with open(os.path.join(GOLDEN, "corrupt_clean.gz"), "rb") as f:
        ix = pp.Core.BuildDeflateIndex(f.read(), meta["chunksize"])
    assert meta["oracle_status"] != 0
    k = meta["chunk"]
    sh = pp.Shard(ix, comp_range(gz, ix, k, 1), k, 1, device=device)
    sh.set_seqpack(pp.PackedReads.empty(1 << 12, 1 << 20, True, device.device))
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == meta["oracle_status"]
    assert not sh.seqpack_ready


def test_packed_cursor_grows_its_slot(tmp_path, device):
    """Slots are sized at open for records of 64 B or more on average (largest batch text / 64 + 4,096
    records): 24,000 records of 14 B, three chunks of ~8,100 records, one per batch, make a batch grow
    its slot before it is packed."""
    import zlib
    from oracle import oracle as O
    txt = b"".join(b"@\n%s\n+\n%s\n" % (s, q) for s, q in
                   ((b"ACGT"[i % 4:] + b"NACG"[:i % 4], b"%04d" % (i % 10000)) for i in range(24000)))
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    gz = co.compress(txt) + co.flush()
    p = tmp_path / "tiny.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, 500)
    oi = O.build_index(gz, 500)
    chunks = []
    for k in range(oi.count - 1):
        off, ch = oi.point(k)[4], O.extract(gz, oi, k)
        chunks.append((off + ch, np.asarray(O.parse(off, ch), np.uint32).reshape(-1, 4)))
    cur = pp.Cursor(ix, str(p), batch_bytes=128 << 10, device=device, packed=True, quality=True)
    assert cur.batches > 1
    most = rmax = 0
    for b in cur:
        sel = chunks[b.first_chunk:b.first_chunk + b.nchunks]
        ref = R.pack_reference([c[0] for c in sel], [c[1] for c in sel])
        assert b.nrecords == ref["seq_len"].size
        assert_equals_reference(b.packed, ref)
        most, rmax = max(most, b.nrecords), max(rmax, int(b.raw_off[-1]))
    assert most > rmax // 64 + 4096             # past what the slots were opened with
    cur.close()


@pytest.mark.parametrize("quality", [True, False])
@pytest.mark.parametrize("name", ["l6_c20", R.SYNTH])
def test_packed_cursor(name, quality, tmp_path, device):
    """64 KiB batches of whole chunks: per batch the planes equal the reference pack of that batch's
    chunks (offsets from 0); the batch's other fields equal a text cursor's."""
    gz, cs = R.load_input(name)
    p = tmp_path / "x.fastq.gz"
    p.write_bytes(gz)
    ix = pp.Core.BuildDeflateIndex(gz, cs)
    text = pp.Cursor(ix, str(p), batch_bytes=64 << 10, device=device)
    cur = pp.Cursor(ix, str(p), batch_bytes=64 << 10, device=device, packed=True, quality=quality)
    assert cur.batches == text.batches > 1
    with pytest.raises(pp.PpgError) as e:      # before the first batch
        cur.packed_reads(0)
    assert e.value.code == _lib.PPG_ARG_ERROR
    nb = 0
    for b in cur:
        tb = text.next_batch()
        with pytest.raises(pp.PpgError) as e:  # a text cursor has no planes
            text.packed_reads(tb.nrecords)
        assert e.value.code == _lib.PPG_ARG_ERROR
        assert b.text is None and b.desc is None and tb.packed is None
        assert (b.first_chunk, b.nchunks, b.record_base, b.nrecords) == \
               (tb.first_chunk, tb.nchunks, tb.record_base, tb.nrecords)
        assert np.array_equal(b.raw_off, tb.raw_off) and np.array_equal(b.rec_off, tb.rec_off)
        ref = R.reference_of_chunks(name, b.first_chunk, b.first_chunk + b.nchunks)
        assert b.packed.records == b.nrecords and b.packed.total_bases == int(ref["seq_off"][-1])
        assert_equals_reference(b.packed, ref, quality)
        nb += 1
    assert nb == cur.batches and text.next_batch() is None
    cur.close()
    text.close()
