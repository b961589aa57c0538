"""The forged FASTQ members (tests/fastq_forge.py; what each holds is asserted in
tests/test_fastq_forge_cpu.py) through the HIP path: every chunk's bytes, record descriptors,
decline flag (flags & 8 == R-P3 fails, exact in both directions: a missed decline is a wrong
answer, a spurious one a slow path), status, record base and the total against the oracle --
plain, under every ring variant, with the chain and the bytewise parse, at the census capacities
0, every byte and the boundary pair, split at the inner cuts, as lone chunks, in several output
batches, across the growth of the descriptor buffer, and through the file ingest and the cursor.
Exact equality everywhere."""
import gc

import numpy as np
import pytest

import fastq_forge as F
import parallelparsing_amd as pp
from test_gpu_parity import assert_same_run, comp_range

pytestmark = pytest.mark.gpu

RINGS = [(10, 9), (11, 9), (12, 9), (13, 9), (15, 9)]


def shard(m, device, **kw):
    return pp.Shard(m.ix, m.comp(), 0, m.n, device=device, **kw)


def check_run(sh, m):
    """every chunk of a member's run against the oracle; all mismatches are reported together
    (records first: a missed decline must show there, not only in the flag)"""
    ref = F.reference(m.name)
    r = sh.results()
    assert (r["status"] == 0).all(), r["status"]
    base = sh.record_base()
    bad_bytes, bad_rec, bad_flag, bad_base, tot = [], [], [], [], 0
    for k, c in enumerate(m.chunks):
        what = (m.name, m.level, k, c.klass, c.mod)
        if r["produced"][k] != len(c.text) or (sh.batches == 1 and sh.chunk_bytes(k).tobytes() != c.text):
            bad_bytes.append(what)
        got = sh.chunk_records(k)
        if not np.array_equal(got, ref[k]) or r["records"][k] != len(ref[k]):
            bad_rec.append(what + (len(got), len(ref[k])))
        if bool(r["flags"][k] & 8) != F.must_decline(c.raw):
            bad_flag.append(what + (int(r["flags"][k]),))
        if base[k] != tot:
            bad_base.append(what)
        tot += len(ref[k])
    # (member, level, chunk, class, out_off mod 16[, got, expected]) of the first few of each kind
    assert not (bad_bytes or bad_rec or bad_flag or bad_base), "\n".join(
        f"{len(bad)} chunks with wrong {what}: {bad[:6]}" for what, bad in
        (("records", bad_rec), ("decline flags", bad_flag), ("bytes", bad_bytes), ("record bases", bad_base)) if bad)
    assert sh.total_records == tot
    return sh


def check_lone(m, device, stride=1, ix=None):
    """the lone-chunk Decompress: the inner full-flush cuts are inner block starts it finds itself
    (or, with an index that has side points, takes from there)"""
    ref = F.reference(m.name)
    ix = ix or m.ix
    for k in range(0, m.n, stride):
        c = m.chunks[k]
        got, buf, rec = pp.Core.ExtractDeflateIndex(comp_range(m.gz, ix, k, 1), ix, k, device=device, with_records=True)
        assert buf[:got].tobytes() == c.text, (m.name, m.level, k, c.klass)
        assert np.array_equal(rec, ref[k]), (m.name, m.level, k, c.klass, c.mod, len(rec), len(ref[k]))


@pytest.mark.parametrize("level", F.LEVELS)
@pytest.mark.parametrize("name", F.NAMES)
def test_plain(name, level, device):
    check_run(shard(F.member(name, level), device).run(), F.member(name, level))


def ring_pass(dev):
    for name in ("seams", "starts"):
        for level in F.LEVELS:
            m = F.member(name, level)
            one = check_run(shard(m, dev).run(), m)
            if m.cuts:
                assert_same_run(one, check_run(shard(m, dev).set_split(*m.side).run(), m), m.n)
            check_lone(m, dev, 7 if name == "seams" else 1)


@pytest.mark.parametrize("ring,lit", RINGS)
def test_ring_variants(ring, lit, monkeypatch):
    """UNIT is 512, 1024, 2048, 4096 and 4096 bytes: a fresh context per pair (the default one is cached)"""
    monkeypatch.setenv("PPG_RING_BITS", str(ring))
    monkeypatch.setenv("PPG_LIT_BITS", str(lit))
    dev = pp.Device(0)
    try:
        ring_pass(dev)
    finally:
        del dev
        gc.collect()


@pytest.mark.parametrize("name", ["writers", "starts", "seams"])
def test_chain_and_bytewise(name, device, monkeypatch):
    for level in F.LEVELS:
        m = F.member(name, level)
        runs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("PPG_PARSE_CHAIN", mode)
            runs[mode] = check_run(shard(m, device).run(), m)
        assert_same_run(runs["1"], runs["0"], m.n)


@pytest.mark.parametrize("nl_bytes", [1 << 40, 1, 63, 64], ids=["cap0", "cap-every-byte", "cap=count", "cap=count-1"])
@pytest.mark.parametrize("name", ["writers", "seams"])
def test_census_capacity(name, nl_bytes, device, monkeypatch):
    """capacity 0 (every clean chunk with a newline goes to emit, every declined one to serial),
    a position per byte (place and chain), and the pair of values that put the boundary chunk of
    `writers` at count == capacity (place) and count == capacity + 1 (emit)"""
    monkeypatch.setenv("PPG_NL_BYTES", str(nl_bytes))
    for level in F.LEVELS:
        m = F.member(name, level)
        check_run(shard(m, device).run(), m)


@pytest.mark.parametrize("nl_bytes", [None, 1 << 40, 1], ids=["default", "cap0", "cap-every-byte"])
@pytest.mark.parametrize("name", ["split_seams", "lone_pieces", "seams", "writers"])
def test_split(name, nl_bytes, device, monkeypatch):
    """split at the inner cuts (at the default capacity the merge-overflow chunks of split_seams
    overflow only in ppg_split_merge): the oracle's results, and the unsplit run's"""
    if nl_bytes is not None:
        monkeypatch.setenv("PPG_NL_BYTES", str(nl_bytes))
    for level in F.LEVELS:
        m = F.member(name, level)
        assert len(m.cuts) >= 6
        one = check_run(shard(m, device).run(), m)
        sp = check_run(shard(m, device).set_split(*m.side).run(), m)
        assert_same_run(one, sp, m.n)


@pytest.mark.parametrize("name,stride", [("starts", 1), ("split_seams", 1), ("lone_pieces", 1), ("seams", 7)])
def test_lone_chunk(name, stride, device):
    """The lone-chunk Decompress cuts a chunk at inner block starts it finds in every 16 KiB of
    compressed bytes: lone_pieces' level-6 chunks at their hazard's cut, which puts the materialize
    kernel's census and its carry (the history's last byte) on the seam."""
    for level in F.LEVELS:
        m = F.member(name, level)
        before = device.decompress_chunk_stats()
        check_lone(m, device, stride)
        after = device.decompress_chunk_stats()
        if name == "lone_pieces" and level == 6:
            assert after["side_points"] - before["side_points"] >= len(m.cuts), (before, after)
        if m.cuts:
            check_lone(m, device, stride, m.index(side=True))


def test_multi_batch(device):
    """out_off restarts with every batch: every alignment of `seams` changes"""
    for level in F.LEVELS:
        m = F.member("seams", level)
        sh = shard(m, device, out_capacity=len(m.text) // 5).run()
        assert sh.batches >= 5
        check_run(sh, m)


@pytest.mark.parametrize("out_capacity", [0, F.GROWTH_OUT_CAPACITY], ids=["one-batch", "batches"])
@pytest.mark.parametrize("variant", F.GROWTH)
def test_growth(variant, out_capacity, device):
    """the descriptor buffer grows in the batch of the crossing chunk (the variant's writer runs
    again); the earlier batches' descriptors survive"""
    for level in F.LEVELS:
        m = F.member(f"growth_{variant}", level)
        sh = shard(m, device, out_capacity=out_capacity).run()
        assert sh.batches == (1 if not out_capacity else len(F.batches([len(c.text) for c in m.chunks], out_capacity)))
        check_run(sh, m)
        check_run(sh.run(), m)          # and again, into the grown buffer


@pytest.mark.parametrize("name", ["writers", "starts"])
def test_file_counts(name, device, tmp_path):
    for level in F.LEVELS:
        m = F.member(name, level)
        p = tmp_path / f"{name}{level}.gz"
        p.write_bytes(m.gz)
        rec, tot, _ = pp.decompress_file(m.ix, str(p), piece_bytes=1, threads=3, device=device)
        assert [int(x) for x in rec] == [len(x) for x in F.reference(name)]
        assert tot == sum(len(x) for x in F.reference(name))


def test_cursor(device, tmp_path):
    """Batch.raw(k) == offset ++ chunk (ppg_pack_raw's head / word / tail split over offsets of 0,
    1, 255, 256, 257 and 32768 bytes) and Batch.records(k) == the oracle's"""
    ref = F.reference("writers")
    for level in F.LEVELS:
        m = F.member("writers", level)
        p = tmp_path / f"w{level}.gz"
        p.write_bytes(m.gz)
        cur = pp.Cursor(m.ix, str(p), batch_bytes=len(m.text) // 4, threads=2, device=device)
        assert cur.batches >= 3
        k = base = 0
        for b in cur:
            assert (b.first_chunk, b.record_base) == (k, base)
            for j in range(b.nchunks):
                c = m.chunks[k]
                assert b.raw(j).tobytes() == c.raw, (level, k, c.klass)
                assert np.array_equal(b.records(j), ref[k]), (level, k, c.klass)
                base += len(ref[k])
                k += 1
        cur.close()
        assert k == m.n
