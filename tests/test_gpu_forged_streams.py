"""The hand-forged DEFLATE members (tests/deflate_forge.py; what each holds is asserted in
tests/test_deflate_forge_cpu.py) through the HIP path: DecompressAll at dense Points and as one
whole-member chunk, split chunks, the lone-chunk Decompress, the file ingest and the GPU
CreateIndex, against the oracle (zlib 1.2.11) byte for byte and record for record; every invalid
member must give the oracle's Z_DATA_ERROR; and every compiled (ring bits, lit bits) instance of
the inflate kernel must give what the default one gives."""
import gc
import zlib

import numpy as np
import pytest

import deflate_forge as F
import parallelparsing_amd as pp
from conftest import load_case
from oracle import oracle as O
from test_gpu_parity import assert_same_run, comp_range, dense_side_points, sha
from test_index_gpu import same_index

pytestmark = pytest.mark.gpu

VALID = ["long_codes", "root_edges", "fixed_hi", "reach", "len258", "headers", "stored"]
INVALID = [c.name for c in F.invalid_cases()]
GOLDEN_SUBSET = ["l6_c200", "memlevel1_c10", "stored_c50", "fixed_c100", "rle_c100"]
# PPG_VARIANTS of ppg_inflate.hip: every (ring bits, litlen root bits) instance the library holds
VARIANTS = [(10, 8), (10, 9), (11, 9), (11, 8), (12, 9), (12, 8), (13, 9), (15, 9)]
BIG = 1 << 30

_ref = {}
_side = {}


def reference(name, cs):
    """(oracle chunk bytes, oracle record tables) of a forged member at a chunk size, computed once"""
    if (name, cs) not in _ref:
        m = F.valid_members()[name]
        oi = O.build_index(m.gz, cs)
        chunks = [O.extract(m.gz, oi, k) for k in range(oi.count - 1)]
        assert b"".join(chunks) == m.text
        _ref[name, cs] = (chunks, [O.parse(oi.point(k)[4], c) for k, c in enumerate(chunks)])
    return _ref[name, cs]


def side_points(key, gz, ix):
    if key not in _side:
        _side[key] = dense_side_points(gz, ix)
    return _side[key]


def run_member(name, cs, device):
    """One forged member at one chunk size through DecompressAll, checked against the oracle."""
    m = F.valid_members()[name]
    chunks, recs = reference(name, cs)
    ix = pp.Core.BuildDeflateIndex(m.gz, cs)
    n = ix.Count - 1
    assert n == len(chunks)
    sh = pp.Shard(ix, comp_range(m.gz, ix, 0, n), 0, n, device=device).run()
    r = sh.results()
    assert (r["status"] == 0).all(), r["status"]
    crc = 0
    for k in range(n):
        b = sh.chunk_bytes(k).tobytes()
        assert b == chunks[k], (name, cs, k, first_diff(b, chunks[k]))
        assert np.array_equal(sh.chunk_records(k), recs[k]), (name, cs, k)
        crc = zlib.crc32(b, crc)
        if k < n - 1:
            assert r["flags"][k] & 7 == 0, (name, cs, k, r["flags"][k])
    assert crc == int.from_bytes(m.gz[-8:-4], "little")
    assert sh.total_records == sum(len(x) for x in recs)
    return ix, sh


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, len(a), len(b)
    return min(len(a), len(b)), len(a), len(b)


def run_split(name, cs, ix, one, device):
    m = F.valid_members()[name]
    n = ix.Count - 1
    bits, outs, win = side_points((name, cs), m.gz, ix)
    if cs == BIG:
        assert bits.size >= 3
    sp = pp.Shard(ix, comp_range(m.gz, ix, 0, n), 0, n, device=device).set_split(bits, outs, win).run()
    assert_same_run(one, sp, n)


def run_extract(name, cs, ix, device, stride=1):
    m = F.valid_members()[name]
    chunks, recs = reference(name, cs)
    for k in range(0, ix.Count - 1, stride):
        got, buf, rec = pp.Core.ExtractDeflateIndex(comp_range(m.gz, ix, k, 1), ix, k, device=device,
                                                    with_records=True)
        assert buf[:got].tobytes() == chunks[k], (name, cs, k, first_diff(buf[:got].tobytes(), chunks[k]))
        assert np.array_equal(rec, recs[k]), (name, cs, k)


@pytest.mark.parametrize("cs", [9, BIG], ids=["dense", "whole"])
@pytest.mark.parametrize("name", VALID)
def test_valid_member(name, cs, device, tmp_path):
    m = F.valid_members()[name]
    ix, one = run_member(name, cs, device)
    run_split(name, cs, ix, one, device)
    run_extract(name, cs, ix, device)
    p = tmp_path / "m.gz"
    p.write_bytes(m.gz)
    rec, tot, _ = pp.decompress_file(ix, str(p), piece_bytes=1, threads=3, device=device)
    assert [int(x) for x in rec] == [len(x) for x in reference(name, cs)[1]]
    assert tot == one.total_records


@pytest.mark.parametrize("piece", [0, 1024])
@pytest.mark.parametrize("name", VALID)
def test_gpu_create_index_valid(name, piece, device):
    m = F.valid_members()[name]
    for cs in (9, BIG):
        same_index(pp.Core.BuildDeflateIndexGpu(m.gz, cs, device=device, piece_bytes=piece),
                   pp.Core.BuildDeflateIndex(m.gz, cs))


@pytest.mark.parametrize("name", INVALID)
def test_invalid_case(name, device):
    """The patched block is chunk 1 of its clean twin's three chunks (the oracle's verdicts are
    checked in test_deflate_forge_cpu.py: -3 for chunk 1 and for CreateIndex, chunks 0 and 2 clean)."""
    c = next(c for c in F.invalid_cases() if c.name == name)
    ix = pp.Core.BuildDeflateIndex(c.clean.gz, 9)
    oi = O.build_index(c.clean.gz, 9)
    assert ix.Count == oi.count == 4
    with pytest.raises(O.OracleError) as oe:
        O.extract(c.bad, oi, 1)
    code = oe.value.code
    assert code == -3
    # the bad chunk alone
    sh = pp.Shard(ix, comp_range(c.bad, ix, 1, 1), 1, 1, device=device)
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == code
    with pytest.raises(pp.PpgError) as e:
        pp.Core.ExtractDeflateIndex(comp_range(c.bad, ix, 1, 1), ix, 1, device=device, with_records=True)
    assert e.value.code == code
    # in the middle of a three-chunk shard: the two good chunks are delivered all the same
    sh = pp.Shard(ix, comp_range(c.bad, ix, 0, 3), 0, 3, device=device)
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == code
    r = sh.results()
    assert [int(s) for s in r["status"]] == [0, code, 0]
    for k in (0, 2):
        exp = O.extract(c.bad, oi, k)
        assert sh.chunk_bytes(k).tobytes() == exp, k
        assert np.array_equal(sh.chunk_records(k), O.parse(oi.point(k)[4], exp)), k
    # CreateIndex: host and GPU fail alike
    for piece in (0, 1024):
        with pytest.raises(pp.PpgError) as e:
            pp.Core.BuildDeflateIndex(c.bad, 9)
        with pytest.raises(pp.PpgError) as g:
            pp.Core.BuildDeflateIndexGpu(c.bad, 9, device=device, piece_bytes=piece)
        assert g.value.code == e.value.code == code


def test_block_type_3_seen_from_the_chunk_before(device):
    """Block type 3 whose header bits lie in the last byte of the previous chunk's slice: zlib reads
    them before it returns that chunk's last byte, so the oracle fails chunks 0 and 1."""
    m, bad = F.type3_peek_case()
    ix = pp.Core.BuildDeflateIndex(m.gz, 9)
    oi = O.build_index(m.gz, 9)
    want = []
    for k in range(3):
        try:
            O.extract(bad, oi, k)
            want.append(0)
        except O.OracleError as e:
            want.append(e.code)
    assert want == [-3, -3, 0]
    sh = pp.Shard(ix, comp_range(bad, ix, 0, 3), 0, 3, device=device)
    with pytest.raises(pp.PpgError) as e:
        sh.run()
    assert e.value.code == -3
    assert [int(x) for x in sh.results()["status"]] == want
    assert sh.chunk_bytes(2).tobytes() == O.extract(bad, oi, 2)
    for k in (0, 1):
        with pytest.raises(pp.PpgError) as e:
            pp.Core.ExtractDeflateIndex(comp_range(bad, ix, k, 1), ix, k, device=device)
        assert e.value.code == -3, k
    got, buf = pp.Core.ExtractDeflateIndex(comp_range(bad, ix, 2, 1), ix, 2, device=device)
    assert buf[:got].tobytes() == O.extract(bad, oi, 2)
    # the clean twin: the peek changes nothing
    sh = pp.Shard(ix, comp_range(m.gz, ix, 0, 3), 0, 3, device=device).run()
    assert b"".join(sh.chunk_bytes(k).tobytes() for k in range(3)) == m.text


@pytest.mark.parametrize("at", [1, 30000])
def test_create_index_match_before_member_start(at, device):
    """The token at output position `at` reaches two bytes before output position 0.  CreateIndex
    starts without history: zlib says "invalid distance too far back".  The trailer fits the text a
    zeroed history would give, so nothing but that rule can reject the member.  (A distance that
    reaches position 0 exactly is valid: members fixed_hi and reach hold some.)"""
    gz, text = F.far_start_member(at)
    for cs in (9, BIG):
        with pytest.raises(O.OracleError) as oe:
            O.build_index(gz, cs)
        assert oe.value.code == -3
        with pytest.raises(pp.PpgError) as e:
            pp.Core.BuildDeflateIndex(gz, cs)
        assert e.value.code == -3
        for piece in (0, 1024):
            with pytest.raises(pp.PpgError) as e:
                pp.Core.BuildDeflateIndexGpu(gz, cs, device=device, piece_bytes=piece)
            assert e.value.code == -3, (cs, piece)


def test_chunk_start_match_takes_dictionary(device):
    """The same construction at chunk level is no error: Decompress always installs a 32 KiB
    dictionary, and a match at distance 32768 at chunk position 0 copies dict[0]."""
    m = F.valid_members()["len258"]
    ix = pp.Core.BuildDeflateIndex(m.gz, 9)
    outs = [ix.point_fields(k)[0] for k in range(ix.Count)]
    _, _, toks = F.inspect(m.deflate)
    ks = [outs.index(t.pos) for t in toks if t.dist == 32768 and t.pos in outs]
    assert len(ks) >= 3
    chunks, _ = reference("len258", 9)
    for k in ks:
        got, buf = pp.Core.ExtractDeflateIndex(comp_range(m.gz, ix, k, 1), ix, k, device=device)
        assert buf[:got].tobytes() == chunks[k]
        assert buf[0] == ix[k].Window[0] == m.text[outs[k] - 32768]


# ---------------------------------------------------------------------------------------------
# every compiled instance of the inflate kernel
@pytest.fixture(scope="module")
def default_runs(device):
    """The default context's shards: forged members at both chunk sizes and the golden subset."""
    runs = {}
    for name in VALID:
        for cs in (9, BIG):
            m = F.valid_members()[name]
            ix = pp.Core.BuildDeflateIndex(m.gz, cs)
            n = ix.Count - 1
            runs[name, cs] = pp.Shard(ix, comp_range(m.gz, ix, 0, n), 0, n, device=device).run()
    for name in GOLDEN_SUBSET:
        meta, gz = load_case(name)
        ix = pp.Core.BuildDeflateIndex(gz, meta["chunksize"])
        n = ix.Count - 1
        runs[name, 0] = pp.Shard(ix, comp_range(gz, ix, 0, n), 0, n, device=device).run()
    yield runs
    runs.clear()


def variant_pass(dev, default_runs):
    for name in VALID:
        for cs in (9, BIG):
            ix, one = run_member(name, cs, dev)
            assert_same_run(default_runs[name, cs], one, ix.Count - 1)
            run_split(name, cs, ix, one, dev)
            run_extract(name, cs, ix, dev)
            m = F.valid_members()[name]
            same_index(pp.Core.BuildDeflateIndexGpu(m.gz, cs, device=dev, piece_bytes=1024), ix)
    for name in GOLDEN_SUBSET:
        meta, gz = load_case(name)
        ix = pp.Core.BuildDeflateIndex(gz, meta["chunksize"])
        n = ix.Count - 1
        one = pp.Shard(ix, comp_range(gz, ix, 0, n), 0, n, device=dev).run()
        for k, c in enumerate(meta["chunks"]):
            assert sha(one.chunk_bytes(k)) == c["sha256"], (name, k)
            assert sha(np.ascontiguousarray(one.chunk_records(k), "<u4").tobytes()) == c["rec_sha256"], (name, k)
        assert_same_run(default_runs[name, 0], one, n)
        bits, outs, win = side_points((name, 0), gz, ix)
        sp = pp.Shard(ix, comp_range(gz, ix, 0, n), 0, n, device=dev).set_split(bits, outs, win).run()
        assert_same_run(one, sp, n)
        for k in range(0, n, 3):
            got, buf, rec = pp.Core.ExtractDeflateIndex(comp_range(gz, ix, k, 1), ix, k, device=dev, with_records=True)
            assert sha(buf[:got]) == meta["chunks"][k]["sha256"] and len(rec) == meta["chunks"][k]["records"], (name, k)
        same_index(pp.Core.BuildDeflateIndexGpu(gz, meta["chunksize"], device=dev, piece_bytes=1024), ix)
    # an invalid member of each kind of block fails the same way in every instance
    for name in ("block_type_3", "stored_nlen", "repeat_overrun", "litlen_symbol_286", "dist_symbol_30",
                 "unused_dist_code"):
        c = next(c for c in F.invalid_cases() if c.name == name)
        ix = pp.Core.BuildDeflateIndex(c.clean.gz, 9)
        sh = pp.Shard(ix, comp_range(c.bad, ix, 0, 3), 0, 3, device=dev)
        with pytest.raises(pp.PpgError) as e:
            sh.run()
        assert e.value.code == -3 and [int(s) for s in sh.results()["status"]] == [0, -3, 0], name


@pytest.mark.parametrize("ring,lit", VARIANTS)
def test_every_kernel_variant(ring, lit, default_runs, monkeypatch):
    """ppg_open picks the instance from PPG_RING_BITS / PPG_LIT_BITS: a fresh context per pair (the
    default one is cached), one at a time.  Each has its own UNIT, REACH and root-table size."""
    monkeypatch.setenv("PPG_RING_BITS", str(ring))
    monkeypatch.setenv("PPG_LIT_BITS", str(lit))
    dev = pp.Device(0)
    try:
        variant_pass(dev, default_runs)
    finally:
        del dev
        gc.collect()    # pytest.raises leaves cycles that hold the context's shards: closed now, not later


def test_unlisted_variant_falls_back(default_runs, monkeypatch):
    """(14, 8) is not compiled: ppg_open silently takes the default (11, 8) instead"""
    monkeypatch.setenv("PPG_RING_BITS", "14")
    monkeypatch.setenv("PPG_LIT_BITS", "8")
    dev = pp.Device(0)
    try:
        for name in ("long_codes", "reach"):
            ix, one = run_member(name, BIG, dev)
            assert_same_run(default_runs[name, BIG], one, ix.Count - 1)
    finally:
        del dev
        gc.collect()


def test_device_finalised_before_its_shard():
    """The cyclic collector may finalise a Device before a Shard that refers to it (both sit in a
    cycle whenever a traceback holds them).  ppg_shard_free reads the context, so the context must
    stay open until its last shard is freed -- and close then."""
    m = F.valid_members()["fixed_hi"]
    dev = pp.Device(0)
    ix = pp.Core.BuildDeflateIndex(m.gz, BIG)
    sh = pp.Shard(ix, comp_range(m.gz, ix, 0, 1), 0, 1, device=dev)
    dev.__del__()                                   # the order the collector may choose
    assert dev.handle is not None and dev.handle.value
    assert sh.run().chunk_bytes(0).tobytes() == m.text
    sh.__del__()
    assert dev.handle is None                       # closed by its last user
