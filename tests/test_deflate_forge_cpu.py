"""The hand-forged DEFLATE members (tests/deflate_forge.py) on the CPU: each valid member is what it
claims to be (zlib, the gzip trailer, the oracle's CreateIndex / Decompress at dense Points and as
one whole-member chunk, the host CreateIndex) and really contains the feature it was written for
(the census, with explicit minimums); each invalid one is rejected by zlib and by the oracle with
Z_DATA_ERROR.  tests/test_gpu_forged_streams.py runs the same members through the HIP path."""
import itertools
import zlib

import pytest

import deflate_forge as F
import parallelparsing_amd as pp
from oracle import oracle as O

VALID = ["long_codes", "root_edges", "fixed_hi", "reach", "len258", "headers", "stored"]
INVALID = [c.name for c in F.invalid_cases()]
BIG = 1 << 30


@pytest.fixture(scope="module")
def census():
    """name -> (text, blocks, tokens) from the pure-Python inflater, once per member"""
    return {n: F.inspect(m.deflate) for n, m in F.valid_members().items()}


def outputs(gz, chunksize):
    ix = O.build_index(gz, chunksize)
    return [ix.point(k)[0] for k in range(ix.count)]


def test_member_list():
    assert sorted(F.valid_members()) == sorted(VALID)
    assert len(INVALID) == len(set(INVALID)) >= 15


def test_writer_primitives():
    w = F.BitWriter()
    w.bits(0b101, 3)
    w.code(0b110, 3, name="c")           # MSB first: 1, 1, 0 follow the field's 1, 0, 1
    w.bits(0xABC, 12, name="f")
    assert w.pos == 18 and w.getvalue() == bytes([0b00011101, 0b10101111, 0b10])
    assert F.patch_bits(w.getvalue(), w.fields["c"], 0b011) == bytes([0b00110101, 0b10101111, 0b10])
    assert F.patch_bits(w.getvalue(), w.fields["f"], 0) == bytes([0b00011101, 0, 0])
    # RFC 1951 3.2.2's example
    assert F.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == {0: (2, 3), 1: (3, 3), 2: (4, 3), 3: (5, 3), 4: (6, 3), 5: (0, 2),
                                                      6: (14, 4), 7: (15, 4)}
    assert F.kraft_left(F.LADDER) == 0 and F.kraft_left(F.CL_DEFAULT) == 0 and F.kraft_left(F.FIXED_LL) == 0
    assert F.apply([b"ab", (5, 2), 99, (3, 1)]) == b"abababac" + b"ccc"
    assert F.apply([(4, 3)], b"xyz") == b"xyzx"
    assert [F.len_symbol(n)[0] for n in (3, 10, 11, 257, 258)] == [257, 264, 265, 284, 285]
    assert F.len_symbol(258, 284) == (284, 5, 31)
    assert [F.dist_symbol(d)[0] for d in (1, 4, 5, 24576, 24577, 32768)] == [0, 3, 4, 28, 29, 29]


@pytest.mark.parametrize("name", VALID)
def test_valid_member(name, census):
    m = F.valid_members()[name]
    assert zlib.decompress(m.gz, 31) == m.text == census[name][0]
    assert zlib.decompress(m.deflate, -15) == m.text
    assert int.from_bytes(m.gz[-8:-4], "little") == zlib.crc32(m.text)
    assert int.from_bytes(m.gz[-4:], "little") == len(m.text)
    for cs in (9, BIG):
        ix = O.build_index(m.gz, cs)
        outs = [ix.point(k)[0] for k in range(ix.count)]
        assert outs[0] == 0 and outs[-1] == len(m.text)
        assert ix.count == 2 if cs == BIG else ix.count >= 4
        for k in range(ix.count - 1):
            assert O.extract(m.gz, ix, k) == m.text[outs[k]:outs[k + 1]], (cs, k)
        hx = pp.Core.BuildDeflateIndex(m.gz, cs)         # the product's host CreateIndex: the same Points
        assert hx.Count == ix.count
        for k in range(ix.count):
            o, n, b, w, off = ix.point(k)
            p = hx[k]
            assert (p.Output, p.Input, p.Bits, bytes(p.Window), bytes(p.offset)) == (o, n, b, w, off), (cs, k)


def regions(tokens, outs):
    """[(token, chunk position, region)] under the chunking given by the Points' outputs"""
    res = []
    for t in tokens:
        _, cpos, clen = F.chunk_of(outs, t.pos)
        res.append((t, cpos, F.region(cpos, clen)))
    return res


def test_census_long_codes(census):
    m = F.valid_members()["long_codes"]
    _, blocks, toks = census["long_codes"]
    t48 = [t for t in toks if t.nbits == 48]
    assert len(t48) >= 100
    for t in t48:   # 15-bit litlen code + 5 extra + 15-bit distance code + 13 extra
        assert (t.ll_bits, t.d_bits, t.lsym, t.dsym >= 28) == (15, 15, 284, True)
    assert {t.bit % 32 for t in t48} == set(range(32))            # one at each stream bit offset mod 32
    assert {t.dsym for t in t48} == {28, 29}
    assert {t.dextra for t in t48} >= {0x1FFF} and {t.lextra for t in t48} >= {0, 31}
    assert any(t.dist == 32768 and t.length == 258 for t in t48)
    whole = regions(t48, outputs(m.gz, BIG))
    n = {r: sum(1 for _, _, x in whole if x == r) for r in ("early", "middle", "tail")}
    assert n["early"] >= 32 and n["middle"] >= 32 and n["tail"] >= 1, n
    dense = outputs(m.gz, 9)
    assert len(dense) >= 10
    assert len({F.chunk_of(dense, t.pos)[0] for t in t48}) >= 8   # and in eight dense chunks (window history)
    assert {t.nbits for t in toks if t.length} >= {48, 32, 19}


def test_census_root_edges(census):
    _, blocks, toks = census["root_edges"]
    for lb, db in itertools.product((8, 9, 10), (8, 9)):          # LBT, LBT+1 for both roots; DB, DB+1
        hit = [t for t in toks if t.ll_bits == lb and t.d_bits == db and 281 <= t.lsym <= 284 and t.dsym >= 28]
        assert any(t.lextra == 31 and t.dextra == 0x1FFF for t in hit), (lb, db)
        assert any(t.lextra == 0 and t.dextra == 0 for t in hit), (lb, db)
    assert any(t.lsym == 284 and t.lextra == 31 for t in toks)    # 258 written as 284 + 31
    assert any(t.dist == 32768 for t in toks) and any(t.dist == 1 for t in toks)


def test_census_fixed_hi(census):
    _, blocks, toks = census["fixed_hi"]
    assert all(b.btype == 1 for b in blocks) and len(blocks) >= 4
    nine = [t for t in toks if t.length == 0 and t.ll_bits == 9]
    assert len(nine) >= 1000 and {t.lsym for t in nine} == set(range(144, 256))
    assert any(t.length == 258 for t in toks) and any(t.dsym == 28 for t in toks)
    # a 9-bit literal right before and right after a match (the bit-serial path next to the table path)
    assert any(a.length == 0 and a.ll_bits == 9 and b.length for a, b in zip(toks, toks[1:]))
    assert any(b.length == 0 and b.ll_bits == 9 and a.length for a, b in zip(toks, toks[1:]))


def test_census_reach(census):
    m = F.valid_members()["reach"]
    _, blocks, toks = census["reach"]
    assert len(m.text) >= 2 * 4096 + 32768
    whole = regions([t for t in toks if t.length], outputs(m.gz, BIG))
    for reach, dd, reg in itertools.product(F.REACHES, (-1, 0, 1), ("early", "middle", "tail")):
        assert any(t.dist == reach + dd and r == reg for t, _, r in whole), (reach, dd, reg)
    # copy_match's test is distance + length <= REACH: both sides of it, short and 258-byte matches
    for reach, dd in itertools.product(F.REACHES, (-1, 0, 1)):
        for n in (64, 258):
            assert any(t.dist + t.length == reach + dd and t.length == n for t, _, _ in whole), (reach, dd, n)
    # dense Points: sources that begin in the Point's window and end in the chunk's own output
    dense = regions([t for t in toks if t.length], outputs(m.gz, 9))
    straddle = [t for t, cpos, _ in dense if t.dist > cpos > t.dist - t.length]
    assert len(straddle) >= 6
    assert any(t.dist < t.length for t in straddle)               # one of them overlapping its own output
    for reach, dd in itertools.product(F.REACHES, (-1, 0, 1)):    # and REACH+-1 with the source in the window
        assert any(t.dist == reach + dd and t.dist > cpos for t, cpos, _ in dense), (reach, dd)


def test_census_len258(census):
    m = F.valid_members()["len258"]
    _, blocks, toks = census["len258"]
    assert len(m.text) >= 2 * 4096 + 32768
    mt = [t for t in toks if t.length]
    assert {t.dist for t in mt if t.length == 258} >= set(range(1, 66))
    runs = [len(list(g)) for k, g in itertools.groupby(toks, lambda t: t.length == 258) if k]
    assert max(runs) >= 18 and sum(1 for r in runs if r >= 18) >= 5   # walk-less carried rounds
    assert sum(1 for t in mt if t.dist == 32768) >= 6
    assert any(t.pos < 32768 < t.pos + t.length for t in mt)      # across pos == 32768
    for unit in (512, 1024, 2048, 4096):                          # across a flush UNIT boundary of every ring
        cross = [t for t in mt if t.length == 258 and t.pos // unit != (t.pos + 257) // unit]
        assert len(cross) >= 8, unit
    dense = regions(mt, outputs(m.gz, 9))
    assert sum(1 for t, cpos, _ in dense if cpos == 0 and t.dist == 32768) >= 3   # chunk position 0 takes dict[0]
    whole = regions(mt, outputs(m.gz, BIG))
    assert {r for t, _, r in whole if t.length == 258} == {"early", "middle", "tail"}


def test_census_headers(census):
    _, blocks, toks = census["headers"]
    dyn = [b for b in blocks if b.btype == 2]
    nz = lambda v: [l for l in v if l]
    one = [i for i, b in enumerate(blocks) if b.btype == 2 and nz(b.d_lens) == [1]]
    assert any(t.length and t.block in one for t in toks)         # one 1-bit distance code, and it is used
    assert any(nz(b.d_lens) == [] and b.out_len for b in dyn)     # no distance code at all
    assert any((b.hlit, b.hdist) == (257, 1) for b in dyn)
    full = [i for i, b in enumerate(blocks) if (b.hlit, b.hdist) == (286, 30) and all(b.ll_lens) and all(b.d_lens)]
    assert any(t.length and t.block in full for t in toks)
    assert {b.hclen for b in dyn} >= {5, 19}
    assert set().union(*(b.cross for b in dyn)) == {16, 17, 18}   # repeats across the litlen->distance boundary
    assert {b.btype for b in blocks if b.out_len == 0} == {0, 1, 2}   # only end-of-block / an empty stored block
    assert any(nz(b.ll_lens) == [1] for b in dyn)                 # the lone 1-bit end-of-block code
    runs = [len(list(g)) for k, g in itertools.groupby(blocks, lambda b: b.out_len == 0) if k]
    assert sorted(runs)[-2:] >= [300, 300]                        # hundreds of empty blocks in a row, twice


def test_census_stored(census):
    m = F.valid_members()["stored"]
    _, blocks, toks = census["stored"]
    st = [b for b in blocks if b.btype == 0]
    assert {(b.bit % 8, b.out_len) for b in st} >= set(itertools.product(range(8), (0, 1, 65535)))
    for b in st[1:]:    # every padding bit between the 3 header bits and the byte boundary is a one
        for p in range(b.bit + 3, b.bit + 3 + (-(b.bit + 3) % 8)):
            assert m.deflate[p >> 3] >> (p & 7) & 1, (b.bit, p)
    assert sum(-(b.bit + 3) % 8 for b in st) >= 3 * sum(range(8))


@pytest.mark.parametrize("name", INVALID)
def test_invalid_case(name):
    c = next(c for c in F.invalid_cases() if c.name == name)
    assert len(c.bad) == len(c.clean.gz) and c.bad != c.clean.gz
    assert zlib.decompress(c.clean.gz, 31) == c.clean.text
    with pytest.raises(zlib.error) as e:
        zlib.decompress(c.bad, 31)
    assert "Error -3" in str(e.value) and c.rule in str(e.value)
    ix = O.build_index(c.clean.gz, 9)
    assert ix.count == 4                                          # the patched block is chunk 1 of 3
    lo, hi = ix.point(1)[1], ix.point(2)[1]
    diff = [i for i in range(len(c.bad)) if c.bad[i] != c.clean.gz[i]]
    assert lo - 1 <= diff[0] and diff[-1] < hi
    for k in (0, 2):
        assert O.extract(c.bad, ix, k) == O.extract(c.clean.gz, ix, k)
    with pytest.raises(O.OracleError) as e:
        O.extract(c.bad, ix, 1)
    assert e.value.code == -3
    for cs in (9, BIG):
        with pytest.raises(O.OracleError) as e:
            O.build_index(c.bad, cs)
        assert e.value.code == -3
        with pytest.raises(pp.PpgError) as e:
            pp.Core.BuildDeflateIndex(c.bad, cs)
        assert e.value.code == -3


def test_type3_peek_case():
    """zlib reads the next block's type before it returns the chunk's last byte"""
    m, bad = F.type3_peek_case()
    ix = O.build_index(m.gz, 9)
    assert ix.count == 4 and ix.point(1)[2] >= 3                  # Bits: the header is inside chunk 0's slice
    for k in (0, 1):
        with pytest.raises(O.OracleError) as e:
            O.extract(bad, ix, k)
        assert e.value.code == -3
    assert O.extract(bad, ix, 2) == m.text[ix.point(2)[0]:]


def test_distinct_error_rules():
    """at least fifteen different rules: a rule is zlib's message plus which field breaks it"""
    cases = F.invalid_cases()
    assert len({c.rule for c in cases if c.rule}) >= 10           # of zlib 1.2.11's eleven inflate messages
    assert len(cases) >= 20


@pytest.mark.parametrize("at", [1, 30000])
def test_far_start_member(at):
    """a match that reaches before output position 0 of the member: CreateIndex has no history"""
    gz, text = F.far_start_member(at)
    assert int.from_bytes(gz[-8:-4], "little") == zlib.crc32(text) and text[at:at + 3] == b"\0\0" + text[:1]
    with pytest.raises(zlib.error) as e:
        zlib.decompress(gz, 31)
    assert "invalid distance too far back" in str(e.value)
    d = zlib.decompressobj(-15, zdict=bytes(32768))               # with a zero dictionary it is that text
    assert d.decompress(gz[10:-8]) == text
    for cs in (9, BIG):
        with pytest.raises(O.OracleError) as e:
            O.build_index(gz, cs)
        assert e.value.code == -3
        with pytest.raises(pp.PpgError) as e:
            pp.Core.BuildDeflateIndex(gz, cs)
        assert e.value.code == -3
