"""TEST HELPER (not a test): FASTQ-shaped texts whose every hazard of the record scan sits at a
chosen byte, as gzip members whose Points fall at chosen text bytes and carry chosen offsets.

The record scan decides per chunk, from flags the inflate flush computes on the fly, whether
"record j = newlines 4j..4j+3" of raw = offset ++ chunk may be used (R-P3: raw[0] != '\\n', no
"\\n\\n", no NUL) and which of four kernels writes the descriptors.  The flags are stitched across
16-byte lanes, steps of up to 1 KiB, the bytewise head and tail of a flush, the flush units of the
ring variants, the chunk start and the side points of a split chunk.  This module places one
hazard per chunk on each of those seams:

  body / nn_chunk / nul_chunk / nl_chunk   a chunk text of a given length from four-line records
                                           with one "\\n\\n", one NUL, or (the clean twin) single
                                           newlines at the same bytes
  Layout                                   chunks back to back, each at a wanted out_off mod 16
  Member                                   zlib with a full flush at every chunk boundary and
                                           every wanted inner cut -> the Points at exactly those
                                           bytes (asserted), the requested offsets substituted
  member(name, level)                      seams, starts, split_seams, lone_pieces, writers, growth_*

`must_decline` is R-P3 itself; `naive_records` the grouping the fast path reports; `route` the
writer a chunk goes to.  What each member holds is asserted in tests/test_fastq_forge_cpu.py.
"""
import functools
import zlib

import numpy as np

import parallelparsing_amd as pp
from oracle import oracle as O

DEFAULT_OFFSET = b"@o"          # non-empty, no newline, not ending in '\n': a chunk's hazards are its own
LINE_LENS = (10, 25, 2, 25)     # identifier, sequence, '+', quality lines, each with its '\n'
MODS = (0, 1, 8, 15)            # out_off mod 16 of the seam chunks
UNITS = (512, 1024, 2048, 4096, 8192)
LEVELS = (6, 0)
WIN = 32768
ACGT = np.frombuffer(b"ACGT", np.uint8)
CHAIN_OFFSET_NL = 1024          # kChainOffsetNl of ppg_parse.hip
NL_BYTES = 64                   # kNlBytesPerEntry of ppg_host.h
GROWTH_OUT_CAPACITY = 20000     # out_capacity of the multi-batch growth runs: the crossing chunk is in the second batch
# hazard classes the reference alone cannot see (its records equal the naive grouping): only the
# decline flag is checked there.  A hazard in a chunk's last two bytes has no complete record after
# it; an empty sequence or quality line is a field like any other; the '+' byte is skipped unread.
FLAG_ONLY = ("nn:edge:last", "nn:tail0:-1", "nn:tail1:-1", "nn:tail1:+0", "nul:last", "chain:gap-end", "chain:gap%4=1",
             "chain:gap%4=3", "serial:nul-plus-skipped")


def must_decline(raw):
    """R-P3: the 4-newline grouping may differ from Parsing.Parse"""
    return raw[:1] == b"\n" or b"\n\n" in raw or 0 in raw


def hazards(raw):
    """how many things in raw decline it"""
    a = np.frombuffer(raw, np.uint8)
    nl = a == 10
    return int(raw[:1] == b"\n") + int((nl[1:] & nl[:-1]).sum()) + int((a == 0).sum())


def naive_records(raw):
    """record j = newlines 4j..4j+3: what ppg_parse_finish + place / emit report"""
    nl = np.flatnonzero(np.frombuffer(raw, np.uint8) == 10).astype(np.uint32)
    n = nl.size // 4
    return nl[:4 * n].reshape(n, 4)


def visible(offset, text):
    """whether a missed decline would change the records (the reference differs from the grouping)"""
    return not np.array_equal(O.parse(offset, text), naive_records(bytes(offset) + bytes(text)))


def nl_capacity(ulen, nl_bytes=NL_BYTES):
    """the census capacity of a chunk (or of a piece of a split chunk) of ulen bytes"""
    return 0 if nl_bytes >= 1 << 40 else ulen // nl_bytes + 64


def route(offset, text, nl_bytes=NL_BYTES, chain=True):
    """the kernel that writes the chunk's descriptors"""
    raw = bytes(offset) + bytes(text)
    over = text.count(b"\n") > nl_capacity(len(text), nl_bytes)
    if not must_decline(raw):
        return "emit" if over else "place"
    if chain and not over and 0 not in raw and offset.count(b"\n") <= CHAIN_OFFSET_NL:
        return "chain"
    return "serial"


def initial_record_capacity(total_out):
    """records the descriptor buffer of a shard holds before it grows"""
    return total_out // 256 + 1024


def batches(lengths, out_capacity):
    """[(first chunk, end chunk)] of a shard's output batches"""
    out, b0, base, pos = [], 0, 0, 0
    for i, n in enumerate(lengths):
        if pos + n - base > out_capacity and i > b0:
            out.append((b0, i))
            b0, base = i, pos
        pos += n
    out.append((b0, len(lengths)))
    return out


# ---------------------------------------------------------------------------------- chunk texts
class Chunk:
    """text, offset, klass (what it is for), kind (None: clean; 'nn' a "\\n\\n" whose second byte is
    text[h]; 'nul' text[h] == 0; 'raw0' text[0] == '\\n' after an empty offset; 'off' the hazard is
    in the offset; 'multi' more than one), cuts (inner full-flush positions), seen (whether the
    reference alone shows a missed decline), out (the chunk's output position in its member)."""

    def __init__(self, text, klass, kind=None, h=None, offset=DEFAULT_OFFSET, cuts=()):
        self.text, self.klass, self.kind, self.h, self.offset = bytes(text), klass, kind, h, bytes(offset)
        self.cuts = tuple(sorted(cuts))
        self.out = self.seen = None
        assert len(self.text) & (len(self.text) - 1) or len(self.text) < 16, "a power-of-two chunk has no zero slack"
        if kind is not None:
            self.seen = visible(self.offset, self.text)

    @property
    def raw(self):
        return self.offset + self.text

    @property
    def mod(self):
        return self.out % 16


def _grid(length, first):
    pos, out, i = first, [], 1
    while pos < length:
        out.append(pos)
        pos += LINE_LENS[i % 4]
        i += 1
    return out


def body(length, rng, forced=(), forbid=(), nul=None, drop=0, first=7, alphabet=ACGT):
    """`length` bytes of four-line records (the first line continues the offset's identifier):
    newlines on a grid of LINE_LENS, none next to a forced one, the forced ones added, the `drop`
    grid newlines before the first forced one removed (that moves a blank line to another field).
    Identifier lines start with '@', third lines with '+'; the parser only counts lines."""
    forced = {f for f in forced if 0 <= f < length}
    s = set(_grid(length, first)) - {f + d for f in forced for d in (-1, 1)} - set(forbid) - forced
    s.discard(nul)
    if drop:
        lo = min(forced | ({nul} if nul is not None else set()), default=length)
        s -= set(sorted((p for p in s if p < lo), reverse=True)[:drop])
    s |= forced
    a = bytearray(alphabet[rng.integers(0, alphabet.size, length)].tobytes())
    for j, p in enumerate(sorted(s)):
        a[p] = 10
        q = p + 1
        if q < length and q not in s and q != nul and (j + 1) % 2 == 0:
            a[q] = b"@+"[(j + 1) // 2 % 2]
    if nul is not None:
        a[nul] = 0
    return a


def ensure_ats(a, cuts=()):
    """CreateIndex at chunk size 9 puts a Point at a block end once it has seen two '@': every
    piece between cuts gets two (in bytes no parser looks at)"""
    edges = [0, *cuts, len(a)]
    for lo, hi in zip(edges, edges[1:]):
        need = 2 - a.count(b"@", lo, hi)
        for p in range(lo, hi):
            if need <= 0:
                break
            if a[p] in b"ACGT":
                a[p] = 64
                need -= 1
        assert need <= 0, "no room for two '@'"
    return a


def _offset(lines, end_nl):
    return b"@o" + b"\nAC" * lines + (b"\n" if end_nl else b"")


def nn_chunk(length, h, rng, klass, cuts=(), **kw):
    """one "\\n\\n" with its second byte at text[h] (h == 0: the first is the offset's last byte),
    moved onto a field where the reference shows it: by dropping grid newlines before it, or by an
    offset of more lines; a few short lines follow it when the chunk ends soon after"""
    forced = {h, h - 1} if h else {h}
    if len([p for p in _grid(length, 7) if p > h + 1]) < 4:
        forced |= {h + 2, h + 4, h + 6}
    state = rng.bit_generator.state
    best = None
    for lines, drop in [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)]:
        rng.bit_generator.state = state
        text = ensure_ats(body(length, rng, forced, drop=drop, **kw), cuts)
        c = Chunk(text, klass, "nn", h, _offset(lines, h == 0), cuts)
        assert hazards(c.raw) == 1, (klass, h)
        best = best or c
        if c.seen:
            return c
    return best


def nul_chunk(length, h, rng, klass, cuts=(), **kw):
    """one NUL at text[h], on a field where the reference shows it (the '+' byte Parsing.Parse skips
    unread is none), with the newlines that end its record when the chunk ends soon after"""
    forced = set()
    if len([p for p in _grid(length, 7) if p > h]) < 4:
        forced = {h + 2, h + 4, h + 6, h + 8}
    state = rng.bit_generator.state
    best = None
    for drop in range(4):
        rng.bit_generator.state = state
        c = Chunk(ensure_ats(body(length, rng, forced, nul=h, drop=drop, **kw), cuts), klass, "nul", h, cuts=cuts)
        assert hazards(c.raw) == 1, (klass, h)
        best = best or c
        if c.seen:
            return c
    return best


def nl_chunk(length, h, rng, klass, cuts=(), **kw):
    """the clean twin: single newlines at text[h] and text[h - 2] (the closest that is no blank line)"""
    c = Chunk(ensure_ats(body(length, rng, {h, h - 2}, **kw), cuts), klass, None, h, cuts=cuts)
    assert not must_decline(c.raw) and c.text[h] == 10, (klass, h)
    return c


class Layout:
    """chunks back to back; align(mod) adds a clean filler so that the next chunk's output
    position (its out_off in a one-batch shard of the whole member) is mod modulo 16"""

    def __init__(self, seed):
        self.pos, self.chunks, self.rng = 0, [], np.random.default_rng(seed)

    def add(self, c):
        c.out = self.pos
        self.chunks.append(c)
        self.pos += len(c.text)
        return c

    def align(self, mod, end_nl=False):
        if self.pos % 16 != mod or end_nl:
            n = 208 + (mod - self.pos - 208) % 16
            self.add(Chunk(ensure_ats(body(n, self.rng, {n - 1} if end_nl else ())), "filler"))
        assert self.pos % 16 == mod
        return self.pos

    def length(self, want, end_mod=None):
        """a chunk length near `want` that is no power of two and ends at end_mod modulo 16"""
        n = want if end_mod is None else want + (end_mod - self.pos - want) % 16
        return n + 16 if n & (n - 1) == 0 else n


def auto_cuts(n, avoid):
    """two inner cuts of a long chunk, away from its hazard"""
    cuts = []
    for c in (n // 3 + 5, 2 * n // 3 + 3):
        while any(abs(c - a) < 4 for a in avoid):
            c += 9
        cuts.append(c)
    return cuts


# ---------------------------------------------------------------------------------- members
def _seam_specs(pos_mod):
    """(class, wanted length, end mod or None, g(pos, length) -> hazard address) of one out_off mod 16"""
    head = -pos_mod % 16
    a0 = lambda pos, n: pos + head                                    # noqa: E731 - the first aligned address
    spec = []
    for d in (-1, 0, 1):
        spec.append((f"lane:{d:+d}", 720, None, lambda pos, n, d=d: a0(pos, n) + 80 + d))
        if head + d >= 0:
            spec.append((f"head:{d:+d}", 720, None, lambda pos, n, d=d: a0(pos, n) + d))
        spec.append((f"step:{d:+d}", 1500, None, lambda pos, n, d=d: a0(pos, n) + 1024 + d))
    if head >= 3:
        spec.append(("head:in", 720, None, lambda pos, n: pos + head // 2))
    z = lambda pos, n: (pos + n) & ~15                                # noqa: E731 - the tail's first address
    spec.append(("tail0:-1", 720, 0, lambda pos, n: z(pos, n) - 1))
    spec.append(("tail1:-1", 720, 1, lambda pos, n: z(pos, n) - 1))
    spec.append(("tail1:+0", 720, 1, lambda pos, n: z(pos, n)))
    for d in (-1, 0, 1):
        spec.append((f"tail15:{d:+d}", 720, 15, lambda pos, n, d=d: z(pos, n) + d))
    spec.append(("tail15:in", 720, 15, lambda pos, n: z(pos, n) + 7))
    for h in (0, 1, 2):
        spec.append((f"edge:{h}", 720, None, lambda pos, n, h=h: pos + h))
    spec.append(("edge:last", 720, None, lambda pos, n: pos + n - 1))
    return spec


def _unit_specs(twin):
    spec = []
    for U in UNITS:
        for m in (1,) if twin else (1, 2):
            for d in (-1, 0, 1):
                spec.append((f"unit{U}x{m}:{d:+d}", U, m, d))
    return spec


def _nul_specs(pos_mod):
    head = -pos_mod % 16
    spec = [("nul:first", 720, None, lambda pos, n: pos),
            ("nul:word0", 720, None, lambda pos, n: pos + head + 32),
            ("nul:word15", 720, None, lambda pos, n: pos + head + 47),
            ("nul:last", 720, None, lambda pos, n: pos + n - 1),
            ("nul:tail", 720, 15, lambda pos, n: ((pos + n) & ~15) + 3)]
    if head >= 2:
        spec.append(("nul:head", 720, None, lambda pos, n: pos + head // 2))
    return spec


def seams_chunks():
    lay = Layout(11)
    long_ones = 0
    for mod in MODS:
        for kind, make in (("nn", nn_chunk), ("nl", nl_chunk)):
            for klass, want, end_mod, g in _seam_specs(mod):
                pos = lay.align(mod)
                n = lay.length(want, end_mod)
                h = g(pos, n) - pos
                assert 0 <= h < n, (klass, mod)
                if kind == "nl" and h == 0:
                    continue          # the clean twin of the chunk start is member `starts`'
                lay.add(make(n, h, lay.rng, f"{kind}:{klass}"))
            for klass, U, m, d in _unit_specs(kind == "nl"):
                pos = lay.align(mod)
                B = ((pos + 3) // U + m) * U      # the m-th UNIT boundary inside the chunk
                n = lay.length(B - pos + 100)
                h = B + d - pos
                long_ones += 1
                cuts = auto_cuts(n, (h,)) if n >= 1500 and long_ones % 2 else ()
                lay.add(make(n, h, lay.rng, f"{kind}:{klass}", cuts))
        for klass, want, end_mod, g in _nul_specs(mod):
            pos = lay.align(mod)
            n = lay.length(want, end_mod)
            lay.add(nul_chunk(n, g(pos, n) - pos, lay.rng, klass))
    return lay.chunks


def starts_chunks():
    lay = Layout(12)
    rng = lay.rng
    for mod in MODS:
        def clean(first_nl, klass, kind, *offsets):
            lay.align(mod)
            text = ensure_ats(body(304, rng, {0} if first_nl else ()))
            for offset in offsets:            # the first offset that puts the hazard where the reference shows it
                c = Chunk(text, klass, kind, 0 if first_nl else None, offset)
                if c.seen or kind is None:
                    break
            return lay.add(c)
        clean(True, "start:empty+nl", "raw0", b"")
        clean(True, "start:nl+nl", "nn", b"@o\n", b"@o\nAC\n")
        clean(False, "start:off=nl", "off", b"\n")
        clean(False, "start:off-nn", "off", b"@o\n\nAC", b"@o\nAC\n\nAC")
        clean(False, "start:off-nul", "off", b"@o\0AC")
        clean(False, "start:off-nul-last", "off", b"@oAC\0")
        clean(False, "start:clean-nl+x", None, b"@o\n")
        clean(True, "start:clean-x+nl", None, b"@oAC")
    return lay.chunks


SPLIT_CASES = (("straddle", nn_chunk, 0), ("before", nn_chunk, -1), ("after", nn_chunk, 1), ("nul-after", nul_chunk, 0),
               ("nul-before", nul_chunk, -1), ("clean-before", nl_chunk, -1), ("clean-after", nl_chunk, 0))


def split_chunks():
    lay = Layout(13)
    rng = lay.rng
    for cm in (0, 1, 15):                     # the cut's address modulo 16
        for klass, make, d in SPLIT_CASES:
            pos = lay.align(8)
            c2 = 850 + (cm - pos - 850) % 16
            lay.add(make(1300, c2 + d, rng, f"split:{klass}", (400, c2)))
    # newline counts between the chunk's own census capacity and the sum of its pieces'
    for k in range(3):
        lay.add(Chunk(ensure_ats(body(3000 + 16 * k, rng), (1000, 2000)), "split:merge-overflow", cuts=(1000, 2000)))
    lay.add(nn_chunk(3100, 1500, rng, "split:merge-overflow-blank", (1000, 2000)))
    return lay.chunks


LONE_RANGE = 16 * 1024          # kMatMinRange of ppg_find.cpp
ALNUM = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", np.uint8)


def lone_chunks():
    """Chunks the lone-chunk Decompress cuts into pieces itself: it takes the first dynamic block
    start in each LONE_RANGE of a chunk's compressed bytes after the first.  26000 bytes of
    62-letter text are about 19 KiB of level-6 output in one block (fewer symbols than the
    encoder's buffer holds at memLevel 9), so the cut after them is that block start, and the hazard
    sits on it as in split_seams.  (Stored blocks are not looked for: at level 0 these chunks are
    decoded whole.)"""
    lay = Layout(16)
    for cm in (0, 1, 15):
        for klass, make, d in SPLIT_CASES:
            pos = lay.align(8)
            c1 = 26000 + (cm - pos - 26000) % 16
            lay.add(make(lay.length(36000), c1 + d, lay.rng, f"lone:{klass}", (c1,), alphabet=ALNUM))
    lay.align(0, end_nl=True)     # (an index's last chunk is not searched: none of the above is it)
    return lay.chunks


def clean_offset(length, newlines, rng):
    """an offset of `length` bytes with `newlines` single newlines, none first or last"""
    a = bytearray(ACGT[rng.integers(0, 4, length)].tobytes())
    if length:
        a[0] = 64
    for i in range(newlines):
        p = (i + 1) * length // (newlines + 1)
        assert 0 < p < length - 1 and a[p - 1] != 10
        a[p] = 10
    return bytes(a)


def record(i, rng, n=20):
    """four lines of a record; the quality holds an '@' (two per record: a Point after every record)"""
    s = ACGT[rng.integers(0, 4, n)].tobytes()
    return [b"@r%d" % i, s, b"+r%d" % i, b"@" + s[1:].lower()]


def _blank_text(R, rng, blanks, n=20):
    """R records, blanks[g] empty lines put before line g (g == 4R: after the last)"""
    lines = [ln for i in range(R) for ln in record(i, rng, n)]
    out = bytearray()
    for g in range(4 * R + 1):
        out += b"\n" * blanks.get(g, 0)
        if g < 4 * R:
            out += lines[g] + b"\n"
    return bytes(out)


def writers_chunks():
    lay = Layout(14)
    rng = lay.rng

    def plain(n, klass, offset, forced=(), cuts=()):
        return lay.add(Chunk(ensure_ats(body(n, rng, forced), cuts), klass, offset=offset, cuts=cuts))

    # ---- place
    for olen in (0, 1, 255, 256, 257, 600, 32768):
        plain(400, f"place:olen{olen}", clean_offset(olen, 0 if olen < 16 else 3, rng))
    for onl in (0, 1, 3, 4, 5, 8):
        for r in range(4):
            n = 300
            while (onl + len(_grid(n, 7))) % 4 != r:
                n += 3
            plain(lay.length(n), f"place:onl{onl}", clean_offset(600, onl, rng))
            assert (onl + lay.chunks[-1].text.count(b"\n")) % 4 == r
            lay.chunks[-1].klass += f"%4={r}"
    lay.add(Chunk(b"@@" + ACGT[rng.integers(0, 4, 38)].tobytes(), "place:body-no-nl", offset=clean_offset(600, 5, rng)))
    lay.add(Chunk(b"@@" + ACGT[rng.integers(0, 4, 38)].tobytes(), "place:no-nl-at-all", offset=b"@oACGT"))
    plain(58, "place:records-in-offset", clean_offset(600, 8, rng))
    assert lay.chunks[-1].text.count(b"\n") == 3
    # the census-capacity boundary: 6336 bytes with 164 newlines (PPG_NL_BYTES 63: capacity 164, 64: 163)
    a = bytearray(ACGT[rng.integers(0, 4, 6336)].tobytes())
    for i in range(164):
        a[38 * i + 20] = 10
    lay.add(Chunk(ensure_ats(a), "place:cap-boundary"))
    # ---- emit: longer than two 4096-byte tiles; newlines at the first and last body byte and around
    # the tile boundaries; for mod != 0 the chunk before ends in '\n' inside the emit chunk's first word
    for mod in (0, 1, 15):
        pos = lay.align(mod, end_nl=True)
        t0 = (pos & ~15) - pos                               # the first tile's start, chunk-relative
        n = lay.length(8192 + 600)
        plain(n, "emit:tiles", DEFAULT_OFFSET, {0, n - 1, t0 + 4095, t0 + 8192, t0 + 8190})
        pos = lay.align(mod, end_nl=True)
        t0 = (pos & ~15) - pos
        plain(lay.length(8192 + 700), "emit:tiles", DEFAULT_OFFSET, {t0 + 4096, t0 + 8191}, (3000, 6000))
    # ---- chain: offset empty, 17 records, a blank line at every line gap (gap 0: raw[0] == '\n')
    R = 17
    for g in range(4 * R + 1):
        lay.add(Chunk(_blank_text(R, rng, {g: 1}), "chain:gap-end" if g == 4 * R else f"chain:gap%4={g % 4}",
                      "raw0" if g == 0 else "nn", 0 if g == 0 else None, b""))
    for g in range(0, 4 * R + 1, 4):
        lay.add(Chunk(_blank_text(R, rng, {g: 2}), "chain:double-blank", "multi", None, b""))
    # both skipped bytes of record k are '\n' (its '@' and its '+'): the walk's longest step, six
    # terminators, at every place of the 64-terminator window -- after s skipped bytes in records 0
    # and 1, so that the step starts at every terminator index modulo 4
    R = 17
    for s in range(4):
        for k in range(2 if s else 0, R):
            blanks = {g: 1 for g in (0, 2, 4)[:s]}
            blanks.update({4 * k: 1, 4 * k + 2: 1})
            lay.add(Chunk(_blank_text(R, rng, blanks), "chain:two-skips", "multi", None, b""))
    for R in (1, 15, 16, 31, 32, 33):
        # (long enough lines that the census keeps every position: no overflow, the chain's)
        lay.add(Chunk(_blank_text(R, rng, {0: 1}, 64), f"chain:R{R}", "raw0", 0, b""))
    for onl in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        for g in (4, 5, 6, 7):
            c = Chunk(_blank_text(5, rng, {g: 1}), f"chain:onl{onl}", "nn", None, b"x\n" * onl)
            if c.seen:
                break
        lay.add(c)
    # ---- serial: a NUL somewhere (record 3 of 6, offset empty)
    base = _blank_text(6, rng, {})
    ends = [i for i, b in enumerate(base) if b == 10]
    r3 = ends[11] + 1                                        # record 3's '@'
    f = [r3, ends[12] + 1, ends[13] + 1, ends[14] + 1]       # first bytes of its four lines
    for klass, p in (("serial:nul-body0", 0), ("serial:nul-id", f[0] + 2), ("serial:nul-seq", f[1] + 3),
                     ("serial:nul-plus-skipped", f[2]), ("serial:nul-qual", f[3] + 3),
                     ("serial:nul-after-record", r3)):
        a = bytearray(_blank_text(6, rng, {}))
        a[p] = 0
        lay.add(Chunk(ensure_ats(a), klass, "nul", p, b""))
    a = bytearray(_blank_text(6, rng, {}))
    a[f[2] + 1] = 0                                          # the third line's second byte: the field itself
    lay.add(Chunk(a, "serial:nul-plus", "nul", f[2] + 1, b""))
    lay.add(Chunk(_blank_text(6, rng, {}), "serial:nul-offset", "off", None, b"@o\0\nAC\n+\nAC\n"))
    return lay.chunks


GROWTH = ("place", "emit", "chain", "serial")


def growth_chunks(variant):
    """~3000 records of 24 bytes in chunks of 16; the chunk that crosses the descriptor buffer's
    initial capacity (chunk 81: records 1296..) is written by `variant`'s kernel"""
    lay = Layout(15)
    rec = lambda i: b"@g%04d\nACGTACG\n+\n@IIIII\n" % i   # noqa: E731
    i = 0

    def block(nrec, klass, blank=False):
        nonlocal i
        t = b"".join(rec(j) for j in range(i, i + nrec))
        i += nrec
        if blank:
            t = t[:24] + b"\n" + t[24:]
        return lay.add(Chunk(t, klass, "nn" if blank else None, 24 if blank else None, b""))

    for _ in range(81):
        block(16, "growth:before")
    {"place": lambda: block(16, "growth:cross"), "emit": lambda: block(64, "growth:cross"),
     "chain": lambda: block(16, "growth:cross", True), "serial": lambda: block(64, "growth:cross", True)}[variant]()
    while i < 3000:
        block(16, "growth:after")
    return lay.chunks


# ---------------------------------------------------------------------------------- gzip members
class Member:
    """name, level, gz, text, chunks; ix / oix: the library's and the oracle's index of exactly the
    chunk boundaries with the chunks' offsets; side: (bits, outputs, windows) of the inner cuts"""

    def __init__(self, name, level, chunks):
        self.name, self.level, self.chunks = name, level, chunks
        self.text = b"".join(c.text for c in chunks)
        self.outs = [c.out for c in chunks] + [len(self.text)]
        # memLevel 9: the encoder ends no block of its own before 32 Ki symbols
        z = zlib.compressobj(level, zlib.DEFLATED, 31, 9)
        parts, cuts = [], []
        for k, c in enumerate(chunks):
            lo = 0
            for cut in c.cuts + (len(c.text),):
                parts.append(z.compress(c.text[lo:cut]))
                if cut < len(c.text):
                    cuts.append(c.out + cut)
                if cut < len(c.text) or k + 1 < len(chunks):
                    parts.append(z.flush(zlib.Z_FULL_FLUSH))
                lo = cut
        parts.append(z.flush())
        self.gz = b"".join(parts)
        self.cuts = cuts
        # the library's Points at chunk size 9: one at every boundary, the wanted ones kept
        dense = pp.Core.BuildDeflateIndex(self.gz, 9)
        at = {dense.point_fields(i)[0]: i for i in range(dense.Count)}
        at[self.outs[-1]] = dense.Count - 1                    # the stream's end
        missing = [o for o in self.outs if o not in at]
        assert not missing, (name, level, "no Point at", missing[:5])
        keep = [dense[at[o]] for o in self.outs]
        offs = [c.offset for c in chunks] + [b""]
        arrays = ([p.Output for p in keep], [p.Input for p in keep], [p.Bits for p in keep],
                  np.frombuffer(b"".join(p.Window for p in keep), np.uint8), [len(o) for o in offs],
                  np.frombuffer(b"".join(offs), np.uint8))
        self.arrays = arrays
        self.ix = self.index()
        self.oix = O.index_from_points(*arrays)
        # side points: the oracle's Points at chunk size 9 strictly inside the chunks -- the inner cuts
        want = set(cuts)
        side = [(8 * n - b, o, w) for o, n, b, w, _ in O.build_index(self.gz, 9).points() if o in want]
        assert [s[1] for s in side] == cuts, (name, level, "inner cuts that are no side points")
        self.side = (np.array([s[0] for s in side], np.int64), np.array(cuts, np.int64),
                     np.frombuffer(b"".join(s[2] for s in side), np.uint8))

    @property
    def n(self):
        return len(self.chunks)

    def index(self, side=False):
        """a new index of the member's chunks; side: with the inner cuts attached as its side points"""
        ix = pp.Index.from_points(*self.arrays, chunk_max_bytes=max(len(c.text) for c in self.chunks))
        return ix.set_side_points(*self.side) if side else ix

    def comp(self, first=0, n=None):
        """the file bytes a Shard of chunks [first, first + n) reads"""
        n = self.n - first if n is None else n
        i0, i1 = self.ix.point_fields(first)[1], self.ix.point_fields(first + n)[1]
        return np.frombuffer(self.gz[i0 - 1:i1], np.uint8)


NAMES = ("seams", "starts", "split_seams", "lone_pieces", "writers") + tuple(f"growth_{v}" for v in GROWTH)


@functools.lru_cache(maxsize=None)
def chunks_of(name):
    if name.startswith("growth_"):
        return growth_chunks(name[7:])
    return {"seams": seams_chunks, "starts": starts_chunks, "split_seams": split_chunks, "lone_pieces": lone_chunks,
            "writers": writers_chunks}[name]()


@functools.lru_cache(maxsize=None)
def member(name, level=6):
    return Member(name, level, chunks_of(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's record table of every chunk of a member (the same at every level)"""
    return [O.parse(c.offset, c.text) for c in chunks_of(name)]
