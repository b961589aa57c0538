"""TEST HELPER (not a test): an RFC 1951 DEFLATE writer driven by explicit tokens, with no encoder.

Every compressed input the rest of the suite uses comes from a zlib-family encoder run over
FASTQ-shaped text, which never writes most of what the format allows.  This module writes streams
from explicit descriptions instead: a bit writer (LSB-first fields, MSB-first Huffman codes),
canonical codes from an explicit per-symbol length list, stored / fixed / dynamic block writers
whose every header field can be chosen, `apply` (the expected text, a byte-by-byte LZ77 copy that
shares nothing with the writer), `gzip_wrap`, `patch_bits` (overwrite a named field of a written
block in place, so an error case has the bit length of its clean twin) and `inspect`, a small
pure-Python inflater that reports what a stream contains (the census the tests assert on).

`valid_members()` and `invalid_cases()` build the forged members the CPU and GPU tests share; each
member's docstring line says which decoder branch it is written for.
"""
import collections
import functools
import struct
import zlib

# ---------------------------------------------------------------------------------- tables
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163,
            195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
             3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
# the 19 code-length symbols, Kraft-complete: 13 codes of 4 bits, 6 of 5 (16/17/18 among the 4-bit ones)
CL_DEFAULT = [4] * 10 + [5] * 6 + [4] * 3

RINGS = (1024, 2048, 4096, 8192, 32768)        # the inflate kernel's LDS ring sizes (ring bits 10..13, 15)
REACHES = tuple(r - 64 for r in RINGS)         # REACH = RING - 64: the oldest byte a match may take from the ring


def len_symbol(length, prefer=None):
    """(symbol, extra bits, extra value) of a match length; 258 may also be written as 284 + 31."""
    if prefer == 284 and length == 258:
        return 284, 5, 31
    for i in range(28, -1, -1):
        if length >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise ValueError(length)


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if dist >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise ValueError(dist)


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, nbits)} for the non-zero lengths.  An over-subscribed list
    still gets (wrapped) codes, so that a stream with such a header can be written."""
    count = collections.Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for bits in range(1, 16):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    out = {}
    for sym, l in enumerate(lengths):
        if l:
            out[sym] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def kraft_left(lengths):
    """unused code space in units of 2^-15 (0: complete, < 0: over-subscribed)"""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


def complete(req, nsyms, used=(), fillers=None):
    """A Kraft-complete length list over nsyms symbols: req {symbol: length} is kept, every other
    symbol of `used` gets one common length (the shortest that fits), and what code space is left
    goes to filler symbols no token uses, one per set bit of the remainder."""
    lens = [0] * nsyms
    for s, l in req.items():
        lens[s] = l
    rest = [s for s in sorted(set(used)) if s not in req]
    if rest:
        for L in range(1, 16):
            if kraft_left(lens) - len(rest) * (1 << (15 - L)) >= 0:
                break
        else:
            raise ValueError("no room for the used symbols")
        for s in rest:
            lens[s] = L
    left = kraft_left(lens)
    if left < 0:
        raise ValueError("over-subscribed")
    free = [s for s in (fillers if fillers is not None else range(nsyms)) if lens[s] == 0]
    for b in range(14, -1, -1):
        if left >> b & 1:
            lens[free.pop(0)] = 15 - b
    assert kraft_left(lens) == 0
    return lens


# ---------------------------------------------------------------------------------- bit writer
class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0
        self.fields = {}          # name -> (bit position, bit count, "bits" | "code")

    @property
    def pos(self):
        return 8 * len(self.buf) + self.nacc

    def bits(self, value, n, name=None):
        """an n-bit field, least significant bit first"""
        if name:
            self.fields[name] = (self.pos, n, "bits")
        self.acc |= (value & ((1 << n) - 1)) << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, code, n, name=None):
        """a Huffman code, most significant bit first"""
        if name:
            self.fields[name] = (self.pos, n, "code")
        self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def raw(self, data):
        assert self.nacc == 0
        self.buf += data

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.nacc else b"")


def patch_bits(data, field, value):
    """data with the field (pos, nbits, kind) overwritten by value; the length does not change"""
    pos, n, kind = field
    if kind == "code":
        value = int(format(value, "0%db" % n)[::-1], 2)
    a = bytearray(data)
    for i in range(n):
        p = pos + i
        a[p >> 3] = (a[p >> 3] & ~(1 << (p & 7))) | ((value >> i & 1) << (p & 7))
    return bytes(a)


# ---------------------------------------------------------------------------------- tokens
def apply(tokens, history=b""):
    """The text a token list stands for: an int is a literal, bytes a run of literals, a tuple
    (length, distance[, litlen symbol]) a byte-by-byte copy; history precedes position 0."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, (bytes, bytearray)):
            out += t
        else:
            length, dist = t[0], t[1]
            if dist > len(out):
                raise ValueError("distance %d before the start" % dist)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(history):])


def _flat(tokens):
    for t in tokens:
        if isinstance(t, (bytes, bytearray)):
            yield from t
        else:
            yield t


def used_symbols(tokens):
    ll, d = {256}, set()
    for t in _flat(tokens):
        if isinstance(t, int):
            ll.add(t)
        else:
            ll.add(len_symbol(t[0], t[2] if len(t) > 2 else None)[0])
            d.add(dist_symbol(t[1])[0])
    return ll, d


def write_tokens(w, tokens, ll_lens, d_lens, name=None, eob=True):
    ll, dc = canonical(ll_lens), canonical(d_lens)
    for i, t in enumerate(_flat(tokens)):
        tag = "%s.tok%d" % (name, i) if name else None
        if isinstance(t, int):
            w.code(*ll[t], name=tag)
            continue
        s, eb, ev = len_symbol(t[0], t[2] if len(t) > 2 else None)
        w.code(*ll[s], name=tag)
        w.bits(ev, eb)
        s, eb, ev = dist_symbol(t[1])
        w.code(*dc[s], name=tag and tag + ".dist")
        w.bits(ev, eb)
    if eob:
        w.code(*ll[256], name=name and name + ".eob")


# ---------------------------------------------------------------------------------- block writers
def stored_block(w, data, final=False, pad=0, len_=None, nlen=None, name=None):
    """BTYPE 0: pad fills the bits up to the byte boundary; LEN / NLEN can be overridden."""
    w.bits(final, 1)
    w.bits(0, 2, name and name + ".btype")
    w.bits(pad, -w.pos % 8)
    n = len(data) if len_ is None else len_
    w.bits(n, 16, name and name + ".len")
    w.bits(n ^ 0xFFFF if nlen is None else nlen, 16, name and name + ".nlen")
    w.raw(data)


def fixed_block(w, tokens, final=False, name=None):
    w.bits(final, 1)
    w.bits(1, 2, name and name + ".btype")
    write_tokens(w, tokens, FIXED_LL, FIXED_D, name)


def plain_cl(lens):
    """every code length as its own symbol: [(symbol, extra bits, extra value)]"""
    return [(l, 0, 0) for l in lens]


def rle_cl(lens):
    """greedy repeat codes 16 / 17 / 18 over the concatenated litlen + distance lengths (a run may
    cross from one alphabet into the other, as RFC 1951 allows)"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            n = min(run, 138)
            out.append((18, 7, n - 11) if n >= 11 else (17, 3, n - 3))
            i += n
        elif v and run >= 4:
            out.append((v, 0, 0))
            n = min(run - 1, 6)
            out.append((16, 2, n - 3))
            i += 1 + n
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def dynamic_block(w, tokens, ll_lens, d_lens, final=False, cl_lens=None, cl_seq=None, hlit=None, hdist=None,
                  hclen=None, name=None):
    """BTYPE 2.  ll_lens / d_lens: explicit per-symbol code lengths.  hlit / hdist default to the
    shortest counts that hold the non-zero lengths (lists shorter than the count are zero padded).
    cl_seq: the code-length symbols [(symbol, extra bits, value)], default plain_cl over
    litlen ++ distance; rle_cl gives the repeat-code form.  cl_lens: the 19 code-length-code
    lengths (default CL_DEFAULT); hclen: how many of them are written."""
    def last(v):
        return max([i + 1 for i, l in enumerate(v) if l] or [0])
    hlit = max(257, last(ll_lens)) if hlit is None else hlit
    hdist = max(1, last(d_lens)) if hdist is None else hdist
    ll_w = (list(ll_lens) + [0] * hlit)[:hlit]
    d_w = (list(d_lens) + [0] * hdist)[:hdist]
    cl_lens = CL_DEFAULT if cl_lens is None else cl_lens
    if cl_seq is None:
        cl_seq = plain_cl(ll_w + d_w)
    elif callable(cl_seq):
        cl_seq = cl_seq(ll_w + d_w)
    if hclen is None:
        hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    w.bits(final, 1)
    w.bits(2, 2, name and name + ".btype")
    w.bits(hlit - 257, 5, name and name + ".hlit")
    w.bits(hdist - 1, 5, name and name + ".hdist")
    w.bits(hclen - 4, 4, name and name + ".hclen")
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3, name and "%s.cl%d" % (name, CL_ORDER[i]))
    cc = canonical(cl_lens)
    p = 0                       # position in litlen ++ distance: a plain length is also field "lens<p>"
    for i, (s, eb, ev) in enumerate(cl_seq):
        if name and s < 16:
            w.fields["%s.lens%d" % (name, p)] = (w.pos, cc[s][1], "code")
        w.code(*cc[s], name=name and "%s.seq%d" % (name, i))
        w.bits(ev, eb, name and "%s.seq%d.extra" % (name, i))
        p += 1 if s < 16 else (3 if s < 18 else 11) + ev
    write_tokens(w, tokens, ll_w, d_w, name)


def gzip_wrap(deflate, text):
    """the 10-byte header, the stream, CRC-32 and ISIZE of text"""
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + deflate +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF))


# ---------------------------------------------------------------------------------- census
Token = collections.namedtuple("Token", "bit pos length dist lsym lextra ll_bits dsym dextra d_bits nbits block")
Block = collections.namedtuple("Block", "bit btype pos out_len hlit hdist hclen cl_syms cross ll_lens d_lens end_bit")


class _Reader:
    def __init__(self, data):
        self.d = data + b"\0" * 8
        self.p = 0

    def bits(self, n):
        v = (int.from_bytes(self.d[self.p >> 3:(self.p >> 3) + 5], "little") >> (self.p & 7)) & ((1 << n) - 1)
        self.p += n
        return v

    def sym(self, table):
        code = 0
        for n in range(1, 16):
            code = code << 1 | self.bits(1)
            s = table.get((n, code))
            if s is not None:
                return s, n
        raise ValueError("no code at bit %d" % (self.p - 15))


def _table(lengths):
    return {(n, c): s for s, (c, n) in canonical(lengths).items()}


def inspect(deflate, history=b""):
    """A pure-Python inflate of a valid stream that keeps what it saw: (text, blocks, tokens).
    tokens holds one Token per literal (length 0) or match: its stream bit offset, output position,
    symbols, code lengths, extra-bit values and total bit count; blocks one Block per block."""
    r = _Reader(deflate)
    out = bytearray(history)
    h = len(history)
    blocks, toks = [], []
    while True:
        bit = r.p
        final, btype = r.bits(1), r.bits(2)
        start = len(out) - h
        hlit = hdist = hclen = 0
        cls, cross, ll_lens, d_lens = (), set(), (), ()
        if btype == 0:
            r.bits(-r.p % 8)
            n, nn = r.bits(16), r.bits(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("stored LEN/NLEN")
            out += r.d[r.p >> 3:(r.p >> 3) + n]
            r.p += 8 * n
        elif btype in (1, 2):
            if btype == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = r.bits(3)
                ct, lens, cls = _table(cl), [], []
                while len(lens) < hlit + hdist:
                    s, _ = r.sym(ct)
                    cls.append(s)
                    before = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.bits(2))
                    else:
                        lens += [0] * (3 + r.bits(3) if s == 17 else 11 + r.bits(7))
                    if before < hlit < len(lens):
                        cross.add(s)            # a repeat that runs from the litlen lengths into the distance ones
                if len(lens) != hlit + hdist:
                    raise ValueError("repeat overruns")
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
            lt, dt = _table(ll_lens), _table(d_lens)
            nb = len(blocks)
            while True:
                tb = r.p
                s, n = r.sym(lt)
                if s < 256:
                    toks.append(Token(tb, len(out) - h, 0, 0, s, 0, n, -1, 0, 0, n, nb))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    le = r.bits(LEN_EXTRA[s - 257])
                    ds, dn = r.sym(dt)
                    de = r.bits(DIST_EXTRA[ds])
                    length, dist = LEN_BASE[s - 257] + le, DIST_BASE[ds] + de
                    toks.append(Token(tb, len(out) - h, length, dist, s, le, n, ds, de, dn, r.p - tb, nb))
                    if dist > len(out):
                        raise ValueError("distance too far back")
                    for _ in range(length):
                        out.append(out[-dist])
        else:
            raise ValueError("block type 3")
        blocks.append(Block(bit, btype, start, len(out) - h - start, hlit, hdist, hclen, tuple(cls), frozenset(cross),
                            tuple(ll_lens), tuple(d_lens), r.p))
        if final:
            return bytes(out[h:]), blocks, toks


def region(pos, chunk_len):
    """where in its chunk a token starts: the inflate kernel decodes the first 32 KiB (history still
    partly the Point's window), the middle, and the last 322 bytes with different round forms"""
    if pos >= chunk_len - 322:
        return "tail"
    return "early" if pos < 32768 else "middle"


def chunk_of(outputs, pos):
    """(chunk number, position inside it, chunk length) of member position pos; outputs: the Points'"""
    import bisect
    k = bisect.bisect_right(outputs, pos) - 1
    return k, pos - outputs[k], outputs[k + 1] - outputs[k]


# ---------------------------------------------------------------------------------- text and members
RECLEN = 64


def lcg(seed):
    x = seed & 0xFFFFFFFF
    while True:
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        yield x >> 16


def fastq_text(nrec, seed=1, qual=b"FGHIJ", bases=b"ACGT", idchars=b"0123456789"):
    """nrec FASTQ records of exactly RECLEN bytes: '@' id(8) LF seq(25) LF '+' LF qual(25) LF"""
    g = lcg(seed)
    out = bytearray()
    for i in range(nrec):
        n, ident = i, bytearray()
        for _ in range(7):
            ident.insert(0, idchars[n % len(idchars)])
            n //= len(idchars)
        out += b"@r" + ident + b"\n"
        out += bytes(bases[next(g) % len(bases)] for _ in range(25)) + b"\n+\n"
        out += bytes(qual[next(g) % len(qual)] for _ in range(25)) + b"\n"
    return bytes(out)


class Tok:
    """A token list under construction that knows its output position (and text, to pick fillers)."""

    def __init__(self, text=b""):
        self.tokens = []
        self.text = bytearray(text)
        self.base = len(text)

    @property
    def pos(self):
        return len(self.text)

    def lit(self, data):
        self.tokens.append(bytes(data))
        self.text += data
        return self

    def match(self, length, dist, prefer=None):
        assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(self.text), (length, dist, self.pos)
        self.tokens.append((length, dist) if prefer is None else (length, dist, prefer))
        for _ in range(length):
            self.text.append(self.text[-dist])
        return self

    def fill_to(self, target, dist=RECLEN, step=258):
        """FASTQ-shaped filler up to output position target: copies of whole records from dist back"""
        while self.pos < target:
            n = min(step, target - self.pos)
            if n < 3:
                self.lit(bytes(self.text[self.pos - dist + i] for i in range(n)))
            else:
                if target - self.pos - n in (1, 2):
                    n -= 2 if n >= 5 else 0
                self.match(n, dist)
        return self

    def take(self):
        """the tokens since the last take (one block's worth)"""
        t, self.tokens = self.tokens, []
        return t


class Member:
    def __init__(self, name, doc):
        self.name, self.doc = name, doc
        self.w = BitWriter()
        self.tokens = []
        self.nblocks = 0

    def _name(self):
        self.nblocks += 1
        return "b%d" % (self.nblocks - 1)

    def stored(self, data, final=False, **kw):
        self.tokens.append(bytes(data))
        stored_block(self.w, data, final, name=self._name(), **kw)

    def fixed(self, tokens, final=False):
        self.tokens += tokens
        fixed_block(self.w, tokens, final, name=self._name())

    def dynamic(self, tokens, ll_lens=None, d_lens=None, final=False, ll_req=None, d_req=None, **kw):
        """explicit lengths, or (None) a complete code over the used symbols, ll_req / d_req kept"""
        ll, d = used_symbols(tokens)
        if ll_lens is None:
            ll_lens = complete(ll_req or {}, 286, ll, fillers=[s for s in range(1, 144) if s not in ll])
        if d_lens is None:
            d_req = dict(d_req or {})
            if not d and not d_req:
                d_lens = [0]
            elif len(d | set(d_req)) == 1 and not d_req:
                d_lens = [0] * 30
                d_lens[min(d)] = 1              # one distance code of one bit: incomplete, and legal
            else:
                d_lens = complete(d_req, 30, d)
        self.tokens += tokens
        dynamic_block(self.w, tokens, ll_lens, d_lens, final, name=self._name(), **kw)

    def finish(self):
        self.deflate = self.w.getvalue()
        self.fields = self.w.fields
        self.text = apply(self.tokens)
        self.gz = gzip_wrap(self.deflate, self.text)
        return self

    def field(self, name):
        """a field's position inside self.gz"""
        p, n, k = self.fields[name]
        return p + 80, n, k


LADDER = list(range(1, 15)) + [15, 15]      # 1, 2, ..., 14, 15, 15: Kraft-complete, sixteen symbols


def m_long_codes():
    m = Member("long_codes", "15-bit litlen + 5 extra + 15-bit distance + 13 extra: the 48-bit token, at every "
               "stream bit offset mod 32, in the early, middle and tail rounds (bit-serial path)")
    alpha = b"ACGT\n@I+01r"
    t = Tok()
    t.lit(fastq_text(270, 3, qual=b"I", idchars=b"01"))          # 17,280 bytes of an 11-letter alphabet
    m.fixed(t.take())
    ll = [0] * 286
    for i, c in enumerate(alpha):
        ll[c] = i + 1                                            # 'A' 1 bit ... 'r' 11 bits
    ll[257], ll[264], ll[256], ll[284], ll[285] = 12, 13, 14, 15, 15
    dl = [0] * 30
    for s in range(14, 28):
        dl[s] = s - 13                                           # 14: 1 bit ... 27: 14 bits
    dl[28] = dl[29] = 15
    assert sorted(l for l in ll if l) == sorted(l for l in dl if l) == LADDER
    i = 0
    while t.pos < 46000:
        for _ in range(12):
            ext = (i * 7) % 32                                   # 284's extra field, 31 included (length 258)
            d = 16385 + (i * 613) % (min(t.pos, 24576) - 16384)
            if i % 2 and t.pos > 24577:
                d = 24577 + (i * 613) % (min(t.pos, 32768) - 24576)
            if i % 16 == 5 and t.pos >= 24576:
                d = 24576                                        # 28 with all thirteen extra bits set
            if i % 16 == 7 and t.pos >= 32768:
                d = 32768                                        # 29 with all thirteen extra bits set
            t.match(227 + ext, d, prefer=284)
            t.lit(b"A")                                          # 1 bit: the next 48-bit token starts 17 bits on
            i += 1
        if i % 24 == 0:
            t.match(10, 3000).match(3, 150)                      # 13 + 9 + 10 bits, 12 + 1 + 6
        m.dynamic(t.take(), ll, dl)
    t.match(258, 32768, prefer=284)                              # the member's last token, in the tail round
    m.dynamic(t.take(), ll, dl, final=True)
    return m.finish()


def m_root_edges():
    m = Member("root_edges", "litlen codes of 8, 9 and 10 bits (LBT and LBT+1 for both root sizes) on the 5-extra-bit "
               "length symbols and distance codes of 8 and 9 bits (DB, DB+1) on the 13-extra-bit symbols, extras "
               "all ones and all zeros")
    t = Tok()
    t.lit(fastq_text(520, 5))                                    # 33,280 bytes: distance 32768 is reachable
    m.fixed(t.take())
    ll_req = {281: 8, 282: 9, 283: 10, 284: 8, 285: 9, 256: 10, 280: 10}
    d_req = {29: 8, 28: 9, 27: 8, 26: 9, 0: 9, 1: 8}
    for rep in range(3):
        for ls in (281, 282, 283, 284):
            for ds in (29, 28, 27, 26, 0, 1):
                for le, de in ((31, 1), (0, 0), (31, 0), (0, 1)):
                    length = LEN_BASE[ls - 257] + le
                    dist = DIST_BASE[ds] + (de and (1 << DIST_EXTRA[ds]) - 1)
                    t.match(length, dist, prefer=284 if ls == 284 else None)
                t.lit(bytes(t.text[t.pos - RECLEN:t.pos - RECLEN + 7]))
        t.match(258, RECLEN).match(115, RECLEN * 3)
        m.dynamic(t.take(), ll_req=ll_req, d_req=d_req, final=rep == 2)
    return m.finish()


def m_fixed_hi():
    m = Member("fixed_hi", "fixed blocks whose literals 144..255 are 9-bit codes (bit-serial with the 8-bit root), "
               "next to 7-/8-bit length codes and the 5-bit distance codes with 13 extra bits")
    t = Tok()
    hi = bytes(range(144, 256))
    for b in range(6):
        t.lit(fastq_text(40, 20 + b, qual=hi))
        t.match(258, RECLEN).match(3, 1).match(115, 2 * RECLEN).match(35, 700)
        if t.pos > 16500:
            t.match(200, 16385).match(9, t.pos)
        t.lit(hi[b::7])
        t.fill_to(t.pos + 300)
        m.fixed(t.take(), final=b == 5)
    return m.finish()


def m_reach():
    m = Member("reach", "distances REACH-1, REACH, REACH+1 (REACH = RING - 64) and distance + length around REACH for "
               "the 1, 2, 4, 8 and 32 KiB rings, in the early, middle and tail rounds; sources that straddle the "
               "Point's window and the chunk's own output")
    t = Tok()
    t.lit(fastq_text(40, 7))

    def block(final=False):
        m.dynamic(t.take(), final=final)

    def head():
        """a block's first tokens: at a dense Point the source starts in the window, ends in the output"""
        t.lit(bytes(t.text[t.pos - RECLEN:t.pos - RECLEN + 30]))
        t.match(258, 130).match(200, 100).match(258, 31)

    def around(reaches, lengths=(3,)):
        for r in reaches:
            for n in lengths:
                for dd in (-1, 0, 1):
                    if r + dd <= t.pos:
                        t.match(n, r + dd)
                    if n > 3 and r + dd - n >= 1:
                        t.match(n, r + dd - n)                   # distance + length = REACH-1, REACH, REACH+1
            t.match(RECLEN, RECLEN * 2)

    block()
    # early (positions < 32768 of a whole-member chunk); the 32 KiB ring's three fit at 32705..32767
    t.fill_to(8300)
    block()
    head()
    around(REACHES[:4], (3, 258, 64))
    block()
    for stop in (16000, 24000, 32705):
        head()
        t.fill_to(stop)
        block()
    assert t.pos == 32705
    t.match(3, 32705).match(3, 32704).match(3, 32703)
    t.fill_to(32768 + 40)
    block()
    # middle
    head()
    around(REACHES, (3, 258, 64))
    block()
    head()
    t.fill_to(45000)
    block()
    # tail: the member's last 322 bytes
    head()
    t.fill_to(45800)
    for r in REACHES:
        for dd in (-1, 0, 1):
            t.match(4, r + dd)
    t.match(20, REACHES[0] - 20).match(20, REACHES[4] - 20)
    m.dynamic(t.take(), final=True)
    return m.finish()


def m_len258():
    m = Member("len258", "length 258 at every distance 1..65, runs of 258-byte matches (the carried rounds) across "
               "every flush UNIT boundary and across position 32768, distance 32768 exactly, and a block that "
               "starts with a match at distance 32768 (chunk position 0 takes dict[0])")
    t = Tok()
    rec = fastq_text(400, 11)
    t.lit(rec[:2048])
    m.dynamic(t.take())
    for d in range(1, 66):
        t.match(258, d)
        t.lit(rec[2048 + 64 * d:2048 + 64 * d + 64])
        if d % 16 == 0:
            m.dynamic(t.take())
    m.fixed(t.take())
    while t.pos < 32768 + 300:
        for d in (RECLEN, 322, 5 * RECLEN, 960, 1, 4032):
            t.match(258, d).match(258, d).match(258, d)
        t.lit(rec[:RECLEN])
        m.dynamic(t.take(), ll_req={285: 1})
    t.match(258, 32768).match(258, 32768).lit(rec[:RECLEN]).match(258, 32768 - 258)
    m.dynamic(t.take())
    for k in range(4):
        t.match(258, 32768).match(3, 32768).lit(rec[64:192])     # block starts: (258, 32768) at chunk position 0
        while t.pos % 8192 > 600 or t.pos < 41000 + 6000 * k:
            t.match(258, 2 * RECLEN if k % 2 else 8128)
        t.lit(rec[192:256])
        (m.fixed if k % 2 else m.dynamic)(t.take())
    t.match(258, 32768).lit(rec[:RECLEN]).match(258, 1).match(258, 65)
    m.fixed(t.take(), final=True)
    return m.finish()


def m_headers():
    m = Member("headers", "legal headers zlib never writes: one 1-bit distance code, no distance code, HLIT 257 / "
               "HDIST 1, HLIT 286 / HDIST 30, HCLEN 5 and 19, repeat codes 16/17/18 across the litlen->distance "
               "boundary, blocks of only end-of-block (fixed, dynamic, stored), hundreds of empty blocks in a row")
    rec = fastq_text(200, 13)
    t = Tok()
    # b0 one distance code of one bit (symbol 10, 4 extra bits), HCLEN 19 (CL_DEFAULT gives every symbol a code)
    t.lit(rec[:320]).match(100, 40).match(30, 33).match(64, 48)
    m.dynamic(t.take())
    # b1 no distance code at all, HLIT 257 / HDIST 1
    t.lit(rec[320:640])
    m.dynamic(t.take(), hlit=257, hdist=1)
    # b2 HLIT 286 / HDIST 30, every symbol coded: 226 x 8 + 60 x 9 bits, 2 x 4 + 28 x 5 bits
    t.lit(rec[640:960]).match(258, 640).match(227, 900, 284).match(3, 1).match(4, 960)
    m.dynamic(t.take(), [8] * 226 + [9] * 60, [4] * 2 + [5] * 28, cl_seq=rle_cl)
    # b3 HCLEN 5 (16 17 18 0 8): only lengths 0 and 8 can be coded -- 256 litlen codes of 8 bits, no distances
    t.lit(rec[960:1280])
    m.dynamic(t.take(), [0] + [8] * 256, [0], cl_lens=[1, 0, 0, 0, 0, 0, 0, 0, 2] + [0] * 7 + [3, 4, 4], cl_seq=rle_cl)
    # b4 a 16 run crossing the boundary: ... 5 5 5 | 5 5 5 5 1 2 3
    t.lit(rec[1280:1600]).match(3, 5).match(4, 6).match(5, 7)
    t2 = t.take()
    ll = complete({257: 5, 258: 5, 259: 5}, 260, used_symbols(t2)[0], fillers=list(range(1, 10)))
    m.dynamic(t2, ll, [5, 5, 5, 5, 1, 2, 3], cl_seq=rle_cl, hlit=260)
    # b5 an 18 run crossing it: litlen 257..285 zero (HLIT 286), then ten zero distance lengths
    t.lit(rec[1600:1920])
    t2 = t.take()
    ll = complete({}, 257, used_symbols(t2)[0], fillers=list(range(1, 10)))
    m.dynamic(t2, ll, [0] * 10 + [1], cl_seq=rle_cl, hlit=286)
    # b6 a 17 run crossing it: two zero litlen lengths, four zero distance lengths
    t.lit(rec[1920:2240]).match(12, 5)
    t2 = t.take()
    ll = complete({}, 266, used_symbols(t2)[0], fillers=list(range(1, 10)))
    m.dynamic(t2, ll, [0, 0, 0, 0, 1], cl_seq=rle_cl, hlit=268)
    # blocks that hold only end-of-block, then hundreds of empty blocks in a row
    m.fixed([])
    m.dynamic([], [0] * 256 + [1], [0])                          # one litlen code of one bit: legal
    m.stored(b"", pad=0x7F)
    for i in range(300):
        m.fixed([])
    t.lit(rec[2240:2560])
    m.fixed(t.take())
    for i in range(300):
        m.stored(b"", pad=0xFF) if i % 3 else m.fixed([])
    for i in range(40):
        m.dynamic([], [0] * 256 + [1], [0])
    t.lit(rec[2560:3200]).match(258, 3200)
    m.dynamic(t.take(), final=True)
    return m.finish()


def m_stored():
    m = Member("stored", "stored blocks of 0, 1 and 65535 bytes starting at every bit alignment 0..7, padding bits "
               "all ones (inflate must skip them unread)")
    rec = fastq_text(1024, 17)                                   # 65,536 bytes
    m.stored(rec[:RECLEN * 4])
    m.aligns = []
    for a in range(8):
        for size in (0, 65535, 1):
            while m.w.pos % 8 != a:                              # 23-bit (odd) and 10-bit blocks move the alignment
                if (m.w.pos - a) % 2:
                    m.fixed([(11, RECLEN)])
                else:
                    m.fixed([])
            m.aligns.append((m.w.pos % 8, size))
            data = rec[:size] if size != 1 else b"@"
            m.stored(data, pad=0xFF)
    m.fixed([(11, RECLEN)], final=True)
    return m.finish()


@functools.lru_cache(None)
def valid_members():
    """name -> Member (gz, text, deflate, fields, tokens, doc), built once per process"""
    ms = [f() for f in (m_long_codes, m_root_edges, m_fixed_hi, m_reach, m_len258, m_headers, m_stored)]
    return {m.name: m for m in ms}


# ---------------------------------------------------------------------------------- invalid cases
# cl code of the error twins: 16, 17, 18 and 0..9 are 4-bit codes, 10..15 5-bit ones, so that any of
# the short lengths can be patched into a repeat code (and back) without moving a bit
Case = collections.namedtuple("Case", "name rule clean bad")

_A = fastq_text(6, 31)
_B = fastq_text(6, 32)
_C = fastq_text(6, 33)


def _twin(kind):
    """block A (fixed) | block B (the kind under test) | block C (fixed, final): at chunk size 9 each
    is one chunk, so the patched block B is chunk 1 of a three-chunk member"""
    m = Member("err_" + kind, "")
    # A ends 6 bits into a byte, so that chunk 0's slice (which ends with that byte) holds fewer than
    # the 3 header bits of block B: zlib, run on chunk 0 alone, cannot see B's block type
    t = Tok().lit(_A).match(3, 1)
    m.fixed(t.take())
    assert m.w.pos % 8 == 6
    if kind == "fixed":
        t.lit(_B[:200]).match(258, 200).match(20, 64).lit(_B[200:])
        m.fixed(t.take())
    elif kind == "stored":
        m.stored(_B, pad=0x15)
    elif kind == "dynamic":
        t.lit(_B[:200]).match(12, 64).match(9, 96).lit(_B[200:])
        toks = t.take()
        ll, d = used_symbols(toks)
        ll_lens = complete({}, 286, ll, fillers=list(range(1, 10)))[:266]
        m.dynamic(toks, ll_lens, [1, 2] + [0] * 9 + [3, 3], cl_seq=rle_cl, hdist=17)   # ends in a 17 run of 4
    elif kind == "onedist":
        t.lit(_B[:200]).match(40, 64).match(9, 64).lit(_B[200:])
        m.dynamic(t.take())
    elif kind == "onlyeob":
        m.dynamic([], [0] * 256 + [1], [0])
        m.fixed([_B])
    m.fixed([_C], final=True)
    return m.finish()


@functools.lru_cache(None)
def invalid_cases():
    """[Case(name, zlib's message for the rule, clean twin Member, bad gz)]: each bad member is its
    clean twin with one named field overwritten in place (same bit length)"""
    out = []

    def add(name, rule, m, field, value):
        out.append(Case(name, rule, m, patch_bits(m.gz, m.field(field), value)))

    fx, st, dy, od, oe = (_twin(k) for k in ("fixed", "stored", "dynamic", "onedist", "onlyeob"))
    blk = inspect(dy.deflate)[1][1]
    seq, hlit = blk.cl_syms, blk.hlit
    cc, fl = canonical(CL_DEFAULT), canonical(FIXED_LL)
    add("block_type_3", "invalid block type", fx, "b1.btype", 3)
    add("stored_nlen", "invalid stored block lengths", st, "b1.nlen", 0x1234)
    add("stored_len", "invalid stored block lengths", st, "b1.len", len(_B) + 1)
    add("hlit_287", "too many length or distance symbols", dy, "b1.hlit", 30)
    add("hlit_288", "too many length or distance symbols", dy, "b1.hlit", 31)
    add("hdist_31", "too many length or distance symbols", dy, "b1.hdist", 30)
    add("hdist_32", "too many length or distance symbols", dy, "b1.hdist", 31)
    add("hclen_4", "", dy, "b1.hclen", 0)            # only 16 17 18 0 get a code: no block can be valid
    assert cc[seq[0]][1] == 4
    add("code16_first", "invalid bit length repeat", dy, "b1.seq0", cc[16][0])
    assert seq[-1] == 17                            # the four zero lengths that end the distance alphabet
    add("repeat_overrun", "invalid bit length repeat", dy, "b1.seq%d.extra" % (len(seq) - 1), 7)
    add("cl_oversubscribed", "invalid code lengths set", dy, "b1.cl0", 1)
    add("cl_incomplete", "invalid code lengths set", dy, "b1.cl0", 5)
    lit = "b1.lens%d" % ord("@")                     # a literal's length, written as a plain symbol
    add("litlen_oversubscribed", "invalid literal/lengths set", dy, lit, cc[1][0])
    add("litlen_incomplete", "invalid literal/lengths set", dy, lit, cc[9][0])
    add("no_end_of_block", "invalid code -- missing end-of-block", dy, "b1.lens256", cc[0][0])
    add("dist_oversubscribed", "invalid distances set", dy, "b1.lens%d" % (hlit + 11), cc[1][0])
    add("dist_incomplete", "invalid distances set", dy, "b1.lens%d" % (hlit + 11), cc[4][0])
    ntok = len(_B[:200])                             # the (258, 200) match of the fixed twin
    add("litlen_symbol_286", "invalid literal/length code", fx, "b1.tok%d" % ntok, fl[286][0])
    add("litlen_symbol_287", "invalid literal/length code", fx, "b1.tok%d" % ntok, fl[287][0])
    add("dist_symbol_30", "invalid distance code", fx, "b1.tok%d.dist" % ntok, 30)
    add("dist_symbol_31", "invalid distance code", fx, "b1.tok%d.dist" % ntok, 31)
    add("unused_dist_code", "invalid distance code", od, "b1.tok%d.dist" % ntok, 1)
    add("unused_litlen_code", "invalid literal/length code", oe, "b1.eob", 1)
    return tuple(out)


def type3_peek_case():
    """(clean Member, bad gz): block type 3 in a block whose three header bits still lie in the last
    byte of the chunk before it.  zlib, still inside the inflate() call that wrote that chunk's last
    byte, reads them: the chunk BEFORE the bad block fails as well."""
    m = Member("err_type3_peek", "")
    m.fixed([_A])
    assert m.w.pos % 8 == 2                          # six bits of this byte are left for block B
    m.fixed([_B])
    m.fixed([_C], final=True)
    m.finish()
    return m, patch_bits(m.gz, m.field("b1.btype"), 3)


def far_start_member(at=1):
    """(gz, text): the token at output position `at` (< 32768) reaches two bytes before output
    position 0.  CreateIndex has no history there (zlib: "invalid distance too far back"); the trailer
    is written for the text an all-zero history would give, so the CRC is not what rejects the member."""
    zeros = bytes(32768)
    rec = fastq_text(600, 41)
    t = Tok(zeros)
    t.lit(rec[:at]).match(3, at + 2).lit(rec[at:])
    toks = t.take()
    w = BitWriter()
    cut = next(i for i, x in enumerate(toks) if isinstance(x, tuple))
    fixed_block(w, toks[:cut])                       # the offending token opens the second block
    fixed_block(w, toks[cut:], final=True)
    text = apply(toks, zeros)
    return gzip_wrap(w.getvalue(), text), text
