"""Reference for the record selection (include/ppgpu.h "record selection"), restated from the
semantics with bytes and numpy, not from the kernels; plus the forged input and the masks the
selection tests share.

select_reference(chunks, hit) takes, per chunk k, the oracle's (offset_k, raw_k, descriptors) as
seqpack_ref.oracle_chunks / seqquery_ref.chunks_of give them, and one bool per record:

  T_j = raw_k[a_j : e_j], a_j = 0 for a chunk's first record and the previous record's n4 + 1
  otherwise, e_j = n4 + 1; the selected T_j back to back, their offsets, their descriptors minus a_j
  and their record numbers."""
import functools
import random
import zlib

import numpy as np

import seqpack_ref as R
import seqquery_ref as Q

FORGED = "forged_select"          # the forged input's name beside the seqpack_ref inputs
FORGED_CHUNK = 10
TINY = "forged_tiny"              # ... and the input of very short records
TINY_CHUNK = 300
TINY_RECORDS = 12000
LONG = "forged_long"              # ... and the input with records longer than the copy kernel's span
LONG_CHUNK = 5000
SPAN = 16384                      # destination bytes per block of ppg_sel_copy (kSelSpan, csrc/ppg_device.h)
FORGED_SEED = 5
MASK_SEED = 11
MASKS = ("all", "none", "alternate", "chunk_first", "chunk_last", "half", "sparse")
# selecting every record and concatenating gives the decompressed text exactly (no duplicates, no
# malformed text: stored_c50, malformed_c40, plusline_c50 and nul_c60 are left out)
WHOLE_TEXT = ("l6_c200", "l6_c20", "l1_c150", "l9_c300", "fixed_c100", "huffonly_c20", "rle_c100", "memlevel1_c10",
              "pigz_c100", "one_record", "short_reads_c30", "long_reads_c10", "crlf_c100")


def record_spans(chunks):
    """Per record of all chunks, in order: (chunk, a_j, e_j)."""
    out = []
    for k, (_, _, desc) in enumerate(chunks):
        a = 0
        for n4 in np.asarray(desc, np.int64).reshape(-1, 4)[:, 3].tolist():
            assert n4 + 1 >= a, "a record ends before it starts"
            out.append((k, a, n4 + 1))
            a = n4 + 1
    return out


def select_reference(chunks, hit):
    """{recno int64[S], sel_off int64[S+1], desc uint32[S,4], bytes uint8[nbytes], records, nbytes} of the
    records j with hit[j] (entries at and past the record count are ignored)."""
    spans = record_spans(chunks)
    hit = np.asarray(hit, bool)
    raws = [bytes(c[1]) for c in chunks]
    descs = np.concatenate([np.asarray(c[2], np.int64).reshape(-1, 4) for c in chunks]) if chunks else np.zeros((0, 4), np.int64)
    recno = [j for j in range(len(spans)) if j < hit.size and hit[j]]
    parts = [raws[spans[j][0]][spans[j][1]:spans[j][2]] for j in recno]
    sel_off = np.zeros(len(recno) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=sel_off[1:])
    desc = np.array([descs[j] - spans[j][1] for j in recno], np.int64).reshape(-1, 4)
    assert (desc >= 0).all()
    return {"recno": np.array(recno, np.int64), "sel_off": sel_off, "desc": desc.astype(np.uint32),
            "bytes": np.frombuffer(b"".join(parts), np.uint8), "records": len(recno), "nbytes": int(sel_off[-1])}


# ---- the forged input: what the copy kernel's word mapping can get wrong ----
def forged_records(seed=FORGED_SEED):
    """Records (bytes, each through its quality line's newline) whose byte lengths cover every residue
    mod 16: 6..15 bytes (an empty identifier, sequence and quality is "@\\n\\n+\\n\\n": several fit one
    16-byte word), 100..400 bytes, and a few longer than 8 KiB; shuffled with a fixed seed."""
    rng = random.Random(seed)
    lengths = [6 + r for r in range(10)] * 10                    # 6 .. 15 bytes, ten of each
    lengths += [100 + 19 * i for i in range(16)]                 # 100 .. 385: 19 is odd, every residue mod 16
    lengths += [rng.randrange(100, 401) for _ in range(120)]
    lengths += [8193 + 16 * 3 + 5, 9001, 12345 + 1, 8200]
    recs = []
    for n, T in enumerate(lengths):
        L = rng.randrange(0, (T - 6) // 2 + 1) if T < 16 else (T - 6) // 2 - rng.randrange(0, 8)
        ident = (b"%d_" % n * 16)[:T - 6 - 2 * L]
        seq = bytes(rng.choice(b"ACGTN") for _ in range(L))
        rec = b"@%s\n%s\n+\n%s\n" % (ident, seq, b"I" * L)
        assert len(rec) == T
        recs.append(rec)
    rng.shuffle(recs)
    return recs


@functools.lru_cache(maxsize=None)
def forged_gz(seed=FORGED_SEED):
    """The forged text as one gzip member at memLevel 1 (the recipe of seqquery_ref.forged_gz: a Point,
    and for most chunks an offset carry, every few records)."""
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
    return co.compress(b"".join(forged_records(seed))) + co.flush()


@functools.lru_cache(maxsize=None)
def tiny_gz():
    """12,000 records of 6 to 15 bytes: more than 512 of them (the records the copy kernel stages at a
    time) fall into one 16 KiB destination span, a chunk of 300 holds more than one 256-record tile,
    and 64 KiB of this text hold more records than a cursor slot is sized for at open (one per 64 B
    of text + 4,096)."""
    rng = random.Random(FORGED_SEED + 1)
    recs = []
    for n in range(TINY_RECORDS):
        L = rng.randrange(0, 3)
        ident = (b"%d" % n)[-rng.randrange(0, 4):] if rng.random() < 0.8 else b""
        recs.append(b"@%s\n%s\n+\n%s\n" % (ident, bytes(rng.choice(b"ACGT") for _ in range(L)), b"I" * L))
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
    return co.compress(b"".join(recs)) + co.flush()


def long_records(seed=FORGED_SEED + 2):
    """Records of 18,000 to 70,000 bytes among records of 100 to 400 and of 6 to 15 bytes: longer than
    one and than two destination spans, so that a record covers several multiples of the span and whole
    spans lie inside one record.  CreateIndex refuses 32 KiB of text without an '@' (SURVEY Q4), so the
    long sequences and qualities carry one every 8,000 bytes; the chunk size keeps the whole text one
    chunk, so that no Point falls on such an '@' and cuts a record in two."""
    rng = random.Random(seed)
    recs = []
    for n, T in enumerate([20000, 250, 40001, 9, 70000, 131, 33000, 50001, 14, 18000, 36001, 377, 65537, 6, 48000]):
        L = (T - 6) // 2 - (rng.randrange(0, 8) if T >= 100 else 0)
        ident = (b"%d_" % n * 16)[:T - 6 - 2 * L]
        seq = bytearray(rng.choice(b"ACGTN") for _ in range(L))
        qual = bytearray(b"I" * L)
        for i in range(7999, L, 8000):
            seq[i] = qual[i] = ord("@")
        rec = b"@%s\n%s\n+\n%s\n" % (ident, bytes(seq), bytes(qual))
        assert len(rec) == T
        recs.append(rec)
    return recs


@functools.lru_cache(maxsize=None)
def long_gz():
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    return co.compress(b"".join(long_records())) + co.flush()


def load_input(name):
    """(gz bytes, chunksize) of a forged input or a seqpack_ref input."""
    forged = {FORGED: (forged_gz, FORGED_CHUNK), TINY: (tiny_gz, TINY_CHUNK), LONG: (long_gz, LONG_CHUNK)}
    if name in forged:
        return forged[name][0](), forged[name][1]
    return R.load_input(name)


@functools.lru_cache(maxsize=None)
def chunks(name):
    return Q.chunks_of(*load_input(name)) if name in (FORGED, TINY, LONG) else R.oracle_chunks(name)


# ---- the masks the tests share ----
@functools.lru_cache(maxsize=None)
def mask_bool(name, which):
    """One bool per record of input `name` (read-only)."""
    ch = chunks(name)
    per = [len(c[2]) for c in ch]
    n = sum(per)
    rng = np.random.default_rng(MASK_SEED)
    first = np.cumsum([0] + per[:-1])
    hit = np.zeros(n, bool)
    if which == "all":
        hit[:] = True
    elif which == "alternate":
        hit[::2] = True
    elif which == "chunk_first":
        hit[[f for f, m in zip(first, per) if m]] = True
    elif which == "chunk_last":
        hit[[f + m - 1 for f, m in zip(first, per) if m]] = True
    elif which == "half":
        hit = rng.random(n) < 0.5
    elif which == "sparse":
        hit = rng.random(n) < 0.02
    else:
        assert which == "none", which
    hit.setflags(write=False)
    return hit


def mask_words(hit, garbage_words=0):
    """The hit-mask words of a bool per record; the bits past the records are 0, or with garbage_words
    all 1 and followed by that many more all-ones words."""
    hit = np.asarray(hit, bool)
    bits = np.zeros((hit.size + 31) // 32 * 32 + 32 * garbage_words, np.uint64)
    bits[:hit.size] = hit
    if garbage_words:
        bits[hit.size:] = 1
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """The reference selection of input `name` under the shared mask `which`; shared and read-only."""
    ref = select_reference(chunks(name), mask_bool(name, which))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def pattern_reference(name, pattern):
    """The reference selection of the records of input `name` whose Sequence contains `pattern`."""
    ch = chunks(name)
    ref = select_reference(ch, Q.query_reference(ch, pattern)["hit"])
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
