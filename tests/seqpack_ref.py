"""Reference for the packed-read format (include/ppgpu.h "packed reads"), restated in numpy from
the format's definition, not from the kernel; plus the inputs the packed-read tests share.

pack_reference(raws, descs) takes, per chunk k, the oracle's raw_k = offset_k + extract(k) and its
O.parse(offset_k, chunk_k) table; everything a test expects comes from it."""
import ctypes as C
import functools
import zlib

import numpy as np

from conftest import CASES, load_case
from oracle import oracle as O

SYNTH = "synth_illumina"          # the synthetic input's name among the cases
SYNTH_CHUNK = 200
ALL_INPUTS = list(CASES) + [SYNTH]

_ACGT = np.zeros(256, bool)
_ACGT[list(b"ACGT")] = True
_CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def pack_reference(raws, descs, quality=True):
    """{seq_off int64[n+1], seq_len uint32[n], bases uint32[T/16], mask uint32[T/32], qual uint8[T] or None}
    over the records of all chunks, in order."""
    lens = []
    for d in descs:
        d = np.asarray(d, np.int64).reshape(-1, 4)
        lens.append(d[:, 1] - d[:, 0] - 1)
    L = np.concatenate(lens) if lens else np.zeros(0, np.int64)
    assert (L >= 0).all()
    P = (L + 31) // 32 * 32
    seq_off = np.zeros(L.size + 1, np.int64)
    np.cumsum(P, out=seq_off[1:])
    T = int(seq_off[-1])
    code = np.zeros(T, np.uint8)      # one entry per base position, folded into words below
    mbit = np.zeros(T, np.uint8)
    qual = np.zeros(T, np.uint8)
    j = 0
    for raw, d in zip(raws, descs):
        r = np.frombuffer(bytes(raw), np.uint8)
        for n1, n2, n3, n4 in np.asarray(d, np.int64).reshape(-1, 4):
            b, ln = int(seq_off[j]), int(n2 - n1 - 1)
            c = r[n1 + 1:n2]
            code[b:b + ln] = np.where(_ACGT[c], _CODE[c], 0)
            mbit[b:b + ln] = ~_ACGT[c]
            q = r[n3 + 1:max(n4, n3 + 1)][:ln]     # raw[n3+1+i] while n3+1+i < n4, i < L
            qual[b:b + q.size] = q
            j += 1
    sh2 = (2 * np.arange(16, dtype=np.uint64))
    bases = (code.reshape(-1, 16).astype(np.uint64) << sh2).sum(axis=1).astype(np.uint32)
    sh1 = np.arange(32, dtype=np.uint64)
    mask = (mbit.reshape(-1, 32).astype(np.uint64) << sh1).sum(axis=1).astype(np.uint32)
    return {"seq_off": seq_off, "seq_len": L.astype(np.uint32), "bases": bases, "mask": mask,
            "qual": qual if quality else None}


@functools.lru_cache(maxsize=None)
def synth_gz():
    """ppg_synth_illumina(seed 7, records 0..3000) as one gzip member (level 6, memLevel 8)."""
    import parallelparsing_amd as pp
    S = pp.synth()
    sz = S.ppg_synth_illumina_size(7, 0, 3000)
    txt = np.zeros(sz, np.uint8)
    assert S.ppg_synth_illumina(7, 0, 3000, C.c_void_p(txt.ctypes.data), sz, 4) == sz
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    return co.compress(txt.tobytes()) + co.flush()


def load_input(name):
    """(gz bytes, chunksize) of a golden case or the synthetic input."""
    if name == SYNTH:
        return synth_gz(), SYNTH_CHUNK
    meta, gz = load_case(name)
    return gz, meta["chunksize"]


@functools.lru_cache(maxsize=None)
def oracle_chunks(name):
    """Per chunk of the input, from the oracle: (offset_k, raw_k, descriptors (n, 4))."""
    gz, cs = load_input(name)
    oi = O.build_index(gz, cs)
    out = []
    for k in range(oi.count - 1):
        off = oi.point(k)[4]
        ch = O.extract(gz, oi, k)
        out.append((off, off + ch, np.asarray(O.parse(off, ch), np.uint32).reshape(-1, 4)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference pack of the whole input (all chunks, with qualities); shared and read-only."""
    ch = oracle_chunks(name)
    ref = pack_reference([c[1] for c in ch], [c[2] for c in ch])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def reference_of_chunks(name, k0, k1):
    """The reference pack of chunks [k0, k1) alone (offsets from 0): a cursor batch."""
    ch = oracle_chunks(name)[k0:k1]
    return pack_reference([c[1] for c in ch], [c[2] for c in ch])
