"""What the pair chunk tests share (tests/test_pair_chunks.py, tests/test_gpu_pair_emission_stages.py): the mate
files, the per-file oracle of their records (oracle.c's Extract + Parse over zlib, the records the reference
parses twice -- SURVEY Q1 -- dropped) and the comparison of an emitted window with it."""
import ctypes as C
import zlib

import numpy as np

import parallelparsing_amd as pp
from oracle import oracle as O


def mate_gz(mate, nrec, seed, flush_every=0):
    """A mate file of the Generator shape; flush_every > 0 ends a deflate block after every that
    many records (full flush), so Points fall on record starts and Q1 duplicates appear."""
    S = pp.synth()
    sz = S.ppg_synth_fastq_size_mate(0, nrec, 150, mate)
    txt = np.zeros(sz, np.uint8)
    S.ppg_synth_fastq_mate(seed, mate, 0, nrec, 150, C.c_void_p(txt.ctypes.data), sz, 8)
    if not flush_every:
        gzb = np.zeros(sz, np.uint8)
        L = S.ppg_synth_gzip(C.c_void_p(txt.ctypes.data), sz, 6, 1 << 20, 8, C.c_void_p(gzb.ctypes.data), gzb.size)
        return gzb[:L].tobytes()
    lines = txt.tobytes().split(b"\n")
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = []
    for g in range(0, nrec, flush_every):
        out.append(co.compress(b"\n".join(lines[4 * g:4 * min(nrec, g + flush_every)]) + b"\n"))
        out.append(co.flush(zlib.Z_FULL_FLUSH))
    out.append(co.flush())
    return b"".join(out)


def oracle_records(gz, chunk):
    """The file's records as the reference parses them chunk by chunk (oracle: Core.cs:133-192 +
    Parsing.cs:11-69 over zlib), each record's bytes raw[start, n4] -- minus the Q1 duplicates
    (a chunk's first record lying wholly inside its Point's offset)."""
    oi = O.build_index(gz, chunk)
    recs, dups = [], 0
    for k in range(oi.count - 1):
        off = oi.point(k)[4]
        raw = off + O.extract(gz, oi, k)
        start = 0
        for j, (n1, n2, n3, n4) in enumerate(O.parse(off, raw[len(off):]).tolist()):
            if j == 0 and n4 < len(off):
                dups += 1
            else:
                recs.append(raw[start:n4 + 1])
            start = n4 + 1
    return recs, dups


def expected_half(recs, lo, hi):
    b = b"".join(recs[lo:hi])
    nl = np.nonzero(np.frombuffer(b, np.uint8) == 10)[0].astype(np.uint32)
    return b, nl.reshape(-1, 4) if nl.size else np.zeros((0, 4), np.uint32)


def check_window(pr, j0, j1, K, recs, nrec, seen):
    for j in range(j0, j1):
        lo, hi = j * K, min((j + 1) * K, nrec)
        for f in (0, 1):
            b, d = pr.copy_chunk(j, f)
            eb, ed = expected_half(recs[f][0], lo, hi)
            assert b.tobytes() == eb, (j, f)
            assert np.array_equal(d, ed), (j, f)
            # and the record reader over the half gives the oracle's records
            if j == j0:
                r = pp.records_from_descriptors(b.tobytes(), d)
                assert r[0].identifier == recs[f][0][lo][1:recs[f][0][lo].index(b"\n")]
        assert j not in seen
        seen.add(j)
