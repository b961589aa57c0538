"""Sequence queries against pulling the records to the host, measured in one process on the GPU box
(one pass; run it under a time limit), on the member tools/seqpack_probe.py uses: a ~1 GiB synthetic
FASTQ member (ppg_synth_fastq, 150 bp, written to $TMPDIR with its index).

  answers   BatchedFASTQ.CountPattern("GTTATACACTGC") and CountBases(): a shard with a bounded
            out_capacity and the query hook per batch; wall clock, once from the file (read and upload
            included) and with the compressed bytes resident from the query before
  cursors   full enumeration through the text cursor and the packed cursor without qualities (what a
            host consumer needs before it can search or count at all; the host-side search itself is
            not timed), alternating with the answers, warm-ups first, the median of the runs
  kernels   layout, offsets, query and reduction on a resident one-batch shard (hipEvents), for the
            census alone and for patterns of 12 and 64 bytes

  python tools/seqquery_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--out profiles/seqquery_probe.json]

Writes records/s and kernel ms, with ppg_build_id, as JSON."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = b"GTTATACACTGC"      # Benchmark/Naive.cs RunPattern


def enumerate_once(pp, ix, path, dev, batch_bytes, threads, packed):
    cur = pp.Cursor(ix, path, batch_bytes=batch_bytes, threads=threads, device=dev, packed=packed, quality=False)
    nrec = 0
    t1 = time.perf_counter()
    for b in cur:
        nrec += b.nrecords
    sec = time.perf_counter() - t1
    cur.close()
    return nrec, sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqquery_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("seqquery_probe: no GPU (nothing is measured without one)")
    seg = 262_144                                    # records per segment: ~100 MB of 150 bp text
    repeats = max(1, round(a.gib * (1 << 30) / (seg * 385)))
    tf = TiledFile(seg, repeats, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_seqquery_{os.getpid()}.fastq.gz")
    try:
        with open(path, "wb") as f:
            for lo in range(0, tf.file_len, 1 << 30):
                f.write(tf.file_bytes(lo, min(tf.file_len, lo + (1 << 30))))
        ix = tf.index(0, tf.npoints)
        dev = pp.Device(0)
        bb = a.batch_mib << 20
        nrec = tf.expected_records()
        # what the answers must be: the segment's text searched on the host, times its repeats
        # (every segment of the member is the same text; exact when no Point falls on a record start:
        # such a record is parsed, and counted, twice)
        seqs = tf.text.tobytes().split(b"\n")[1::4]
        want_hits = sum(PATTERN in s_ for s_ in seqs) * repeats
        want_a = sum(s_.count(b"A") for s_ in seqs) * repeats
        exact = nrec == seg * repeats
        fq = pp.BatchedFASTQ(ix, path, device=dev)
        fq.query_out_capacity = bb

        def count_pattern(cold):
            if cold:
                fq.Dispose()       # the next query reads and uploads the file again
            t0 = time.perf_counter()
            hits = fq.CountPattern(PATTERN)
            return hits, time.perf_counter() - t0

        def count_bases():
            t0 = time.perf_counter()
            n_a = fq.CountBases()["A"]
            return n_a, time.perf_counter() - t0

        # count_pattern_from_file: file -> answer; count_pattern / count_bases: the compressed file
        # resident from the query before, decode + query per batch
        modes = {"count_pattern_from_file": lambda: count_pattern(True), "count_pattern": lambda: count_pattern(False),
                 "count_bases": count_bases,
                 "text_cursor": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, False),
                 "packed_cursor_noqual": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, True)}
        expect = {"count_pattern_from_file": want_hits, "count_pattern": want_hits, "count_bases": want_a,
                  "text_cursor": nrec, "packed_cursor_noqual": nrec}
        runs = {k: [] for k in modes}
        for r in range(a.warmups + a.runs):          # alternating
            for name, fn in modes.items():
                got, sec = fn()
                assert got == expect[name] or (not exact and got > expect[name]), (name, got, expect[name])
                if r >= a.warmups:
                    runs[name].append(sec)
        out = {"build_id": _lib.lib.ppg_build_id().decode(), "text_GiB": int(tf.text.size) * repeats / (1 << 30),
               "gz_GB": tf.file_len / 1e9, "records": nrec, "chunk_records": a.chunk, "chunks": tf.npoints - 1,
               "batch_MiB": a.batch_mib, "threads": a.threads, "warmups": a.warmups, "runs": a.runs,
               "pattern": PATTERN.decode(), "hits_host_search": want_hits, "count_A_host_search": want_a,
               "host_search_exact": exact, "wall_clock": {}}
        for name, secs in runs.items():
            sec = statistics.median(secs)
            out["wall_clock"][name] = {"records_per_s": nrec / sec, "seconds_median": sec, "seconds_all": secs}
        # kernels on a resident one-batch shard of the same member
        n = tf.npoints - 1
        _, i0, _, _ = ix.point_fields(0)
        _, i1, _, _ = ix.point_fields(n)
        with open(path, "rb") as f:
            f.seek(i0 - 1)
            comp = np.frombuffer(f.read(i1 - i0 + 1), np.uint8)
        sh = pp.Shard(ix, comp, 0, n, device=dev).run()
        fn = _lib.lib.ppgx_seqquery_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int, C.POINTER(C.c_float)]
        out["kernels"] = {}
        for key, pat in (("census_only", b""), ("pattern_12", PATTERN), ("pattern_64", (PATTERN * 6)[:64])):
            ms = (C.c_float * 4)()
            pp.check(fn(sh.handle, pat, len(pat), 9, ms), "ppgx_seqquery_times")
            q = sh.query_sequences(pat)
            out["kernels"][key] = {"layout_ms": ms[0], "offsets_ms": ms[1], "query_ms": ms[2], "reduce_ms": ms[3],
                                   "records": q.records, "bases": q.bases, "hits": q.hits,
                                   "records_per_s_query_kernel": q.records / ms[2] * 1e3,
                                   "sequence_GBps_query_kernel": q.bases / ms[2] / 1e6}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
    finally:
        if os.path.exists(path):
            os.remove(path)


if __name__ == "__main__":
    main()
