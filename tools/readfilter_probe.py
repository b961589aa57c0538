"""Read filters against the query and against moving every record's text, measured in one process on the
GPU box (one pass; run it under a time limit), on the member the seqpack, seqquery and seqselect probes
use: a ~1 GiB synthetic FASTQ member (ppg_synth_fastq, 150 bp, written to $TMPDIR with its index).

  kernels   layout, measure and decide on a resident one-batch shard (hipEvents, the median of 9), without
            criteria and with all four, each with and without the metrics plane (the mask is always
            written), and with both forms of the Quality histogram (one LDS add per run of equal bytes of
            a lane, one per byte); ppg_seq_query, census alone and with a 12-byte pattern, is timed in the
            same process as the yardstick
  cursors   from the file, alternating, warm-ups first, the median of the runs: CountPassing with the file
            read and uploaded again (decode + filter, no text to the host), Where(filter=...) with a filter
            that passes about a tenth of the records (a mean-quality bound at the 90th percentile of the
            file's own per-record means) and with one that passes all, the text cursor, and Where(pattern);
            records/s and the bytes each copies to the host

  python tools/readfilter_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--out profiles/readfilter_probe.json]

Writes kernel ms, records/s and bytes, with ppg_build_id, as JSON."""
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


def enumerate_once(pp, ix, path, dev, batch_bytes, threads, pattern, flt):
    """(records scanned, records handed to the host, bytes copied to the host, seconds)."""
    cur = pp.Cursor(ix, path, batch_bytes=batch_bytes, threads=threads, device=dev, pattern=pattern, filter=flt)
    scanned = got = nbytes = 0
    t1 = time.perf_counter()
    for b in cur:
        scanned += b.nrecords
        if pattern is None and flt is None:
            got += b.nrecords
            nbytes += int(b.raw_off[-1]) + 16 * b.nrecords
        else:
            s = b.selected
            got += s.records
            nbytes += s.nbytes + 32 * s.records + 8        # text, descriptors, recno, sel_off
    sec = time.perf_counter() - t1
    cur.close()
    return scanned, got, nbytes, sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readfilter_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("readfilter_probe: no GPU (nothing is measured without one)")
    seg = 262_144                                    # records per segment: ~100 MB of 150 bp text
    repeats = max(1, round(a.gib * (1 << 30) / (seg * 385)))
    tf = TiledFile(seg, repeats, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_readfilter_{os.getpid()}.fastq.gz")
    try:
        with open(path, "wb") as f:
            for lo in range(0, tf.file_len, 1 << 30):
                f.write(tf.file_bytes(lo, min(tf.file_len, lo + (1 << 30))))
        ix = tf.index(0, tf.npoints)
        dev = pp.Device(0)
        bb = a.batch_mib << 20
        nrec = tf.expected_records()
        out = {"build_id": _lib.lib.ppg_build_id().decode(), "text_GiB": int(tf.text.size) * repeats / (1 << 30),
               "gz_GB": tf.file_len / 1e9, "records": nrec, "chunk_records": a.chunk, "chunks": tf.npoints - 1,
               "batch_MiB": a.batch_mib, "threads": a.threads, "warmups": a.warmups, "runs": a.runs,
               "pattern": PATTERN.decode(), "kernels": {}, "from_file": {}}

        # ---- kernels on a resident one-batch shard ----
        n = tf.npoints - 1
        _, i0, _, _ = ix.point_fields(0)
        _, i1, _, _ = ix.point_fields(n)
        with open(path, "rb") as f:
            f.seek(i0 - 1)
            comp = np.frombuffer(f.read(i1 - i0 + 1), np.uint8)
        sh = pp.Shard(ix, comp, 0, n, device=dev).run()
        # the file's own numbers: a mean-quality bound about a tenth of the records reach
        r0 = sh.filter_reads(pp.ReadFilter(), metrics=True)
        m = r0.metrics_host()
        mean_milli = 1000 * (m["qual_sum"].astype(np.int64) - 33 * m["qual_length"].astype(np.int64)) // \
            np.maximum(m["qual_length"].astype(np.int64), 1)
        bound = int(np.percentile(mean_milli, 90)) + 1
        tenth = pp.ReadFilter(min_mean_quality=bound / 1000)
        every = pp.ReadFilter(min_length=1)
        four = pp.ReadFilter(min_length=1, max_length=100000, max_n=150, min_mean_quality=bound / 1000, low_quality=20,
                             max_low_fraction=1.0)
        top = np.argsort(r0.qual_count)[::-1][:4]
        out["file"] = {"bases": r0.bases, "other": r0.other, "qual_bytes": r0.qual_bytes,
                       "top_quality_bytes": {chr(int(v)): int(r0.qual_count[v]) for v in top},
                       "mean_quality_bound_milli": bound,
                       "passed_tenth": sh.filter_reads(tenth).passed, "passed_every": sh.filter_reads(every).passed}
        del m, mean_milli, r0
        fn = _lib.lib.ppgx_readfilter_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        for key, flt in (("criteria_0", pp.ReadFilter()), ("criteria_15", four)):
            s = flt.struct()
            assert s.criteria == (0 if key == "criteria_0" else 15)
            for metrics in (0, 1):
                for hist, hname in ((0, "hist_runs"), (1, "hist_bytes")):
                    ms = (C.c_float * 3)()
                    pp.check(fn(sh.handle, C.byref(s), 1, metrics, hist, 9, ms), "ppgx_readfilter_times")
                    out["kernels"][f"{key}_{'metrics' if metrics else 'mask_only'}_{hname}"] = {
                        "layout_ms": ms[0], "measure_ms": ms[1], "decide_ms": ms[2], "sum_ms": ms[0] + ms[1] + ms[2]}
        qn = _lib.lib.ppgx_seqquery_times
        qn.restype = C.c_int
        qn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_float)]
        for key, pat in (("seq_query_census", b""), ("seq_query_pattern12", PATTERN)):
            ms = (C.c_float * 4)()
            pp.check(qn(sh.handle, pat if pat else None, len(pat), 9, ms), "ppgx_seqquery_times")
            out["kernels"][key] = {"layout_ms": ms[0] + ms[1], "query_ms": ms[2], "reduce_ms": ms[3], "sum_ms": sum(ms)}
        del sh

        # ---- from the file ----
        fq = pp.BatchedFASTQ(ix, path, device=dev)
        fq.query_out_capacity = bb

        def count_passing():
            fq.Dispose()       # the count reads and uploads the file again
            t0 = time.perf_counter()
            count_passing.passed = fq.CountPassing(tenth).passed      # the answer: no record reaches the host
            return nrec, 0, 0, time.perf_counter() - t0

        modes = {"count_passing_from_file": count_passing,
                 "where_filter_tenth": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, None, tenth),
                 "where_filter_every": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, None, every),
                 "text_cursor": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, None, None),
                 "where_pattern": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, PATTERN, None)}
        runs = {k: [] for k in modes}
        seen = {}
        for r in range(a.warmups + a.runs):          # alternating
            for name, f_ in modes.items():
                scanned, got, nbytes, sec = f_()
                assert scanned == nrec, (name, scanned, nrec)
                seen[name] = (got, nbytes)
                if r >= a.warmups:
                    runs[name].append(sec)
        assert seen["where_filter_tenth"][0] == count_passing.passed == out["file"]["passed_tenth"], (seen, out["file"])
        assert seen["where_filter_every"][0] == seen["text_cursor"][0] == nrec, seen
        for name, secs in runs.items():
            sec = statistics.median(secs)
            out["from_file"][name] = {"records_per_s": nrec / sec, "seconds_median": sec, "seconds_all": secs,
                                      "records_to_host": seen[name][0], "bytes_to_host": seen[name][1]}
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
