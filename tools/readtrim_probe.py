"""Read trimming against the read filter, the query and against moving every record's text, measured in one
process on the GPU box (one pass; run it under a time limit), on the member the seqpack, seqquery,
seqselect and readfilter probes use: a ~1 GiB synthetic FASTQ member (ppg_synth_fastq, 150 bp, written to
$TMPDIR with its index).

  kernels   layout, measure (without and with the adapter compare) and decide on a resident one-batch
            shard (hipEvents, the median of 9), for the realistic trim below and for the quality cuts
            alone; ppg_rf_measure (the read filter: the same Sequence and Quality bytes) and
            ppg_seq_query are timed in the same process on the same batch as the yardsticks
  cursors   from the file, alternating, warm-ups first, the median of the runs: CountTrimmed with the file
            read and uploaded again (decode + trim, nothing to the host), Where(trim=...), Where(filter=...)
            with a length filter every record passes, and the text cursor; records/s and the bytes each
            copies to the host

The realistic trim: trailing quality 20, window (4, 20), the first 33 bases of the TruSeq adapter with the
defaults (overlap 3, error rate 0.1), min_length 36.

  python tools/readtrim_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--out profiles/readtrim_probe.json]

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
TRUSEQ = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def enumerate_once(pp, ix, path, dev, batch_bytes, threads, flt, trim):
    """(records scanned, records handed to the host, bytes copied to the host, seconds)."""
    cur = pp.Cursor(ix, path, batch_bytes=batch_bytes, threads=threads, device=dev, filter=flt, trim=trim)
    scanned = got = nbytes = 0
    t1 = time.perf_counter()
    for b in cur:
        scanned += b.nrecords
        if flt is None and trim is None:
            got += b.nrecords
            nbytes += int(b.raw_off[-1]) + 16 * b.nrecords
        else:
            s = b.selected
            got += s.records
            nbytes += s.nbytes + (32 if trim is None else 40) * s.records + 8   # text, descriptors, recno, sel_off, windows
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readtrim_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("readtrim_probe: no GPU (nothing is measured without one)")
    seg = 262_144                                    # records per segment: ~100 MB of 150 bp text
    repeats = max(1, round(a.gib * (1 << 30) / (seg * 385)))
    tf = TiledFile(seg, repeats, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_readtrim_{os.getpid()}.fastq.gz")
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
               "kernels": {}, "from_file": {}}
        realistic = pp.ReadTrim(trailing_quality=20, window=(4, 20), adapter=TRUSEQ, min_length=36)
        quality = pp.ReadTrim(trailing_quality=20, window=(4, 20), min_length=36)
        every = pp.ReadFilter(min_length=1)

        # ---- kernels on a resident one-batch shard ----
        n = tf.npoints - 1
        _, i0, _, _ = ix.point_fields(0)
        _, i1, _, _ = ix.point_fields(n)
        with open(path, "rb") as f:
            f.seek(i0 - 1)
            comp = np.frombuffer(f.read(i1 - i0 + 1), np.uint8)
        sh = pp.Shard(ix, comp, 0, n, device=dev).run()
        r0 = sh.trim_reads(realistic, windows=False)
        out["file"] = {"bases": r0.bases, "kept": r0.kept, "trimmed": r0.trimmed, "cut": r0.cut,
                       "bases_window": r0.bases_window, "bases_kept": r0.bases_kept}
        fn = _lib.lib.ppgx_readtrim_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
        for key, trim in (("realistic", realistic), ("quality_cuts", quality)):
            s = trim.struct()
            ms = (C.c_float * 4)()
            pp.check(fn(sh.handle, C.byref(s), 1, 9, ms), "ppgx_readtrim_times")
            out["kernels"]["trim_" + key] = {"layout_ms": ms[0], "measure_no_adapter_ms": ms[1], "measure_ms": ms[2],
                                             "decide_ms": ms[3], "adapter": bool(s.ops & 8)}
        ff = _lib.lib.ppgx_readfilter_times
        ff.restype = C.c_int
        ff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        s = every.struct()
        ms = (C.c_float * 3)()
        pp.check(ff(sh.handle, C.byref(s), 1, 0, 0, 9, ms), "ppgx_readfilter_times")
        out["kernels"]["read_filter"] = {"layout_ms": ms[0], "measure_ms": ms[1], "decide_ms": ms[2]}
        qn = _lib.lib.ppgx_seqquery_times
        qn.restype = C.c_int
        qn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_float)]
        for key, pat in (("seq_query_census", b""), ("seq_query_pattern12", PATTERN)):
            ms = (C.c_float * 4)()
            pp.check(qn(sh.handle, pat if pat else None, len(pat), 9, ms), "ppgx_seqquery_times")
            out["kernels"][key] = {"layout_ms": ms[0] + ms[1], "query_ms": ms[2], "reduce_ms": ms[3]}
        del sh

        # ---- from the file ----
        fq = pp.BatchedFASTQ(ix, path, device=dev)
        fq.query_out_capacity = bb

        def count_trimmed():
            fq.Dispose()       # the count reads and uploads the file again
            t0 = time.perf_counter()
            count_trimmed.kept = fq.CountTrimmed(realistic).kept      # the answer: no record reaches the host
            return nrec, 0, 0, time.perf_counter() - t0

        modes = {"count_trimmed_from_file": count_trimmed,
                 "where_trim": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, None, realistic),
                 "where_filter_every": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, every, None),
                 "text_cursor": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, None, None)}
        runs = {k: [] for k in modes}
        seen = {}
        for r in range(a.warmups + a.runs):          # alternating
            for name, f_ in modes.items():
                scanned, got, nbytes, sec = f_()
                assert scanned == nrec, (name, scanned, nrec)
                seen[name] = (got, nbytes)
                if r >= a.warmups:
                    runs[name].append(sec)
        assert seen["where_trim"][0] == count_trimmed.kept == out["file"]["kept"], (seen, out["file"])
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
