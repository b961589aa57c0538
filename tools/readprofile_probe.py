"""The read profile against the read filter and the query, measured in one process on the GPU box (one pass;
run it under a time limit), on the member the seqpack, seqquery, seqselect, readfilter and readtrim probes
use: a ~1 GiB synthetic FASTQ member (ppg_synth_fastq, 150 bp, written to $TMPDIR with its index).

  kernels   layout, measure and finish + totals on a resident one-batch shard (hipEvents, the median of 9),
            for 160 and 1,024 positions, over every record and over the keep mask and the windows of the
            realistic trim (tools/readtrim_probe.py); ppg_rf_measure (the read filter: the same Sequence and
            Quality bytes) and ppg_seq_query are timed in the same process on the same batch as the yardsticks
  counts    from the file, alternating, warm-ups first, the median of the runs: Profile() and CountPassing()
            with the file read and uploaded again (decode + stage, nothing but the result to the host)

  python tools/readprofile_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--out profiles/readprofile_probe.json]

Writes kernel ms, records/s and the result's bytes, with ppg_build_id, as JSON."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readprofile_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("readprofile_probe: no GPU (nothing is measured without one)")
    seg = 262_144                                    # records per segment: ~100 MB of 150 bp text
    repeats = max(1, round(a.gib * (1 << 30) / (seg * 385)))
    tf = TiledFile(seg, repeats, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_readprofile_{os.getpid()}.fastq.gz")
    try:
        with open(path, "wb") as f:
            for lo in range(0, tf.file_len, 1 << 30):
                f.write(tf.file_bytes(lo, min(tf.file_len, lo + (1 << 30))))
        ix = tf.index(0, tf.npoints)
        dev = pp.Device(0)
        nrec = tf.expected_records()
        out = {"build_id": _lib.lib.ppg_build_id().decode(), "text_GiB": int(tf.text.size) * repeats / (1 << 30),
               "gz_GB": tf.file_len / 1e9, "records": nrec, "chunk_records": a.chunk, "chunks": tf.npoints - 1,
               "batch_MiB": a.batch_mib, "warmups": a.warmups, "runs": a.runs, "kernels": {}, "from_file": {}}
        realistic = pp.ReadTrim(trailing_quality=20, window=(4, 20), adapter=TRUSEQ, min_length=36)
        every = pp.ReadFilter(min_length=1)

        # ---- kernels on a resident one-batch shard ----
        n = tf.npoints - 1
        _, i0, _, _ = ix.point_fields(0)
        _, i1, _, _ = ix.point_fields(n)
        with open(path, "rb") as f:
            f.seek(i0 - 1)
            comp = np.frombuffer(f.read(i1 - i0 + 1), np.uint8)
        sh = pp.Shard(ix, comp, 0, n, device=dev).run()
        t = sh.trim_reads(realistic, mask=True, windows=True)
        r0 = sh.profile_reads(pp.ReadProfile(160))
        r1 = sh.profile_reads(pp.ReadProfile(160), mask=t.keep_mask, windows=t.windows)
        assert r0.profiled == nrec and r1.profiled == t.kept and r1.bases == t.bases_kept, (r0, r1, t)
        out["file"] = {"bases": r0.bases, "qual_bytes": r0.qual_bytes, "longer": r0.longer,
                       "quality_bins_in_use": int((r0.table["qhist"].sum(axis=0) > 0).sum()),
                       "trim_kept": t.kept, "trim_bases_kept": t.bases_kept}
        dev.after_torch()
        fn = _lib.lib.ppgx_readprofile_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
        for pos in (160, 1024):
            for key, (m, w) in (("all", (None, None)), ("trimmed", (t.keep_mask, t.windows))):
                s = pp.ReadProfile(pos).struct(m is not None, w is not None)
                ms = (C.c_float * 3)()
                pp.check(fn(sh.handle, C.byref(s), C.c_void_p(m.data_ptr()) if m is not None else None,
                            32 * m.numel() if m is not None else 0, C.c_void_p(w.data_ptr()) if w is not None else None,
                            w.shape[0] if w is not None else 0, 9, ms), "ppgx_readprofile_times")
                out["kernels"][f"profile_{pos}_{key}"] = {"layout_ms": ms[0], "measure_ms": ms[1], "finish_ms": ms[2],
                                                          "result_bytes": 8 * (173 + 72 * pos)}
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
        del sh, t

        # ---- from the file ----
        fq = pp.BatchedFASTQ(ix, path, device=dev)
        fq.query_out_capacity = a.batch_mib << 20

        def profile():
            fq.Dispose()       # the count reads and uploads the file again
            t0 = time.perf_counter()
            profile.seen = fq.Profile(pp.ReadProfile(160)).profiled
            return time.perf_counter() - t0

        def passing():
            fq.Dispose()
            t0 = time.perf_counter()
            passing.seen = fq.CountPassing(every).passed
            return time.perf_counter() - t0

        modes = {"profile_from_file": profile, "count_passing_from_file": passing}
        runs = {k: [] for k in modes}
        for r in range(a.warmups + a.runs):          # alternating
            for name, f_ in modes.items():
                sec = f_()
                if r >= a.warmups:
                    runs[name].append(sec)
        assert profile.seen == passing.seen == nrec, (profile.seen, passing.seen, nrec)
        for name, secs in runs.items():
            sec = statistics.median(secs)
            out["from_file"][name] = {"records_per_s": nrec / sec, "seconds_median": sec, "seconds_all": secs,
                                      "bytes_to_host": 8 * (173 + 72 * 160 + tf.npoints - 1) if name.startswith("profile") else
                                      8 * (265 + tf.npoints - 1)}
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
