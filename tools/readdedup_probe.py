"""The read dedup against the read filter, measured in one process on the GPU box (one pass; run it under a time
limit), on a ~1 GiB synthetic FASTQ member of 150 bp reads (ppg_synth_fastq, written to $TMPDIR with its
index).  Unlike the other probes' member this one is a single segment, not a tile repeated: every read is
generated on its own, so that "as generated" means all distinct.

  kernels   layout, measure, insert (with the table made empty first), decide + totals and levels on a resident
            one-batch shard (hipEvents, the median of 9), at the smallest legal table, for three cases on the
            same resident text:
              distinct    whole reads as generated;
              copy_heavy  windows the probe forges: every second record keeps its first 6 bases alone, so half
                          the records are copies of at most 4,096 keys;
              hot_key     windows of length 0: every record has the empty key, one row takes every insert.
            ppg_rf_measure (the read filter: the same Sequence bytes, and the Quality bytes) is timed in the
            same process on the same batch as the yardstick
  counts    from the file, alternating, warm-ups first, the median of the runs: Duplication() (its counting run
            and its dedup run, the file read and uploaded again) and CountPassing()

  python tools/readdedup_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--out profiles/readdedup_probe.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readdedup_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("readdedup_probe: no GPU (nothing is measured without one)")
    records = max(1, round(a.gib * (1 << 30) / (262_144 * 385))) * 262_144     # the other probes' record count
    tf = TiledFile(records, 1, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_readdedup_{os.getpid()}.fastq.gz")
    try:
        with open(path, "wb") as f:
            for lo in range(0, tf.file_len, 1 << 30):
                f.write(tf.file_bytes(lo, min(tf.file_len, lo + (1 << 30))))
        ix = tf.index(0, tf.npoints)
        dev = pp.Device(0)
        nrec = tf.expected_records()
        slots = pp.ReadDedup.min_slots(nrec)
        out = {"build_id": _lib.lib.ppg_build_id().decode(), "text_GiB": int(tf.text.size) / (1 << 30),
               "gz_GB": tf.file_len / 1e9, "records": nrec, "chunk_records": a.chunk, "chunks": tf.npoints - 1,
               "batch_MiB": a.batch_mib, "warmups": a.warmups, "runs": a.runs, "slots": slots,
               "table_bytes": 24 * slots, "kernels": {}, "from_file": {}}
        every = pp.ReadFilter(min_length=1)

        # ---- kernels on a resident one-batch shard ----
        n = tf.npoints - 1
        _, i0, _, _ = ix.point_fields(0)
        _, i1, _, _ = ix.point_fields(n)
        with open(path, "rb") as f:
            f.seek(i0 - 1)
            comp = np.frombuffer(f.read(i1 - i0 + 1), np.uint8)
        sh = pp.Shard(ix, comp, 0, n, device=dev).run()
        assert sh.batches == 1 and sh.total_records == nrec
        tdev = torch.device("cuda", dev.device)
        table = torch.zeros((slots, 3), dtype=torch.int64, device=tdev)
        heavy = torch.zeros((nrec, 2), dtype=torch.int32, device=tdev)
        heavy[:, 1] = 150
        heavy[1::2, 1] = 6
        hot = torch.zeros((nrec, 2), dtype=torch.int32, device=tdev)
        cases = (("distinct", None), ("copy_heavy", heavy), ("hot_key", hot))
        fn = _lib.lib.ppgx_readdedup_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
        for key, rows in cases:
            r = sh.dedup_reads(pp.ReadDedup(), windows=rows, table=table)
            assert r.participating == nrec and r.overflow == 0 and r.level_reads.sum() == nrec, r
            dev.after_torch()
            s = pp.ReadDedup().struct(use_windows=rows is not None)
            ms = (C.c_float * 5)()
            pp.check(fn(sh.handle, C.byref(s), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                        nrec if rows is not None else 0, C.c_void_p(table.data_ptr()), slots, 9, ms), "ppgx_readdedup_times")
            out["kernels"][key] = {"layout_ms": ms[0], "measure_ms": ms[1], "init_insert_ms": ms[2], "decide_ms": ms[3],
                                   "levels_ms": ms[4], "unique": r.unique, "max_count": r.max_count, "key_bases": r.bases,
                                   "duplication_rate": r.duplication_rate}
        ff = _lib.lib.ppgx_readfilter_times
        ff.restype = C.c_int
        ff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        s = every.struct()
        ms = (C.c_float * 3)()
        pp.check(ff(sh.handle, C.byref(s), 1, 0, 0, 9, ms), "ppgx_readfilter_times")
        out["kernels"]["read_filter"] = {"layout_ms": ms[0], "measure_ms": ms[1], "decide_ms": ms[2]}
        del sh, table, heavy, hot

        # ---- from the file ----
        fq = pp.BatchedFASTQ(ix, path, device=dev)
        fq.query_out_capacity = a.batch_mib << 20

        def duplication():
            fq.Dispose()       # the count reads and uploads the file again
            t0 = time.perf_counter()
            duplication.seen = fq.Duplication().participating
            return time.perf_counter() - t0

        def passing():
            fq.Dispose()
            t0 = time.perf_counter()
            passing.seen = fq.CountPassing(every).passed
            return time.perf_counter() - t0

        modes = {"duplication_from_file": duplication, "count_passing_from_file": passing}
        runs = {k: [] for k in modes}
        for r in range(a.warmups + a.runs):          # alternating
            for name, f_ in modes.items():
                sec = f_()
                if r >= a.warmups:
                    runs[name].append(sec)
        assert duplication.seen == passing.seen == nrec, (duplication.seen, passing.seen, nrec)
        for name, secs in runs.items():
            sec = statistics.median(secs)
            out["from_file"][name] = {"records_per_s": nrec / sec, "seconds_median": sec, "seconds_all": secs,
                                      "passes_over_the_file": 2 if name.startswith("duplication") else 1,
                                      "bytes_to_host": 8 * ((40 if name.startswith("duplication") else 265) + tf.npoints - 1)}
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
