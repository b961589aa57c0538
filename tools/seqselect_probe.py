"""Record selection against moving every record's text, measured in one process on the GPU box (one
pass; run it under a time limit), on the member tools/seqquery_probe.py uses: a ~1 GiB synthetic
FASTQ member (ppg_synth_fastq, 150 bp, written to $TMPDIR with its index).

  kernels   count, scan, place and copy on a resident one-batch shard (hipEvents, the median of 9),
            selecting every record (no mask), a random 10 % and 0.1 %, and the hits of "GTTATACACTGC";
            ppg_pack_raw -- the text cursor's kernel, which also moves every text byte once -- is timed
            on the same batch as the yardstick
  cursors   from the file, alternating, warm-ups first, the median of the runs: the select cursor with
            the pattern and with b"" (every record), the text cursor, and CountPattern with the file
            read and uploaded again (decode + query, no text to the host: the floor of a selective
            query); records/s and the bytes each copies to the host

  python tools/seqselect_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--out profiles/seqselect_probe.json]

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


def enumerate_once(pp, ix, path, dev, batch_bytes, threads, pattern):
    """(records scanned, records handed to the host, bytes copied to the host, seconds)."""
    cur = pp.Cursor(ix, path, batch_bytes=batch_bytes, threads=threads, device=dev, pattern=pattern)
    scanned = got = nbytes = 0
    t1 = time.perf_counter()
    for b in cur:
        scanned += b.nrecords
        if pattern is None:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqselect_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("seqselect_probe: no GPU (nothing is measured without one)")
    seg = 262_144                                    # records per segment: ~100 MB of 150 bp text
    repeats = max(1, round(a.gib * (1 << 30) / (seg * 385)))
    tf = TiledFile(seg, repeats, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_seqselect_{os.getpid()}.fastq.gz")
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
        fn = _lib.lib.ppgx_seqselect_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
        words = (sh.total_records + 31) // 32
        tdev = torch.device("cuda", dev.device)
        gen = torch.Generator(device=tdev).manual_seed(7)
        bit = torch.arange(32, dtype=torch.int64, device=tdev)

        def random_mask(p):
            hit = (torch.rand(words * 32, generator=gen, device=tdev) < p).reshape(-1, 32).to(torch.int64)
            return (hit << bit).sum(dim=1).to(torch.int32)      # (the low 32 bits)

        masks = (("all", None), ("random_10pct", random_mask(0.1)), ("random_0.1pct", random_mask(0.001)),
                 ("pattern_hits", sh.query_sequences(PATTERN, mask=True).hit_mask))
        for key, m in masks:
            torch.cuda.synchronize(tdev)
            dev.after_torch()
            ms, sz = (C.c_float * 5)(), (C.c_int64 * 3)()
            pp.check(fn(sh.handle, C.c_void_p(m.data_ptr()) if m is not None else None, 32 * words if m is not None else 0, 9,
                        ms, sz), "ppgx_seqselect_times")
            out["kernels"][key] = {"count_ms": ms[0], "scan_ms": ms[1], "place_ms": ms[2], "copy_ms": ms[3],
                                   "pack_raw_ms": ms[4], "selected_records": sz[0], "selected_bytes": sz[1],
                                   "raw_text_bytes": sz[2], "copy_over_pack_raw": ms[3] / ms[4],
                                   "copy_GBps_read_plus_written": 2 * sz[1] / ms[3] / 1e6 if ms[3] > 0 else None}
        del sh, masks

        # ---- from the file ----
        fq = pp.BatchedFASTQ(ix, path, device=dev)
        fq.query_out_capacity = bb

        def count_pattern():
            fq.Dispose()       # the query reads and uploads the file again
            t0 = time.perf_counter()
            count_pattern.hits = fq.CountPattern(PATTERN)      # the answer: no record reaches the host
            return nrec, 0, 0, time.perf_counter() - t0

        modes = {"select_cursor_pattern": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, PATTERN),
                 "select_cursor_all": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, b""),
                 "text_cursor": lambda: enumerate_once(pp, ix, path, dev, bb, a.threads, None),
                 "count_pattern_from_file": count_pattern}
        runs = {k: [] for k in modes}
        seen = {}
        for r in range(a.warmups + a.runs):          # alternating
            for name, f_ in modes.items():
                scanned, got, nbytes, sec = f_()
                assert scanned == nrec, (name, scanned, nrec)
                seen[name] = (got, nbytes)
                if r >= a.warmups:
                    runs[name].append(sec)
        assert seen["select_cursor_pattern"][0] == count_pattern.hits, (seen, count_pattern.hits)
        out["pattern_hits"] = count_pattern.hits
        assert seen["select_cursor_all"][0] == seen["text_cursor"][0] == nrec, seen
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
