"""Packed reads against text, measured in one process on the GPU box (one pass; run it under a
time limit): full enumeration of a ~1 GiB synthetic FASTQ member (ppg_synth_fastq, 150 bp, written
to $TMPDIR with its index) through the text cursor, the packed cursor with qualities and the packed
cursor without -- alternating, two warm-ups each, the median of five -- and the layout / pack
kernels beside ppg_pack_raw on a resident one-batch shard of the same member (hipEvents).

  python tools/seqpack_probe.py [--gib 1.0] [--chunk 1000] [--batch-mib 256] [--threads 8] [--out profiles/seqpack_probe.json]

Writes records/s, bytes crossing PCIe (device -> host) per record and kernel ms, with ppg_build_id,
as JSON.  PPG_CURSOR_VERBOSE=1 in the environment adds the cursor's per-batch stage times on stderr."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = (("text", False, False), ("packed_qual", True, True), ("packed_noqual", True, False))


def enumerate_once(pp, ix, path, dev, batch_bytes, threads, packed, quality):
    t0 = time.perf_counter()
    cur = pp.Cursor(ix, path, batch_bytes=batch_bytes, threads=threads, device=dev, packed=packed, quality=quality)
    t_open = time.perf_counter() - t0
    nrec = d2h = nb = 0
    t1 = time.perf_counter()
    for b in cur:
        nrec += b.nrecords
        if packed:
            tb = b.packed.total_bases
            d2h += 8 * (b.nrecords + 1) + 4 * b.nrecords + tb // 4 + tb // 8 + (tb if quality else 0)
        else:
            d2h += int(b.raw_off[-1]) + 16 * b.nrecords
        nb += 1
    sec = time.perf_counter() - t1
    cur.close()
    return {"records": nrec, "seconds": sec, "open_s": t_open, "batches": nb, "d2h_bytes": d2h}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    # records per index chunk: one wave decodes a chunk, so a 1 GiB member in 10,000-record chunks is
    # 280 waves and every batch waits ~45 ms for its slowest wave, whatever crosses PCIe afterwards
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqpack_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("seqpack_probe: no GPU (nothing is measured without one)")
    seg = 262_144                                    # records per segment: ~100 MB of 150 bp text
    repeats = max(1, round(a.gib * (1 << 30) / (seg * 385)))
    tf = TiledFile(seg, repeats, a.chunk, threads=16)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ppg_seqpack_{os.getpid()}.fastq.gz")
    try:
        with open(path, "wb") as f:
            for lo in range(0, tf.file_len, 1 << 30):
                f.write(tf.file_bytes(lo, min(tf.file_len, lo + (1 << 30))))
        ix = tf.index(0, tf.npoints)
        pp.IndexIO.Serialize(ix, path + "i")
        dev = pp.Device(0)
        bb = a.batch_mib << 20
        runs = {m[0]: [] for m in MODES}
        for r in range(a.warmups + a.runs):          # alternating: text, packed, packed, text, ...
            for name, packed, quality in MODES:
                res = enumerate_once(pp, ix, path, dev, bb, a.threads, packed, quality)
                assert res["records"] == tf.expected_records(), (name, res["records"], tf.expected_records())
                if r >= a.warmups:
                    runs[name].append(res)
        out = {"build_id": _lib.lib.ppg_build_id().decode(), "text_GiB": int(tf.text.size) * repeats / (1 << 30),
               "gz_GB": tf.file_len / 1e9, "records": tf.expected_records(), "chunk_records": a.chunk,
               "chunks": tf.npoints - 1, "batch_MiB": a.batch_mib, "threads": a.threads, "warmups": a.warmups, "runs": a.runs, "enumeration": {}}
        for name, rs in runs.items():
            sec = statistics.median(x["seconds"] for x in rs)
            n = rs[0]["records"]
            out["enumeration"][name] = {
                "records_per_s": n / sec, "seconds_median": sec, "seconds_all": [x["seconds"] for x in rs],
                "open_s_median": statistics.median(x["open_s"] for x in rs), "batches": rs[0]["batches"],
                "d2h_bytes_per_record": rs[0]["d2h_bytes"] / n, "d2h_GBps": rs[0]["d2h_bytes"] / sec / 1e9}
        t = out["enumeration"]["text"]
        for name in ("packed_qual", "packed_noqual"):
            e = out["enumeration"][name]
            e["speedup_vs_text"] = e["records_per_s"] / t["records_per_s"]
            e["byte_ratio_vs_text"] = t["d2h_bytes_per_record"] / e["d2h_bytes_per_record"]
        # kernels on a resident one-batch shard of the same member
        n = tf.npoints - 1
        _, i0, _, _ = ix.point_fields(0)
        _, i1, _, _ = ix.point_fields(n)
        with open(path, "rb") as f:
            f.seek(i0 - 1)
            comp = np.frombuffer(f.read(i1 - i0 + 1), np.uint8)
        sh = pp.Shard(ix, comp, 0, n, device=dev).run()
        fn = _lib.lib.ppgx_seqpack_times
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
        out["kernels"] = {}
        for key, q in (("with_qual", 1), ("without_qual", 0)):
            ms, by = (C.c_float * 4)(), (C.c_int64 * 2)()
            pp.check(fn(sh.handle, q, 9, ms, by), "ppgx_seqpack_times")
            out["kernels"][key] = {"layout_ms": ms[0], "offsets_ms": ms[1], "pack_ms": ms[2], "pack_raw_ms": ms[3],
                                   "plane_bytes": by[0], "raw_text_bytes": by[1], "records": sh.total_records,
                                   "pack_GBps_written": by[0] / ms[2] / 1e6, "pack_raw_GBps_written": by[1] / ms[3] / 1e6}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
    finally:
        for p in (path, path + "i"):
            if os.path.exists(p):
                os.remove(p)


if __name__ == "__main__":
    main()
