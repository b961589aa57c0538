"""The k-mer counter against the dedup's insert and the pack kernel, measured in one process on the GPU box (one
pass; run it under a time limit), k = 21 canonical on three packed read sets forged on the device:

  genome    2.88 M reads of 150 bp sampled from a 4 Mbase random genome, either strand, 1 % substitutions: the
            realistic case, ~108 x coverage; the distinct keys are the genome's and the errors'.
  distinct  500,000 random reads: 65 M k-mers, practically all distinct, in a table of 2 GiB: the table's worst case.
  polyg     `genome` with every tenth read replaced by poly-G: one hot key with 37 M occurrences.

  kernels   ppgx_kmercount_times per input (hipEvents, the median of 5): the table made empty, the unit table and
            totals, the insert, the spectrum's passes, a select of the rows with count >= 2 and a lookup of their
            keys; beside them, on the resident batch of a ~1 GiB synthetic FASTQ member (TiledFile, one segment,
            2.88 M records), ppg_dd_insert with its table's emptying and the pack kernel without qualities.
  calls     whole ppg_kmers_count calls on `genome` (wall clock, scratch allocation and the result's copy
            included, the median of 3): the table the doubling ends with, and the undersized ones before it, which
            must fail fast.

  python tools/kmercount_probe.py [--reads 2883584] [--out profiles/kmercount_probe.json]

Writes the times and the valid k-mers per second, with ppg_build_id, as JSON."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ, K, GENOME = 150, 21, 4_000_000


def pack_codes(codes, torch, pp):
    """A PackedReads (no N, no qualities) of an (n, 150) uint8 tensor of 2-bit codes, in slices to bound the scratch."""
    n = codes.shape[0]
    tdev = codes.device
    sh16 = 2 * torch.arange(16, device=tdev, dtype=torch.int64)
    words = torch.empty(10 * n, dtype=torch.int32, device=tdev)
    step = 1 << 18
    for a in range(0, n, step):
        c = codes[a:a + step]
        padded = torch.zeros((c.shape[0], 160), dtype=torch.int64, device=tdev)
        padded[:, :READ] = c
        w = (padded.view(-1, 10, 16) << sh16).sum(dim=2)
        words[10 * a:10 * (a + c.shape[0])] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32).reshape(-1)
    return pp.PackedReads(torch.arange(n + 1, device=tdev, dtype=torch.int64) * 160,
                          torch.full((n,), READ, dtype=torch.int32, device=tdev), words,
                          torch.zeros(5 * n, dtype=torch.int32, device=tdev), None, n, 160 * n)


def forge_genome_reads(n, g, tdev, torch):
    genome = torch.randint(0, 4, (GENOME,), generator=g, device=tdev, dtype=torch.uint8)
    start = torch.randint(0, GENOME - READ, (n,), generator=g, device=tdev)
    codes = torch.empty((n, READ), dtype=torch.uint8, device=tdev)
    step = 1 << 18
    j = torch.arange(READ, device=tdev)
    for a in range(0, n, step):
        c = genome[start[a:a + step, None] + j[None, :]]
        err = torch.rand(c.shape, generator=g, device=tdev) < 0.01
        c = torch.where(err, (c + torch.randint(1, 4, c.shape, generator=g, device=tdev, dtype=torch.uint8)) & 3, c)
        flip = torch.rand((c.shape[0], 1), generator=g, device=tdev) < 0.5
        codes[a:a + step] = torch.where(flip, 3 - c.flip(1), c)
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_883_584)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmercount_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("kmercount_probe: no GPU (nothing is measured without one)")
    dev = pp.Device(0)
    tdev = torch.device("cuda", dev.device)
    g = torch.Generator(device=tdev).manual_seed(20261021)
    kc = pp.KmerCount(K, True)
    per_read = READ - K + 1

    fn = _lib.lib.ppgx_kmercount_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]

    def view_of(p):
        return _lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(), None, p.records)

    def one_call(p, table):
        """(status, wall ms) of a whole ppg_kmers_count into `table`."""
        v, s, res, spec = view_of(p), kc.struct(), _lib.PpgKmerCountResult(), np.zeros(_lib.PPG_KMER_SPECTRUM, np.int64)
        torch.cuda.synchronize()
        dev.after_torch()
        t0 = time.perf_counter()
        rc = _lib.lib.ppg_kmers_count(dev.handle, C.byref(s), C.byref(v), None, 0, None, 0, C.c_void_p(table.data_ptr()),
                                      table.numel() // 2, C.byref(res), spec.ctypes.data_as(C.c_void_p), spec.size)
        return rc, 1e3 * (time.perf_counter() - t0)

    def measure(name, codes, calls=False):
        p = pack_codes(codes, torch, pp)
        n = p.records
        r = pp.count_kmers(p, kc, device=dev)                               # sized by doubling
        assert r.kmers == n * per_read == r.total_count and r.invalid == 0 and r.overflow == 0
        slots, table = r.slots, r.table
        ms, sizes = (C.c_float * 6)(), (C.c_int64 * 4)()
        v, s = view_of(p), kc.struct()
        dev.after_torch()
        pp.check(fn(dev.handle, C.byref(s), C.byref(v), C.c_void_p(table.data_ptr()), slots, 5, ms, sizes), "ppgx_kmercount_times")
        assert list(sizes)[:2] == [r.kmers, r.distinct] and sizes[3] == 0
        o = {"reads": n, "kmers": r.kmers, "distinct": r.distinct, "singletons": r.singletons, "max_count": r.max_count,
             "max_key": kc.word(r.max_key), "slots": slots, "table_bytes": 16 * slots, "doubling_retries": r.retries,
             "empty_table_ms": ms[0], "unit_table_ms": ms[1], "insert_ms": ms[2], "spectrum_ms": ms[3],
             "select_ge2_ms": ms[4], "select_ge2_rows": int(sizes[2]), "lookup_ms": ms[5],
             "kmers_per_s": r.kmers / (ms[2] / 1e3), "spectrum_head": r.spectrum[:8].tolist()}
        if calls:
            o["calls"] = {}
            for sl in (slots, slots // 2, slots // 4, 1 << 20, 64):
                t = table[:sl]
                got = sorted(one_call(p, t) for _ in range(3))
                assert all(rc == (0 if sl == slots else _lib.PPG_BUF_ERROR) for rc, _ in got), (sl, got)
                o["calls"][str(sl)] = {"status": "ok" if sl == slots else "buf_error", "wall_ms": got[1][1]}
        print(name, json.dumps(o), flush=True)
        del p, r, table
        return o

    out = {"build_id": _lib.lib.ppg_build_id().decode(), "k": K, "canonical": True, "read_len": READ, "reps": 5, "inputs": {}}
    codes = forge_genome_reads(a.reads, g, tdev, torch)
    out["inputs"]["genome"] = dict(measure("genome", codes, calls=True), genome_bases=GENOME, substitutions=0.01)
    codes[::10] = 2
    out["inputs"]["polyg"] = dict(measure("polyg", codes), polyg_reads=(a.reads + 9) // 10)
    del codes
    out["inputs"]["distinct"] = measure("distinct", torch.randint(0, 4, (500_000, READ), generator=g, device=tdev, dtype=torch.uint8))
    torch.cuda.empty_cache()

    # ---- the yardsticks: the dedup's insert and the pack kernel on a resident batch of as many records ----
    records = max(1, round(a.reads / 262_144)) * 262_144
    tf = TiledFile(records, 1, a.chunk, threads=16)
    ix = tf.index(0, tf.npoints)
    npts = tf.npoints - 1
    _, i0, _, _ = ix.point_fields(0)
    _, i1, _, _ = ix.point_fields(npts)
    sh = pp.Shard(ix, np.frombuffer(tf.file_bytes(i0 - 1, i1), np.uint8), 0, npts, device=dev).run()
    nrec = sh.total_records
    assert sh.batches == 1 and nrec == tf.expected_records()
    fd = _lib.lib.ppgx_readdedup_times
    fd.restype = C.c_int
    fd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    dslots = pp.ReadDedup.min_slots(nrec)
    dtable = torch.zeros((dslots, 3), dtype=torch.int64, device=tdev)
    dms, ds = (C.c_float * 5)(), pp.ReadDedup().struct()
    dev.after_torch()
    pp.check(fd(sh.handle, C.byref(ds), None, 0, C.c_void_p(dtable.data_ptr()), dslots, 9, dms), "ppgx_readdedup_times")
    fp = _lib.lib.ppgx_seqpack_times
    fp.restype = C.c_int
    fp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    pms, pbytes = (C.c_float * 4)(), (C.c_int64 * 2)()
    pp.check(fp(sh.handle, 0, 9, pms, pbytes), "ppgx_seqpack_times")
    out["yardsticks"] = {"records": nrec, "dedup_init_insert_ms": dms[2], "dedup_slots": dslots, "seq_pack_no_quality_ms": pms[2]}
    out["derived"] = {"streamed_bytes_per_record": 40 + 20 + 12 + 2 * 20, "starts_per_record": per_read,
                      "atomics_per_record_max": 2 * per_read, "table_row_bytes": 16,
                      "note": "from the formats, not counted by the kernel; equal keys combined before memory lower the atomics"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
