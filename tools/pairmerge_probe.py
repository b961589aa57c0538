"""The pair merge against the pair overlap and the pack kernel, measured in one process on the GPU box (one pass;
run it under a time limit), on the 2.88 M pairs of 150 bp reads of tools/pairoverlap_probe.py.

  pairs     read 1 is every record of a ~1 GiB synthetic FASTQ member, packed with its qualities by the pack
            kernel; read 2 is forged from it on the device as in the overlap's probe (fragments of known length F),
            with independent quality bytes in [35, 74).  The rows are the overlap kernel's, under fastp's parameters.
  answer    before anything is timed: as many reads are merged as pairs were found, every merged read has length I,
            and for the pairs forged without an error the merged read is the known fragment (read 1's bases, then
            the complement of read 2's from its far end), checked on the first 262,144 merged reads.
  kernels   ppg_pm_count + ppg_pm_scan, ppg_pm_place, ppg_pm_emit with and without the output's quality plane
            (hipEvents, the median of 9), beside ppg_po_overlap on the same pairs and the pack kernel with
            qualities on read 1's resident batch.
  errors    the pairs above are forged without an error, so no unit of theirs has a disagreement and the emit never
            runs the branch that counts ties and corrected bases.  A second run replaces every base of read 2 by
            another at probability --sub-rate (0.01) and times the merge again on the rows the overlap finds then
            ("with_errors" in the JSON).
  bytes     derived from the formats, not counted: per merged read both mates' packed words that hold a position
            of [0, I) (8 + 4 + 32 B per 32-base unit), 32 B of PpgMergeRec each way, and 44 B (12 B without the
            quality plane) written per unit of the output, plus 12 B of seq_off / seq_len.

  python tools/pairmerge_probe.py [--gib 1.0] [--chunk 1000] [--out profiles/pairmerge_probe.json]

Writes the kernel ms, the merged reads per second and the bytes per second, with ppg_build_id, as JSON."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

READ = 150
HBM_BYTES_PER_S = 6.29e12      # a float4 copy on this part (79 % of the 8 TB/s of its specification)


def with_errors(p2, n, rate, tdev, torch):
    """Read 2 with every base replaced by another one at probability `rate`; the other planes are shared."""
    import parallelparsing_amd as pp
    g = torch.Generator(device=tdev).manual_seed(20261022)
    sh16 = 2 * torch.arange(16, device=tdev, dtype=torch.int64)
    codes = (((p2.bases.view(n, 10).to(torch.int64) & 0xFFFFFFFF)[:, :, None] >> sh16) & 3).reshape(n, 160)
    hit = torch.rand((n, 160), generator=g, device=tdev) < rate
    hit[:, READ:] = False
    codes = torch.where(hit, (codes + torch.randint(1, 4, (n, 160), generator=g, device=tdev)) & 3, codes)
    w = (codes.view(n, 10, 16) << sh16).sum(dim=2)
    w = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32).reshape(-1)
    return pp.PackedReads(p2.seq_off, p2.seq_len, w.contiguous(), p2.mask, p2.qual, n, 160 * n), int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--sub-rate", type=float, default=0.01, help="substitutions per base of read 2 in the second run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairmerge_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    from pairoverlap_probe import forge_mates
    if pp.device_count() < 1:
        sys.exit("pairmerge_probe: no GPU (nothing is measured without one)")
    records = max(1, round(a.gib * (1 << 30) / (262_144 * 385))) * 262_144     # the other probes' record count
    tf = TiledFile(records, 1, a.chunk, threads=16)
    ix = tf.index(0, tf.npoints)
    dev = pp.Device(0)
    tdev = torch.device("cuda", dev.device)
    n = tf.expected_records()
    npts = tf.npoints - 1
    _, i0, _, _ = ix.point_fields(0)
    _, i1, _, _ = ix.point_fields(npts)
    comp = np.frombuffer(tf.file_bytes(i0 - 1, i1), np.uint8)
    sh = pp.Shard(ix, comp, 0, npts, device=dev).run()
    assert sh.batches == 1 and sh.total_records == n
    p1 = sh.pack_sequences(quality=True)
    assert int(p1.seq_len.min()) == int(p1.seq_len.max()) == READ
    p2, F = forge_mates(p1, n, tdev, torch)
    g = torch.Generator(device=tdev).manual_seed(20261021)
    q2 = torch.zeros((n, 160), dtype=torch.uint8, device=tdev)
    q2[:, :READ] = torch.randint(35, 74, (n, READ), generator=g, device=tdev, dtype=torch.uint8)
    p2.qual = q2.reshape(-1)

    # ---- the answer first ----
    o = pp.PairOverlap()
    ov = pp.pair_overlap(p1, p2, o, found_mask=False, device=dev)
    r = pp.pair_merge(p1, p2, ov.rows, device=dev)
    rows = ov.rows.to(torch.int64)
    assert r.merged == ov.found and r.stale == 0 and r.overlap_bases == ov.overlap_bases
    assert r.disagree + r.n_filled + r.n_both == ov.mismatches
    pair_of = r.pair_of
    assert bool((r.reads.seq_len[:r.merged].to(torch.int64) == rows[pair_of, 3]).all()) and r.merged_bases == int(rows[:, 3].sum())
    ns = min(r.merged, 262_144)
    pr, off = pair_of[:ns], r.reads.seq_off[:ns]
    sh16 = 2 * torch.arange(16, device=tdev, dtype=torch.int64)
    # (a record's words and those behind them, which the comparison below leaves out; the last record's are clamped)
    codes = lambda p, first, nw: (((p.bases.to(torch.int64)[((first[:, None] >> 4) + torch.arange(nw, device=tdev)[None, :])   # noqa: E731
                                                            .clamp(max=p.bases.numel() - 1)] & 0xFFFFFFFF)[:, :, None] >> sh16) & 3
                                  ).reshape(first.numel(), 16 * nw)
    Fm = rows[pr, 3]
    exact = (rows[pr, 2] == 0) & (F[pr] == Fm) & ~(p1.mask[:5 * n].view(n, 5)[pr] != 0).any(dim=1)   # forged without an error
    got = codes(r.reads, off, 18)                                     # up to 288 bases (the longest I here is 270)
    c1, c2 = codes(p1, p1.seq_off[pr], 10), codes(p2, p2.seq_off[pr], 10)
    pos = torch.arange(288, device=tdev)[None, :]
    want = torch.where(pos < READ, torch.nn.functional.pad(c1, (0, 128)), 3 - c2.gather(1, (Fm[:, None] - 1 - pos).clamp(0, 159)))
    inside = pos < Fm[:, None]
    assert int(exact.sum()) > ns // 2 and bool(((got == want) | ~inside)[exact].all())
    del got, c1, c2, want, inside

    # ---- the kernels ----
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(),
                                p.qual.data_ptr(), n) for p in (p1, p2)]
    fm = _lib.lib.ppgx_pairmerge_times
    fm.restype = C.c_int
    fm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float),
                   C.POINTER(C.c_int64)]
    m, mms, sizes = pp.PairMerge().struct(), (C.c_float * 4)(), (C.c_int64 * 2)()
    dev.after_torch()
    pp.check(fm(dev.handle, C.byref(m), C.byref(views[0]), C.byref(views[1]), n, C.c_void_p(ov.rows.data_ptr()), 9, mms, sizes),
             "ppgx_pairmerge_times")
    assert list(sizes) == [r.merged, r.padded_bases]
    fo = _lib.lib.ppgx_pairoverlap_times
    fo.restype = C.c_int
    fo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    s, oms = o.struct(), (C.c_float * 1)()
    pp.check(fo(dev.handle, C.byref(s), C.byref(views[0]), C.byref(views[1]), n, 9, oms), "ppgx_pairoverlap_times")
    fp = _lib.lib.ppgx_seqpack_times
    fp.restype = C.c_int
    fp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    pms, pbytes = (C.c_float * 4)(), (C.c_int64 * 2)()
    pp.check(fp(sh.handle, 1, 9, pms, pbytes), "ppgx_seqpack_times")

    # ---- the same pairs with sequencing errors: the emit's disagreement branch (ties, corrected) runs ----
    p2e, nsub = with_errors(p2, n, a.sub_rate, tdev, torch)
    ove = pp.pair_overlap(p1, p2e, o, found_mask=False, device=dev)
    re_ = pp.pair_merge(p1, p2e, ove.rows, device=dev)
    assert re_.merged == ove.found and re_.stale == 0 and re_.overlap_bases == ove.overlap_bases
    assert re_.disagree + re_.n_filled + re_.n_both == ove.mismatches and re_.disagree > 0 and min(re_.corrected) > 0
    viewe = _lib.PpgPackedView(p2e.seq_off.data_ptr(), p2e.seq_len.data_ptr(), p2e.bases.data_ptr(), p2e.mask.data_ptr(),
                               p2e.qual.data_ptr(), n)
    emms, esizes = (C.c_float * 4)(), (C.c_int64 * 2)()
    dev.after_torch()
    pp.check(fm(dev.handle, C.byref(m), C.byref(views[0]), C.byref(viewe), n, C.c_void_p(ove.rows.data_ptr()), 9, emms, esizes),
             "ppgx_pairmerge_times")
    assert list(esizes) == [re_.merged, re_.padded_bases]
    errors = {"sub_rate": a.sub_rate, "substitutions": nsub,
              "result": dict({k: getattr(re_, k) for k in re_.TOTALS}, agree=re_.agree, corrected=list(re_.corrected)),
              "kernels": {"merge_count_scan_ms": float(emms[0]), "merge_place_ms": float(emms[1]), "merge_emit_ms": float(emms[2]),
                          "merge_emit_no_quality_ms": float(emms[3]),
                          "merged_reads_per_s_emit": re_.merged / (float(emms[2]) / 1e3)}}

    # ---- the bytes, from the formats ----
    I, d = rows[pair_of, 3], rows[pair_of, 0]
    units = int(r.padded_bases // 32)
    u1 = (torch.minimum(I, torch.full_like(I, READ)) + 31) // 32                      # read 1's words with a position < I
    lo2 = torch.clamp(-d, min=0)                                                      # read 2's positions [0, L2 - max(-d, 0))
    u2 = (READ - lo2 + 31) // 32
    read_b = 44 * int((u1 + u2).sum()) + 32 * r.merged
    write_q, write_nq = 44 * units + 44 * r.merged, 12 * units + 44 * r.merged        # planes + PpgMergeRec + seq_off / seq_len
    emit_q, emit_nq = float(mms[2]) / 1e3, float(mms[3]) / 1e3
    out = {"build_id": _lib.lib.ppg_build_id().decode(), "pairs": n, "read_len": READ, "reps": 9,
           "params": {"min_overlap": o.min_overlap, "max_diff": o.max_diff, "max_err_milli": o.max_err_milli,
                      "qual_hi": int(m.qual_hi), "qual_lo": int(m.qual_lo)},
           "result": dict({k: getattr(r, k) for k in r.TOTALS}, agree=r.agree, corrected=list(r.corrected),
                          checked_error_free=int(exact.sum())),
           "kernels": {"merge_count_scan_ms": float(mms[0]), "merge_place_ms": float(mms[1]), "merge_emit_ms": float(mms[2]),
                       "merge_emit_no_quality_ms": float(mms[3]), "pair_overlap_ms": float(oms[0]),
                       "seq_pack_quality_ms": float(pms[2]),
                       "merged_reads_per_s": r.merged / ((float(mms[0]) + float(mms[1]) + float(mms[2])) / 1e3),
                       "merged_reads_per_s_emit": r.merged / emit_q},
           "bytes": {"units": units, "read": read_b, "written": write_q, "written_no_quality": write_nq,
                     "read_per_merged": read_b / r.merged, "written_per_merged": write_q / r.merged,
                     "emit_bytes_per_s": (read_b + 44 * units) / emit_q, "emit_no_quality_bytes_per_s": (read_b + 12 * units) / emit_nq,
                     "hbm_share": (read_b + 44 * units) / emit_q / HBM_BYTES_PER_S,
                     "hbm_share_no_quality": (read_b + 12 * units) / emit_nq / HBM_BYTES_PER_S,
                     "note": "derived from the formats, not counted by the kernel; hbm_share is of a 6.29 TB/s copy"},
           "with_errors": errors}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
