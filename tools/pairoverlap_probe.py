"""The pair overlap against the read filter and the pack kernel, measured in one process on the GPU box (one pass;
run it under a time limit), on 2.88 M pairs of 150 bp reads.

  pairs     read 1 is every record of a ~1 GiB synthetic FASTQ member (TiledFile, one segment), packed without
            qualities by the pack kernel.  Read 2 is forged from it on the device, from fragments of known length
            F: a third shorter than the read (40 .. 149: read-through, both mates are cut), a third of 150 .. 270
            (the mates overlap by 30 or more), a sixth of 271 .. 400 (no overlap to find) and a sixth unrelated
            reads.  A fragment starts with read 1; read 2 is the first 150 bases of its reverse complement, the
            read-through filled with random bases.  Every pair with an overlap of 30 or more must come back with
            insert size F: the probe checks that before it times anything.
  kernel    ppg_po_overlap with fastp's parameters over all pairs, rows and found mask written (hipEvents, the
            median of 9), beside ppg_rf_measure and the pack kernel without qualities on read 1's resident batch.
  compares  derived from the semantics, not counted by the kernel: a pair's candidates are tried in order up to
            the accepted one (all 241 when none is), `first_words` is one 32-base word compare per candidate tried,
            `whole_words` every word of every tried candidate's overlap (at most 5).  The kernel does at least the
            first and at most the second per candidate, plus the rest of the round of 64 in which the winner sits.

  python tools/pairoverlap_probe.py [--gib 1.0] [--chunk 1000] [--out profiles/pairoverlap_probe.json]

Writes the kernel ms and the compares per second, with ppg_build_id, as JSON."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ, MIN_OV = 150, 30


def forge_mates(p1, n, tdev, torch):
    """(PackedReads of read 2, fragment lengths F with 0 for an unrelated pair) from read 1's planes."""
    import parallelparsing_amd as pp
    g = torch.Generator(device=tdev).manual_seed(20260421)
    sh16 = 2 * torch.arange(16, device=tdev, dtype=torch.int64)
    words = (p1.bases[:10 * n].view(n, 10).to(torch.int64) & 0xFFFFFFFF)
    codes1 = ((words[:, :, None] >> sh16) & 3).reshape(n, 160)[:, :READ].to(torch.uint8)
    kind = torch.randint(0, 6, (n,), generator=g, device=tdev)
    F = torch.where(kind < 2, torch.randint(40, 150, (n,), generator=g, device=tdev),
                    torch.where(kind < 4, torch.randint(150, 271, (n,), generator=g, device=tdev),
                                torch.randint(271, 401, (n,), generator=g, device=tdev)))
    frag = torch.cat([codes1, torch.randint(0, 4, (n, 400 - READ), generator=g, device=tdev, dtype=torch.uint8)], dim=1)
    j = torch.arange(READ, device=tdev)
    src = F[:, None] - 1 - j[None, :]                                     # read 2's base j is the complement of this one
    r2 = torch.where(src >= 0, 3 - frag.gather(1, src.clamp(min=0)),
                     torch.randint(0, 4, (n, READ), generator=g, device=tdev, dtype=torch.uint8))
    unrelated = kind == 5
    r2[unrelated] = torch.randint(0, 4, (int(unrelated.sum()), READ), generator=g, device=tdev, dtype=torch.uint8)
    F = torch.where(unrelated, torch.zeros_like(F), F)
    del frag, src
    padded = torch.zeros((n, 160), dtype=torch.int64, device=tdev)
    padded[:, :READ] = r2
    w = (padded.view(n, 10, 16) << sh16).sum(dim=2)
    w = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32).reshape(-1)
    p2 = pp.PackedReads(torch.arange(n + 1, device=tdev, dtype=torch.int64) * 160,
                        torch.full((n,), READ, dtype=torch.int32, device=tdev), w.contiguous(),
                        torch.zeros(5 * n, dtype=torch.int32, device=tdev), None, n, 160 * n)
    return p2, F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairoverlap_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import parallelparsing_amd as pp
    from parallelparsing_amd import _lib
    from parallelparsing_amd.tiled import TiledFile
    if pp.device_count() < 1:
        sys.exit("pairoverlap_probe: no GPU (nothing is measured without one)")
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
    p1 = sh.pack_sequences(quality=False)
    assert int(p1.seq_len.min()) == int(p1.seq_len.max()) == READ
    p2, F = forge_mates(p1, n, tdev, torch)

    # ---- the answer first ----
    o = pp.PairOverlap()
    r = pp.pair_overlap(p1, p2, o, device=dev)
    ov = torch.where(F <= READ, F, 2 * READ - F)
    expect = (F > 0) & (ov >= MIN_OV) & ~(p1.mask[:5 * n].view(n, 5) != 0).any(dim=1)   # (an N of read 1 is a mismatch)
    rows = r.rows.to(torch.int64)
    assert bool((rows[expect, 3] == F[expect]).all()) and bool((rows[expect, 0] == F[expect] - READ).all())
    assert bool((rows[expect, 2] == 0).all()) and r.found >= int(expect.sum())
    # the candidates of the semantics in order: d = 0 .. 120, then -1 .. -120; tried up to the winner
    cand_ov = torch.cat([READ - torch.arange(0, READ - MIN_OV + 1), READ - torch.arange(1, READ - MIN_OV + 1)]).to(tdev)
    cum_words = torch.cumsum((cand_ov + 31) // 32, 0)
    d = rows[:, 0]
    rank = torch.where(d >= 0, d, READ - MIN_OV - d)
    found = rows[:, 3] > 0
    tried = torch.where(found, rank + 1, torch.full_like(rank, cand_ov.numel()))
    first_words, whole_words = int(tried.sum()), int(cum_words[tried - 1].sum())

    # ---- the kernels ----
    views = [_lib.PpgPackedView(p.seq_off.data_ptr(), p.seq_len.data_ptr(), p.bases.data_ptr(), p.mask.data_ptr(), None, n)
             for p in (p1, p2)]
    fn = _lib.lib.ppgx_pairoverlap_times
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]
    s, ms = o.struct(), (C.c_float * 1)()
    dev.after_torch()
    pp.check(fn(dev.handle, C.byref(s), C.byref(views[0]), C.byref(views[1]), n, 9, ms), "ppgx_pairoverlap_times")
    overlap_ms = float(ms[0])
    ff = _lib.lib.ppgx_readfilter_times
    ff.restype = C.c_int
    ff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    fs, fms = pp.ReadFilter(min_length=1).struct(), (C.c_float * 3)()
    pp.check(ff(sh.handle, C.byref(fs), 1, 0, 0, 9, fms), "ppgx_readfilter_times")
    fp = _lib.lib.ppgx_seqpack_times
    fp.restype = C.c_int
    fp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    pms, pbytes = (C.c_float * 4)(), (C.c_int64 * 2)()
    pp.check(fp(sh.handle, 0, 9, pms, pbytes), "ppgx_seqpack_times")
    sec = overlap_ms / 1e3
    out = {"build_id": _lib.lib.ppg_build_id().decode(), "pairs": n, "read_len": READ, "reps": 9,
           "params": {"min_overlap": o.min_overlap, "max_diff": o.max_diff, "max_err_milli": o.max_err_milli},
           "forged": {"read_through_40_149": int(((F > 0) & (F < READ)).sum()), "overlapping_150_270": int(((F >= READ) & (F <= 270)).sum()),
                      "apart_271_400": int((F > 270).sum()), "unrelated": int((F == 0).sum())},
           "result": dict({k: getattr(r, k) for k in r.TOTALS}, clipped=list(r.clipped), median_insert=r.median_insert,
                          expected_found=int(expect.sum())),
           "kernels": {"pair_overlap_ms": overlap_ms, "read_filter_measure_ms": float(fms[1]),
                       "seq_pack_no_quality_ms": float(pms[2]), "pairs_per_s": n / sec},
           "compares": {"candidates_per_pair_max": int(cand_ov.numel()), "words_per_candidate_max": 5,
                        "first_words": first_words, "whole_words": whole_words,
                        "first_words_per_s": first_words / sec, "whole_words_per_s": whole_words / sec,
                        "note": "derived from the semantics and the rows, not counted by the kernel"},
           "bytes": {"packed_planes_per_set": int(p1.total_bases // 4 + p1.total_bases // 8 + 12 * n + 8), "rows": 16 * n}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
