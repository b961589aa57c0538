"""The record stages under the pair emission (include/ppgpu.h, the emit section; csrc/ppg_pairs.hip).

ppg_pairs_emit_begin runs a multi-batch shard's batches again as the windows advance: those re-runs do not run
the record stages, so at every point of an emission each attached stage's *_ready answer, result, per-chunk
counts and every caller buffer it wrote are bit-identical to what the shard's own run() left.
ppg_pairs_emit_run is the shards' own run: the stages run once per batch, are unready from the call until the
last window, and are ready after PPG_STREAM_END with what run() leaves on a twin shard; stopping early leaves
them unready.  The pair chunks stay oracle-exact with stages attached, in both forms.

Input: two mate files of 6,000 records of 150 bp (R1 with a full flush every 37 records, so Q1 duplicates
exist), chunk sizes that do not line up, 7 output batches per shard; a second R2 1,200 records short, so R1's last
batch holds no pair.  All seven stages on one mask and one rows tensor as in
test_gpu_readdedup.test_query_filter_trim_dedup_profile_select_chain, every caller buffer with 4 KiB of 0xA5
behind it.  The snapshot a comparison starts from is tied to the Python references of the stages first."""
import ctypes as C

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib, paired
from pairs_ref import mate_gz, oracle_records, check_window
import seqquery_ref as Q
from stage_rig import PATTERN, STAGES, Rig, assert_twins, references

pytestmark = pytest.mark.gpu

NREC, SHORT, K = 6000, 1200, 1000
CHUNKS = (300, 200)            # the files' chunk boundaries never line up
CAP = 384 << 10                # three chunks of output per batch


@pytest.fixture(scope="module")
def files():
    """gz: R1, R2, the short R2; per file its chunk size, oracle chunks and oracle records; refs of R1 and R2."""
    gz = [mate_gz(1, NREC, 0, flush_every=37), mate_gz(2, NREC, 1), mate_gz(2, NREC - SHORT, 1)]
    cs = (CHUNKS[0], CHUNKS[1], CHUNKS[1])
    ch = [Q.chunks_of(g, c) for g, c in zip(gz, cs)]
    recs = [oracle_records(g, c) for g, c in zip(gz, cs)]
    assert [len(r[0]) for r in recs] == [NREC, NREC, NREC - SHORT]
    assert recs[0][1] > 10 and recs[1][1] == 0 and recs[2][1] == 0   # R1 carries Q1 duplicates
    for c in ch[:2]:   # the per-chunk loops take two rounds in nearly every chunk
        assert sum(len(k[2]) > 256 for k in c) >= len(c) - 2
    return {"gz": gz, "cs": cs, "ch": ch, "recs": recs, "refs": [references(ch[0]), references(ch[1])]}


def rigs(files, device, r2=1, which=STAGES):
    rg = [Rig(files, 0, device, which, cap=CAP), Rig(files, r2, device, which, cap=CAP)]
    assert all(r.sh.batches >= 4 for r in rg)
    return rg


def recs_of(files, r2=1):
    return [files["recs"][0], files["recs"][r2]]


def emit_and_compare(pr, rg, snaps, recs, npairs, where):
    """One whole re-run emission: every window oracle-exact, everything as the snapshot after each."""
    seen, windows = set(), 0
    for j0, j1 in pr.emit(rg[0].sh, rg[1].sh, K):
        check_window(pr, j0, j1, K, recs, npairs, seen)
        windows += 1
        for r, s in zip(rg, snaps):
            r.assert_same(s, (where, "window", windows))
    assert seen == set(range(-(-npairs // K))) and windows > 1
    for r, s in zip(rg, snaps):
        r.assert_same(s, (where, "after the last window"))
    return windows


@pytest.mark.parametrize("short", [0, SHORT])
def test_rerun_emission_leaves_the_stages_alone(files, device, short):
    r2 = 2 if short else 1
    recs, npairs = recs_of(files, r2), NREC - short
    rg = rigs(files, device, r2)
    for r in rg:
        r.sh.run()
        r.assert_ready(1, "run")
    rg[0].assert_reference(files["refs"][0])
    if not short:
        rg[1].assert_reference(files["refs"][1])
    snaps = [r.snapshot() for r in rg]
    pr = paired.Pairs()
    res = pr.check(rg[0].sh, rg[1].sh)
    assert res["pairs"] == npairs and res["mismatches"] == short and res["duplicates"][0] == recs[0][1]
    if short:   # R1's last batch holds no pair: it is never run again
        b = rg[0].sh.record_base()
        assert b[-3] - recs[0][1] >= npairs
    for r, s in zip(rg, snaps):
        r.assert_same(s, "after the check")
    emit_and_compare(pr, rg, snaps, recs, npairs, "first emission")
    assert pr.emit_stats()["reruns"] > 0
    # an emission abandoned half way, then a second one on the same check
    it = pr.emit(rg[0].sh, rg[1].sh, K)
    seen = set()
    for _ in range(2):
        check_window(pr, *next(it), K, recs, npairs, seen)
    it.close()
    for r, s in zip(rg, snaps):
        r.assert_same(s, "stopped early")
    emit_and_compare(pr, rg, snaps, recs, npairs, "second emission")
    assert pr.emit_stats()["reruns"] > 0
    rg[0].assert_reference(files["refs"][0])


@pytest.mark.parametrize("stage", STAGES)
def test_rerun_emission_one_stage(files, device, stage):
    """Each stage attached alone, through one window of the re-run emission: a failure names the stage."""
    rg = rigs(files, device, which=(stage,))
    for r in rg:
        r.sh.run()
        r.assert_ready(1, "run")
    snaps = [r.snapshot() for r in rg]
    pr = paired.Pairs()
    assert pr.check(rg[0].sh, rg[1].sh)["mismatches"] == 0
    it = pr.emit(rg[0].sh, rg[1].sh, K)
    check_window(pr, *next(it), K, recs_of(files), NREC, set())
    assert pr.emit_stats()["reruns"] > 0
    for r, s in zip(rg, snaps):
        r.assert_same(s, stage)
    it.close()


@pytest.mark.parametrize("plain_first", [False, True])
def test_fused_emission_runs_the_stages_once(files, device, plain_first):
    """emit_run with every stage attached: unready from the call until the last window (also when an earlier
    plain run left them ready), ready after PPG_STREAM_END with what run() leaves on twin shards."""
    recs = recs_of(files)
    rg, twins = rigs(files, device), rigs(files, device)
    for t in twins:
        t.sh.run()
    if plain_first:
        for r in rg:
            r.sh.run()
            r.assert_ready(1, "plain run")
    pr = paired.Pairs()
    seen, windows = set(), 0
    for j0, j1 in pr.emit_run(rg[0].sh, rg[1].sh, K):
        windows += 1
        for r in rg:
            r.assert_ready(0, ("window", windows))
        check_window(pr, j0, j1, K, recs, NREC, seen)
    assert seen == set(range(-(-NREC // K))) and windows > 1 and pr.emit_stats()["reruns"] == 0
    for r in rg:
        r.assert_ready(1, "after the last window")
    assert_twins(rg, twins, "after the last window")
    for r, ref in zip(rg, files["refs"]):
        r.assert_reference(ref)
    assert pr.check(rg[0].sh, rg[1].sh)["mismatches"] == 0


def test_fused_emission_stopped_early(files, device):
    """Stopped after the first window: every stage unready, the shards unrun (a one-shot stage call is
    PPG_ARG_ERROR); a plain run afterwards leaves what it leaves on a twin."""
    rg, twins = rigs(files, device), rigs(files, device)
    for r in rg:                                     # (ready before: the emission has to take that back)
        r.sh.run()
    pr = paired.Pairs()
    it = pr.emit_run(rg[0].sh, rg[1].sh, K)
    check_window(pr, *next(it), K, recs_of(files), NREC, set())
    it.close()
    for r in rg:
        r.assert_ready(0, "stopped early")
        res = _lib.PpgSeqQueryResult()
        assert _lib.lib.ppg_shard_query_seq(r.sh.handle, *pp._pattern_arg(PATTERN), None, 0, None, C.byref(res)) == _lib.PPG_ARG_ERROR
        assert r.sh.total_records == -1
        r.assert_canaries()
    with pytest.raises(pp.PpgError) as e:
        pr.check(rg[0].sh, rg[1].sh)
    assert e.value.code == _lib.PPG_ARG_ERROR
    for r, t in zip(rg, twins):
        r.sh.run()
        t.sh.run()
    assert_twins(rg, twins, "run after the stop")
    rg[0].assert_reference(files["refs"][0])
