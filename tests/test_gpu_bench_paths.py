"""bench.py's multi-rank paths, rehearsed on the one GPU of the box (every rank on cuda:0,
PPG_BENCH_ONE_DEVICE=1) with gloo for torch.distributed and the library's host transport for the
count all-gather: the driver's `python bench.py --gpus N` (the bench launches its own ranks) and
the paired configs[4] path on two ranks, which must find exactly the single-rank pair count."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_raw(args, ranks=1, timeout=240, env_extra=None):
    env = dict(os.environ, PPG_BENCH_ONE_DEVICE="1", PPG_DIST_BACKEND="gloo", **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    if ranks > 1 and "--gpus" not in args:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
               "--master-addr", "127.0.0.1", "--master-port", str(29400 + os.getpid() % 500)] + cmd[1:]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def _bench(args, ranks=1, timeout=240):
    r = _bench_raw(args, ranks, timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


SMALL = ["--seg-records", "40000", "--repeats", "6", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
         "--no-ingest"]


def test_bench_launches_its_own_ranks_and_gathers_in_the_abi():
    one = _bench(SMALL)
    two = _bench(SMALL + ["--gpus", "2"])
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["scaling"] == "strong" and two["config"]["workload"].startswith("configs[3]")
    assert two["config"]["records"] == one["config"]["records"]          # the bench asserts the exact count too
    assert two["communicator"]["world_size"] == 2
    assert "ppg_shard_gather_counts" in two["communicator"]["count_gather"]


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline line without the --full legs, and --dump-outputs writes what
    its last timed step computed: float arrays under 64 MB, the per-chunk records summing to the
    line's record count, the sampled chunks' descriptors one row per record."""
    import numpy as np
    d = tmp_path / "out"
    args = [a for a in SMALL if not a.startswith("--no-")]
    line = _bench(args + ["--dump-outputs", str(d)])
    assert not {"cpu_baseline", "ingest", "enumerate", "decompress_chunk"} & set(line)
    assert line["steps"] == 1 and line["ms_per_step"] > 0
    files = sorted(d.glob("*.npy"))
    arrs = {f.stem: np.load(f) for f in files}
    assert sum(f.stat().st_size for f in files) < 64e6
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    rec = arrs["chunk_records"]
    assert int(rec.sum()) == line["config"]["records"] and not arrs["chunk_status"].any()
    pick = arrs["sample_chunks"].astype(int)
    assert pick[0] == 0 and pick[-1] == rec.size - 1
    for k in pick:
        assert arrs[f"descriptors_chunk{k}"].shape == (int(rec[k]), 4)
        assert arrs[f"text_chunk{k}"].size == min(int(arrs["chunk_produced"][k]), 2 * (384 << 10))
    assert arrs["text_chunk0"][0] == ord("@") and arrs[f"text_chunk{pick[-1]}"][-1] == ord("\n")


def test_bench_paired_two_ranks_same_pairs():
    args = ["--paired", "--seg-records", "100000", "--paired-repeats", "3", "--steps", "1", "--warmup", "1"]
    one = _bench(args)
    two = _bench(args, ranks=2)
    assert one["config"]["pairs"] == two["config"]["pairs"] == 300000
    assert two["n_gpus"] == 2 and two["config"]["pair_check"].startswith("ppg_pairs_check: keys to pair owners")


def test_bench_rccl_glue_world1():
    """The bench's N > 1 glue under nccl = RCCL, at world size 1 (one GPU on this box): the process
    group, rank 0's ppg_comm_unique_id broadcast, ppg_comm_init, and ppg_shard_gather_counts over
    RCCL every step."""
    env = dict(os.environ, PPG_BENCH_FORCE_DIST="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PPG_BENCH_ONE_DEVICE", "PPG_DIST_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", str(29000 + os.getpid() % 400),
           os.path.join(ROOT, "bench.py")] + SMALL
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    c = line["communicator"]
    assert c["backend"] == "nccl" and c["world_size"] == 1
    assert c["count_gather"] == "libppgpu ppg_shard_gather_counts over RCCL (ncclAllGather)"
    one = _bench(SMALL)
    assert line["config"]["records"] == one["config"]["records"]
    assert len(line["setup_s"]["per_rank"]) == 1


def test_bench_shares_the_input_between_ranks():
    """N > 1: local rank 0 builds the member once and the other ranks memory-map it from /dev/shm
    (VERDICT r02 next #2); the shared copy is gone after the run."""
    import glob
    before = set(glob.glob("/dev/shm/ppg_bench_*"))
    two = _bench(SMALL + ["--gpus", "2"])
    st = two["setup_s"]
    assert st["input_how"].startswith("built (shared via /dev/shm/")
    assert len(st["per_rank"]) == 2
    assert set(glob.glob("/dev/shm/ppg_bench_*")) == before


def test_bench_world8_rehearsal():
    """configs[3]'s world size on the one-GPU box: `bench.py --gpus 8` starts
    eight ranks (all on cuda:0, gloo + the library's host transport for the count gather) and runs
    the whole N = 8 path -- ppg_partition's ranges, the per-rank auto split, gather_pairs, the count
    gather, max-over-ranks timing -- to the single-rank record count (the bench asserts it)."""
    one = _bench(SMALL + ["--repeats", "16"])
    eight = _bench(SMALL + ["--repeats", "16", "--gpus", "8"], timeout=420)
    assert eight["n_gpus"] == 8 and eight["scaling"] == "strong"
    assert eight["config"]["workload"].startswith("configs[3]")
    assert eight["config"]["records"] == one["config"]["records"]
    assert eight["communicator"]["world_size"] == 8
    assert "ppg_shard_gather_counts" in eight["communicator"]["count_gather"]
    assert len(eight["setup_s"]["per_rank"]) == 8


@pytest.mark.parametrize("world,fail", [(2, "set_split@1"), (8, "shard@5"), (8, "input@0")])
def test_setup_failure_fails_every_rank_loudly(world, fail):
    """one rank's setup failure -- a real library error from ppg_shard_set_split
    (side points past their chunks), or an injected one at the shard / input stage (local rank 0's
    build: the waiting ranks read its failure file) -- is agreed before the next collective: every
    rank exits non-zero naming the failing rank, promptly, instead of stranding its peers in gloo /
    RCCL (PPG_BENCH_FAIL, a test hook)."""
    import time
    stage, bad = fail.split("@")
    t = time.time()
    r = _bench_raw(SMALL + ["--gpus", str(world)], timeout=300, env_extra={"PPG_BENCH_FAIL": fail})
    assert r.returncode != 0, r.stdout[-2000:]
    agreed = "shard" if stage == "set_split" else stage
    # input@0: local rank 0 could not build the member, so every rank lacks its input
    want = (f"setup failed at 'input' on rank(s) {list(range(world))} of {world}; rank 0: RuntimeError: injected"
            if fail == "input@0" else f"setup failed at '{agreed}' on rank(s) [{bad}] of {world}")
    import re
    said = set(re.findall(r"\[bench\] rank (\d+): " + re.escape(want), r.stderr))
    assert said == {str(i) for i in range(world)}, r.stderr[-3000:]   # every rank said so
    if stage == "set_split":
        assert "ppg_shard_set_split" in r.stderr or "ARG_ERROR" in r.stderr or "PpgError" in r.stderr, r.stderr[-3000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert time.time() - t < 240


def test_bench_world8_rehearsal_end_to_end_leg():
    """The N > 1 line's per-rank evidence and end-to-end leg, world 8 on the one
    GPU: every rank's own step / inflate times, batches and records; every rank streams its range of
    the member from a file through ppg_file_decompress_all, max-over-ranks seconds, records exact."""
    args = [a for a in SMALL if a != "--no-ingest"] + ["--full", "--repeats", "16", "--gpus", "8",
                                                       "--ingest-piece-gib", "0.25"]
    eight = _bench(args, timeout=420)
    pr = eight["per_rank"]["ranks"]
    assert [p["rank"] for p in pr] == list(range(8))
    assert sum(p["records"] for p in pr) == eight["config"]["records"]
    assert all(p["batches"] >= 1 and p["inflate_ms_per_step"] > 0 for p in pr)
    ing = eight["ingest"]
    assert "error" not in ing, ing
    assert ing["records"] == eight["config"]["records"] and len(ing["per_rank"]) == 8
    assert abs(ing["seconds_max_over_ranks"] - max(p["seconds"] for p in ing["per_rank"])) < 1e-3
