"""GPU: `python bench.py --gpus 2` with no launcher around it must start two ranks by itself and print ONE JSON line
for the two-rank job.  On the single-GPU test box both ranks share cuda:0 and the collective runs over gloo
(LINETR_BENCH_ONE_DEVICE / LINETR_BENCH_BACKEND test hooks): the plumbing is what is checked, not the numbers."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _run(extra, expect_failure=False, gpus=2, **more_env):
    env = dict(os.environ, LINETR_BENCH_ONE_DEVICE="1", LINETR_BENCH_BACKEND="gloo", **more_env)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "3", "--warmup", "1",
                        "--settle-s", "0.2", *extra], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert (p.returncode != 0) if expect_failure else (p.returncode == 0), p.stderr[-2000:]
    _run.returncode = p.returncode
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_default_workload_self_launch():
    d = _run(["--pairs", "4", "--full"])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak"
    assert d["config"]["descriptors_per_step"] > 2 * 4 * 2 * 150      # both ranks' descriptors are counted
    assert d["gathered_rows_checked"] is True and d["gather_ms"] > 0 and d["collective_backend"] == "gloo"
    assert d["global_match"]["matches"] > 0
    # pre-flight: both ranks saw each other through the benchmark's own backend; one gather time per rank
    assert d["preflight"]["ranks_seen"] == 2 and d["preflight"]["backend"] == "gloo" and len(d["gather_ms_per_rank"]) == 2


def test_a_bad_gather_fails_loudly():
    """A rank that received rows differing from what their owner packed must end the run with a non-zero exit code and ONE JSON line
    that carries "error" and a null value -- never a normal-looking line (the failure is injected on the last rank)."""
    d = _run(["--pairs", "4", "--full"], expect_failure=True, LINETR_BENCH_INJECT="bad_gather")
    assert d["value"] is None and "gathered_rows_checked" in d["error"] and d["n_gpus"] == 2


def test_one_gpu_plain_run_is_the_headline_alone(tmp_path):
    """Without --full a run prints the headline of its timed steps, writes --dump-outputs, and measures nothing else."""
    d = _run(["--pairs", "4", "--dump-outputs", str(tmp_path)], gpus=1)
    assert d["metric"] == "line_descriptors_per_sec" and d["unit"] == "line-descriptors/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and "bf16" in d["dtype"]
    assert d["value"] == pytest.approx(d["config"]["descriptors_per_step"] / d["ms_per_step"] * 1e3, rel=1e-3)
    assert not {"roofline", "kernels", "oracle_check", "pair_match_ms", "producer", "cfg2", "cfg4", "cfg5", "cpu_baseline"} & set(d)
    assert (tmp_path / "line_desc.npy").exists() and (tmp_path / "cu_n.npy").exists()


def test_cfg4_self_launch():
    d = _run(["--workload", "cfg4", "--pairs-total", "16", "--pairs", "4"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert "recall_vs_homography_rank0" not in d              # a plain run: the recall check is --full's


# ---- more than two ranks: a ring of three (rank r's next rank is not also its previous one), an odd world and uneven shards.  Same
# one-device / gloo plumbing mode, tiny workloads: pre-flight, uneven shards, the slab gather, global matching, the one-JSON-line
# contract.  Three is the most one device takes here: pytest and bench.py's launching process hold the GPU as well, and at most six
# processes may have it open at once.

def test_three_ranks_default_workload():
    d = _run(["--pairs", "2", "--full"], gpus=3)
    assert d["n_gpus"] == 3 and d["scaling"] == "weak" and d["steps"] == 3
    assert d["config"]["descriptors_per_step"] > 3 * 2 * 2 * 150            # all three ranks' descriptors are counted
    assert d["gathered_rows_checked"] is True and d["collective_backend"] == "gloo"
    assert d["preflight"]["ranks_seen"] == 3 and len(d["preflight"]["devices"]) == 3 and len(d["gather_ms_per_rank"]) == 3
    assert d["global_match"]["matches"] > 0 and "rank 1" in d["global_match"]["against"]
    assert "cpu_baseline" not in d               # (the CPU baseline is reported at N = 1 only, as the contract asks)


def test_three_ranks_cfg4_uneven_shards():
    """19 pairs over 3 ranks: rank 0 owns 7 pairs, ranks 1-2 own 6 -- slab heights agreed by the MAX all-reduce, every rank's
    queries matched against candidates other ranks own."""
    d = _run(["--workload", "cfg4", "--pairs-total", "19", "--pairs", "2", "--candidates", "3", "--full"], gpus=3)
    assert d["n_gpus"] == 3 and d["scaling"] == "strong"
    assert d["config"]["pairs_total"] == 19 and d["config"]["collective"] == "all_gather(slab)"
    assert d["config"]["pair_matches_per_step"] == 19 * 3
    assert d["config"]["descriptors_per_step"] > 19 * 2 * 150
    assert d["preflight"]["ranks_seen"] == 3
    assert d["recall_vs_homography_rank0"]["matches"] > 0


def test_three_ranks_a_bad_rank_fails_with_exit_code_3():
    d = _run(["--pairs", "2", "--full"], expect_failure=True, gpus=3, LINETR_BENCH_INJECT="bad_gather")
    assert d["value"] is None and "gathered_rows_checked" in d["error"] and d["n_gpus"] == 3
    assert _run.returncode != 0
