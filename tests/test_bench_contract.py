"""bench.py driver contract on CPU: the config it builds for N ranks gives every rank whole
micro-batches of the configured size (a short DistributedSampler shard would silently shrink the
per-GPU batch at 8 GPUs), and it names the BASELINE.json metric."""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from llmtrain.data.synthetic_tokens import SyntheticTokensDataModule

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    spec = importlib.util.spec_from_file_location("bench_main", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    assert spec.loader is not None
    spec.loader.exec_module(mod)
    return mod


def test_metric_matches_baseline_json() -> None:
    assert _bench().BASELINE_METRIC == json.loads((ROOT / "BASELINE.json").read_text())["metric"]


@pytest.mark.parametrize("world", [1, 2, 4, 8])
@pytest.mark.parametrize("mb,accum", [(128, 1), (16, 2)])
def test_every_rank_gets_full_micro_batches(world: int, mb: int, accum: int) -> None:
    bench = _bench()
    args = argparse.Namespace(model="gpt2-124m", micro_batch=mb, grad_accum=accum, dropout=0.0,
                              path="fused", warmup=1, steps=2, bucket_mb=64.0, device="cuda",
                              grad_reduce_dtype="fp32", deterministic=False)
    cfg = bench.make_config(args, world)
    n = cfg.data.extra["train_sequences"]
    assert n // world >= mb * accum
    # the last rank's shard through the real data module (world hinted via the ddp section);
    # a small vocab keeps the Markov table cheap, the sharding arithmetic is the same
    small = cfg.model_copy(update={
        "ddp": cfg.ddp.model_copy(update={"world_size": world, "rank": world - 1}),
        "model": cfg.model.model_copy(update={"vocab_size": 512, "block_size": 8}),
    })
    dm = SyntheticTokensDataModule()
    dm.setup(small, tokenizer=None)
    batch = next(iter(dm.train_dataloader()))
    assert batch["input_ids"].shape == (mb, 8)


def _run_bench(*argv: str, env_extra: dict[str, str] | None = None) -> subprocess.CompletedProcess:
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2", **(env_extra or {}))
    cmd = [sys.executable, str(ROOT / "bench.py"), "--device", "cpu", "--model", "tiny", "--steps", "2",
           "--warmup", "1", "--micro-batch", "2", *argv]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def _json_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, stdout  # rank 0 prints exactly one line
    return json.loads(lines[0])


@pytest.mark.slow
def test_bench_gpus_2_spawns_two_ranks() -> None:
    """``bench.py --gpus 2`` without a launcher starts 2 ranks itself (gloo on CPU here, RCCL on the
    GPU box) — the number it prints is a real 2-rank job, not one GPU with a warning."""
    proc = _run_bench("--gpus", "2")
    assert proc.returncode == 0, proc.stderr[-3000:]
    res = _json_line(proc.stdout)
    assert res["n_gpus"] == 2 and res["config"]["parallelism"] == "dp2"
    assert res["config"]["backend"] == "gloo"
    assert len(res["per_rank_tokens_per_sec"]) == 2 and len(res["exposed_allreduce_ms"]) == 2
    assert res["config"]["global_batch"] == 2 * 2
    assert res["value"] > 0 and res["steps"] == 2 and res["warmup"] == 1
    # a multi-rank line explains itself: RCCL transports / channels (empty on gloo) and the
    # exposed tail bucket (the tied embedding) with its queue and collective times
    assert set(res["rccl"]) >= {"transport_counts", "channels", "fallback", "env"}
    if res.get("buckets_rank0"):
        assert res["tail_bucket"]["bucket"] == res["buckets_rank0"][-1]["bucket"]
        # (queue / collective times come from GPU events: on the CPU gloo path only the payload)
        assert res["tail_bucket"]["payload_mib"] == res["buckets_rank0"][-1]["payload_mib"]


def test_bench_rejects_world_size_mismatch() -> None:
    proc = _run_bench("--gpus", "2", env_extra={"WORLD_SIZE": "1"})
    assert proc.returncode == 2
    assert "WORLD_SIZE=1" in proc.stderr


def test_dump_sample_is_fixed_sorted_and_bounded() -> None:
    bench = _bench()
    small = bench.sample_positions(1000)
    assert small.tolist() == list(range(1000))  # below the cap: every position
    total = 3 * bench.DUMP_SAMPLE + 7
    pos = bench.sample_positions(total)
    assert pos.shape == (bench.DUMP_SAMPLE,) and pos.dtype == np.int64
    assert (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < total  # sorted, distinct, in range
    assert np.array_equal(pos, bench.sample_positions(total))  # the same sample every time
    # loss + grad_norm + grads + params (float32) + sample_index (float64) stay far below 64 MB
    assert 2 * 4 + bench.DUMP_SAMPLE * (4 + 4 + 8) <= 32 * 2**20 + 8


def test_bench_dump_outputs_and_full(tmp_path: Path) -> None:
    """``--dump-outputs`` writes what the last timed step computed, the same from run to run with
    the same arguments (seeded init, data and sample); ``--full`` is accepted, exits 0 and leaves
    the headline fields of the result line as they are."""
    runs = []
    for name, extra in (("a", ()), ("b", ("--full",))):
        proc = _run_bench("--gpus", "1", "--dump-outputs", str(tmp_path / name), *extra)
        assert proc.returncode == 0, proc.stderr[-3000:]
        res = _json_line(proc.stdout)
        assert res["full"] is bool(extra) and res["steps"] == 2 and res["ms_per_step"] > 0
        arrays = {p.stem: np.load(p) for p in sorted((tmp_path / name).glob("*.npy"))}
        assert set(arrays) == {"loss", "grad_norm", "grads", "params", "sample_index"}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 10**6
        assert all(np.isfinite(a).all() for a in arrays.values())
        assert arrays["grads"].shape == arrays["params"].shape == arrays["sample_index"].shape
        assert arrays["grads"].size > 0 and np.abs(arrays["grads"]).max() > 0
        assert abs(float(arrays["loss"][0]) - res["final_loss"]) <= 1e-4  # the last timed step's loss
        # the norm of the dumped gradients (tiny model: every element is kept) is the dumped norm
        assert np.linalg.norm(arrays["grads"].astype(np.float64)) == pytest.approx(float(arrays["grad_norm"][0]), rel=1e-4)
        runs.append((res, arrays))
    (res_a, a), (res_b, b) = runs
    for key in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config"):
        assert res_a[key] == res_b[key]
    for name in a:  # fp32 on CPU with a fixed thread count: the same sums in the same order
        np.testing.assert_allclose(a[name], b[name], rtol=1e-6, atol=1e-8, err_msg=name)


def test_bench_single_rank_cpu_contract() -> None:
    proc = _run_bench("--gpus", "1")
    assert proc.returncode == 0, proc.stderr[-3000:]
    res = _json_line(proc.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in res
    assert res["n_gpus"] == 1 and res["higher_is_better"] is True and res["scaling"] == "weak"
