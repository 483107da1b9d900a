"""Process-wide kernel policy: the fast (atomic) kernels or one of the deterministic schedules.

Read by the GEMM router (:mod:`llmtrain.ops.gemm`) and the engine; re-exported by
:mod:`llmtrain.ops`."""

from __future__ import annotations

import contextlib
import os
from collections.abc import Iterator

import torch

from llmtrain.ops import _ext

_POLICY = {"gemm_all_ours": False, "single_stream": False, "deterministic": False}

# How run.deterministic keeps the step bitwise reproducible (LLMTRAIN_DET_SCHEDULE overrides):
#  * "serial": the weight-gradient GEMMs run on the main stream (no side stream), the LM-head logits
#    and dX GEMMs on our fixed-order kernel (the logits' tuned library solution is a Stream-K kernel
#    and the one library GEMM of the configuration whose bitwise guarantee failed once,
#    profiles/r5/det/; round 6 took it off the library), and the other forward / dX GEMMs on our
#    kernel below the size cap, on hipBLASLt's tuned solutions above it.  Evidence for the library
#    GEMMs that remain: bitwise-equal repeats at micro-batch 32 of GPT-2 124M and GPT-2 XL (the
#    XL preset; 3 whole runs x 20 steps) (bench/determinism_probe.py, profiles/r4/det/,
#    profiles/r5/det/) and 800 bitwise repeats of the Stream-K solutions of the forward
#    projections, alone and beside a concurrent stream (bench/sk_repeat.py); other shapes are
#    unpinned, and each library GEMM of a serial run is named once in the log (gemm._det_library).
#  * "ours": every forward / dX GEMM on the hand-written kernel (csrc/gemm_fused.hip), side stream
#    kept; slower because that kernel trails hipBLASLt at 128K rows (docs/round4.md).
DET_SCHEDULES = ("serial", "ours")


def set_deterministic(on: bool, schedule: str | None = None) -> bool:
    """Process-wide deterministic mode of the HIP kernels (``run.deterministic`` on GPU): the
    split-K weight-gradient GEMM and the embedding token gradient switch from float atomics to
    fixed-order reductions (every other reduction is fixed-order always), and the GEMM schedule
    becomes one of :data:`DET_SCHEDULES` — hipBLASLt's Stream-K solutions combine partial tiles in
    an order that depends on which workgroups finish first, which the weight-gradient side stream
    perturbs (bench/determinism_probe.py --runs, docs/round3.md).  Returns the previous setting.
    The CPU reference ops are deterministic anyway.  Prefer :func:`kernel_policy`, which restores
    the previous policy on exit (the Trainer scopes its steps with it)."""
    if on:
        schedule = schedule or os.environ.get("LLMTRAIN_DET_SCHEDULE", "serial")
        if schedule not in DET_SCHEDULES:
            raise ValueError(f"deterministic schedule must be one of {DET_SCHEDULES}, not {schedule!r}")
    _POLICY["gemm_all_ours"] = bool(on) and schedule == "ours"
    _POLICY["single_stream"] = bool(on) and schedule == "serial"
    _POLICY["deterministic"] = bool(on)
    if not _ext.load():
        return False
    prev = bool(torch.ops.llmtrain_hip.get_deterministic())
    torch.ops.llmtrain_hip.set_deterministic(bool(on))
    return prev


def policy_state() -> tuple[dict[str, bool], bool]:
    """Snapshot of the process-wide kernel policy: the Python routing flags and the C++
    deterministic flag (False when the extension is not loaded)."""
    cpp = bool(torch.ops.llmtrain_hip.get_deterministic()) if _ext.is_loaded() else False
    return dict(_POLICY), cpp


def restore_policy(state: tuple[dict[str, bool], bool]) -> None:
    """Undo every policy change since :func:`policy_state` returned ``state``."""
    flags, cpp = state
    _POLICY.update(flags)
    if _ext.is_loaded():
        torch.ops.llmtrain_hip.set_deterministic(bool(cpp))


@contextlib.contextmanager
def kernel_policy(deterministic: bool, schedule: str | None = None) -> Iterator[None]:
    """Run a block under ``run.deterministic = deterministic`` and restore the previous policy on
    exit, so one Trainer's setting never leaks into the next one in the same process (a test
    suite, a notebook)."""
    prev = policy_state()
    set_deterministic(deterministic, schedule)
    try:
        yield
    finally:
        restore_policy(prev)


def single_stream() -> bool:
    """True when the deterministic "serial" schedule forbids the weight-gradient side stream."""
    return _POLICY["single_stream"]


def gemm_policy() -> str:
    """The forward / dX GEMM schedule in force: ``"fast"``, or the deterministic ``"serial"`` / ``"ours"``."""
    if not _POLICY["deterministic"]:
        return "fast"
    return "ours" if _POLICY["gemm_all_ours"] else "serial"
