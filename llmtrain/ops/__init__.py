"""Fused ops of the MI355X training path.

Each function runs the hand-written gfx950 HIP kernel (``torch.ops.llmtrain_hip.*``) when its
inputs live on a GPU and the plain-PyTorch oracle from :mod:`llmtrain.ops.reference` when they
live on the CPU (unit tests of the fused engine).  There is exactly one GPU implementation per
op and no silent fallback: a GPU tensor with the extension missing raises (``_ext.require``).
The forward / data-gradient GEMMs and their routing live in :mod:`llmtrain.ops.gemm`, the
process-wide kernel policy in :mod:`llmtrain.ops.policy`; both are re-exported here, and callers
(the engine, the A/B scripts under bench/) reach every op through this package.
"""

from __future__ import annotations

import torch

from llmtrain.ops import reference as ref
from llmtrain.ops._ext import hip_ops
from llmtrain.ops.gemm import head_dx, head_logits, linear_dx, linear_dx_gd, linear_dx_gelu_bwd, linear_fwd
from llmtrain.ops.gemm import linear_fwd_gelu, linear_fwd_gelu_gd, wgrad_accum
from llmtrain.ops.gemm import linear_dx_attn  # noqa: F401 - public, though __all__ never listed it
from llmtrain.ops.policy import _POLICY  # noqa: F401 - the flags themselves, for tests that read them
from llmtrain.ops.policy import kernel_policy, policy_state, restore_policy, set_deterministic, single_stream

__all__ = [
    "adamw_flat", "add_layernorm_fwd", "attn_bwd", "attn_fwd", "attn_key_masks", "clip_coef", "colsum_accum",
    "cross_entropy_fwd_bwd", "embedding_bwd", "embedding_fwd", "gelu_bwd", "gelu_fwd", "head_dx", "head_logits", "hip_ops",
    "kernel_policy", "layernorm_bwd", "linear_dx", "linear_dx_gd", "linear_dx_gelu_bwd", "linear_fwd", "linear_fwd_gelu",
    "linear_fwd_gelu_gd", "ln_param_reduce", "policy_state", "restore_policy", "scale", "set_deterministic", "single_stream",
    "sumsq", "wgrad_accum",
]


def _on_gpu(t: torch.Tensor) -> bool:
    return t.device.type == "cuda"


def add_layernorm_fwd(x, delta, weight, bias, eps: float, out_dtype: torch.dtype, dropout=(0.0, 0)):
    """``xs = x + dropout(delta)``, ``y = LN(xs)``; ``dropout = (p, site_seed)`` masks the branch."""
    p, seed = dropout
    if _on_gpu(x):
        xs, y, mean, rstd = hip_ops().add_layernorm_fwd(x, delta, weight, bias, eps, out_dtype, p, seed)
        return (x if delta is None else xs), y, mean, rstd
    return ref.add_layernorm_fwd(x, delta, weight, bias, eps, out_dtype, p, seed)


def layernorm_bwd(
    dy, xs, mean, rstd, weight, dresid, dweight, dbias, dy_scale=None, *, want_lowp=False, dproj_bias=None,
    dropout=(0.0, 0), defer_params=False, grad_dtype=torch.float32,
):
    """LayerNorm backward with two optional fusions for the producer of the normalised input:

    * ``want_lowp`` also returns ``dx`` in ``dy``'s dtype (the GEMM operand of the projection
      whose output was added to the residual stream), and
    * ``dproj_bias`` (fp32 ``[d]``) accumulates ``colsum(dx)`` — that projection's bias grad;

    both see the branch's dropout mask ``dropout = (p, site_seed)`` (the residual-stream ``dx``
    itself does not).  Returns ``(dx, dx_lowp | None)``.  ``grad_dtype``: storage of the
    residual-gradient stream (``dresid`` in, ``dx`` out) — fp32, or bf16 for the engine's bf16
    gradient stream, where ``dx_lowp`` without dropout IS ``dx`` (one write, not two).

    ``defer_params``: dgamma / dbeta are NOT accumulated yet; a third value ``parts`` (partial rows,
    ``[2, rows, d]``) goes to :func:`ln_param_reduce`, which reduces two LayerNorms in one launch.
    """
    p, seed = dropout
    glp = grad_dtype == torch.bfloat16
    if defer_params:
        if dproj_bias is not None:
            raise ValueError("layernorm_bwd: defer_params takes no dproj_bias")
        if _on_gpu(dy):
            dx, dx_lp, parts = hip_ops().layernorm_bwd_deferred(
                dy, xs, mean, rstd, weight, dresid, dweight, dbias, dy_scale, want_lowp, p, seed, glp
            )
            return dx, (dx_lp if want_lowp else None), parts
        pw, pb = torch.zeros_like(dweight), torch.zeros_like(dbias)
        dx = ref.layernorm_bwd(dy, xs, mean, rstd, weight, dresid, pw, pb, dy_scale, grad_dtype)
        branch = ref._apply_dropout(dx.float(), p, seed)
        return dx, (branch.to(dy.dtype) if want_lowp else None), torch.stack([pw, pb])[:, None, :]
    if _on_gpu(dy):
        dx, dx_lp = hip_ops().layernorm_bwd(
            dy, xs, mean, rstd, weight, dresid, dweight, dbias, dy_scale, want_lowp, dproj_bias, p, seed, glp
        )
        return dx, (dx_lp if want_lowp else None)
    dx = ref.layernorm_bwd(dy, xs, mean, rstd, weight, dresid, dweight, dbias, dy_scale, grad_dtype)
    branch = ref._apply_dropout(dx.float(), p, seed)
    if dproj_bias is not None:
        ref.colsum_accum(branch, dproj_bias)
    return dx, (branch.to(dy.dtype) if want_lowp else None)


def ln_param_reduce(parts: list, dst: list) -> None:
    """``dst[2i] += rows of parts[i][0]``, ``dst[2i + 1] += rows of parts[i][1]`` for the deferred
    LayerNorm backwards of :func:`layernorm_bwd` — one fixed-order launch on GPU for LayerNorms with
    equal partial-row counts (a block's ln_2 and ln_1), separate launches otherwise."""
    if not parts:
        return
    if parts[0].device.type != "cuda":
        for i, pr in enumerate(parts):
            dst[2 * i] += pr[0].sum(0)
            dst[2 * i + 1] += pr[1].sum(0)
        return
    if len({tuple(pr.shape) for pr in parts}) == 1:
        hip_ops().ln_param_reduce(list(parts), list(dst))
        return
    for i, pr in enumerate(parts):
        hip_ops().ln_param_reduce([pr], [dst[2 * i], dst[2 * i + 1]])


def cross_entropy_fwd_bwd(logits, labels, vocab: int, row_weight):
    if _on_gpu(logits):
        return hip_ops().cross_entropy_fwd_bwd(logits, labels, vocab, row_weight)
    return ref.cross_entropy_fwd_bwd(logits, labels, vocab, row_weight)


def scale(x, s):
    """``x * s`` for a 0-/1-element fp32 device scalar ``s`` (an autograd upstream gradient):
    one HIP pass with fp32 math and a single rounding on GPU, no host sync."""
    if _on_gpu(x) and x.is_contiguous() and x.numel() % 8 == 0 and x.dtype in (torch.bfloat16, torch.float32):
        return hip_ops().scale(x, s.reshape(1).float())
    return (x.float() * s.float()).to(x.dtype)


def gelu_fwd(u):
    if _on_gpu(u):
        return hip_ops().gelu_fwd(u)
    return ref.gelu_fwd(u)


def gelu_bwd(dg, u, dbias):
    if _on_gpu(dg):
        return hip_ops().gelu_bwd(dg, u, dbias)
    return ref.gelu_bwd(dg, u, dbias)


def colsum_accum(dy, out) -> None:
    if _on_gpu(dy):
        hip_ops().colsum_accum(dy, out)
    else:
        ref.colsum_accum(dy, out)


def embedding_fwd(ids, wte, wpe, dropout=(0.0, 0), out_dtype=torch.float32):
    """Token + position embedding (+ dropout), ``out_dtype`` = the residual stream's storage."""
    p, seed = dropout
    if _on_gpu(ids):
        return hip_ops().embedding_fwd(ids, wte, wpe, p, seed, out_dtype == torch.bfloat16)
    return ref.embedding_fwd(ids, wte, wpe, p, seed, out_dtype)


def embedding_bwd(dx, ids, dwte, dwpe, dropout=(0.0, 0)) -> None:
    """Token / position embedding gradients from the residual-stream gradient ``dx`` (fp32 or
    bf16: the scatter kernels read either stream as is)."""
    p, seed = dropout
    if _on_gpu(dx):
        hip_ops().embedding_bwd(dx.contiguous(), ids, dwte, dwpe, p, seed)
    else:
        ref.embedding_bwd(dx, ids, dwte, dwpe, p, seed)


def attn_key_masks(mask: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Device forms of a ``[B, T]`` key-padding mask for the attention kernels: ``key_bits``
    ``[B, ceil(T/64)]`` int64 (bit j of word w = key 64w + j is valid; the forward reads one word
    per 64-key tile) and ``key_valid`` ``[B, T]`` uint8 (the backward reads its lane's key)."""
    bsz, seqlen = mask.shape
    valid = mask.bool()
    words = -(-seqlen // 64)
    padded = torch.zeros(bsz, words * 64, dtype=torch.int64, device=mask.device)
    padded[:, :seqlen] = valid.to(torch.int64)
    shifts = torch.arange(64, dtype=torch.int64, device=mask.device)
    bits = (padded.view(bsz, words, 64) << shifts).sum(dim=-1)  # wraps into bit 63 as int64
    return bits.contiguous(), valid.to(torch.uint8).contiguous()


def attn_fwd(qkv, bsz: int, seqlen: int, n_heads: int, dropout=(0.0, 0), key_masks=None):
    """Causal flash attention over packed ``qkv``; ``key_masks`` = :func:`attn_key_masks` of the
    batch's key-padding mask (None = every key valid)."""
    p, seed = dropout
    if _on_gpu(qkv):
        bits = None if key_masks is None else key_masks[0]
        return hip_ops().attn_fwd(qkv, bsz, seqlen, n_heads, p, seed, bits)
    valid = None if key_masks is None else key_masks[1]
    return ref.attn_fwd(qkv, bsz, seqlen, n_heads, p, seed, valid)


def attn_bwd(
    dout, qkv, out, lse, bsz: int, seqlen: int, n_heads: int, dropout=(0.0, 0), qkv_bias_grad=None, delta=None,
    key_masks=None,
):
    """Attention backward -> packed ``dqkv``; ``qkv_bias_grad`` (fp32 ``[3d]``), when given,
    accumulates ``colsum(dqkv)`` (fused into the kernels on GPU).  ``delta`` (GPU): the row
    constants ``rowsum(dO * O)`` already computed by :func:`linear_dx_attn`, which then also added
    the V part of ``qkv_bias_grad`` when there is no dropout; the delta pass is skipped."""
    p, seed = dropout
    valid = None if key_masks is None else key_masks[1]
    if _on_gpu(dout):
        return hip_ops().attn_bwd(dout, qkv, out, lse, bsz, seqlen, n_heads, p, seed, qkv_bias_grad, delta, valid)
    dqkv = ref.attn_bwd(dout, qkv, out, lse, bsz, seqlen, n_heads, p, seed, valid)
    if qkv_bias_grad is not None:
        ref.colsum_accum(dqkv, qkv_bias_grad)
    return dqkv


def sumsq(x):
    if _on_gpu(x):
        return hip_ops().sumsq(x)
    return ref.sumsq(x)


def clip_coef(sumsq_t, max_norm: float):
    """``[norm, coef]`` of the gradient clip from the global squared norm (fp32, one element):
    ``norm = sqrt(sumsq)``, ``coef = min(1, max_norm / (norm + 1e-6))`` (``clip_grad_norm_``), and
    ``coef = NaN`` when the norm is NaN/Inf, which makes :func:`adamw_flat` skip the step."""
    if _on_gpu(sumsq_t):
        return hip_ops().clip_coef(sumsq_t.reshape(1).float(), float(max_norm))
    return ref.clip_coef(sumsq_t, max_norm)


def adamw_flat(
    param, grad, exp_avg, exp_avg_sq, shadow, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale, dyn=None,
    skipped=None,
):
    """``dyn`` (GPU only): device ``[decay, step_size, bc2_sqrt]`` read by the kernel instead of the
    values formed from ``lr``/``step`` — a hipGraph-captured step stages them before each replay.
    A non-finite ``grad_scale`` skips the update (nothing is written); ``skipped`` (int32 ``[2]``,
    optional) then counts it: ``[total, consecutive]``, the second reset by an applied step."""
    if _on_gpu(param):
        hip_ops().adamw_flat(
            param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, weight_decay, step, grad_scale, dyn,
            skipped,
        )
        return
    if dyn is not None:
        raise ValueError("adamw_flat: device-staged scalars exist only on the GPU path")
    ref.adamw_flat(
        param, grad, exp_avg, exp_avg_sq, shadow, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
        weight_decay=weight_decay, step=step, grad_scale=grad_scale, skipped=skipped,
    )
