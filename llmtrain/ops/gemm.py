"""Forward and data-gradient GEMMs: which kernel each one runs on, and running it.

Every such GEMM of the step is a :class:`GemmSite`.  :func:`route` decides from plain values
(shape, placement, kernel policy, knobs) whether a site's call takes the hand-written fused-epilogue
kernel (csrc/gemm_fused.hip) or the library (hipBLASLt through ``torch.mm`` / ``torch.addmm``);
:func:`run_gemm` launches the kernel over :func:`row_chunks`; the public functions build the
route's inputs from their tensors and compose the library form of their epilogue.  CPU tensors
always take the library branch, which is then the plain-PyTorch oracle of the op.
"""

from __future__ import annotations

import logging
import os
import warnings
from dataclasses import dataclass
from enum import IntEnum
from typing import NamedTuple

import torch

from llmtrain.ops import reference as ref
from llmtrain.ops._ext import hip_ops
from llmtrain.ops.policy import gemm_policy

class Epilogue(IntEnum):
    """Epilogues of ``gemm_fused`` (the values of csrc/gemm_fused.hip's header comment)."""

    BIAS = 0  # C = acc + bias (bias optional)
    BIAS_GELU = 1  # U = acc + bias, C2 = gelu(U)
    DGELU = 2  # C = acc * gelu'(U), dbias += colsum(C)
    ATTN_DELTA = 3  # C = acc, delta = per-head rowsum(C * U), dbias += colsum(C)
    BIAS_GELU_GD = 4  # C = gelu'(u), C2 = gelu(u) of u = acc + bias
    MUL = 5  # C = acc * U (U = the stored gelu'(u)), dbias += colsum(C)


@dataclass(frozen=True)
class GemmSite:
    """One forward / dX GEMM call site: what the sites differ in, for :func:`route` and
    :func:`run_gemm`."""

    tag: str  # name in warnings; for size-routed sites also the LLMTRAIN_FGEMM_ANY / _NEVER entry
    lib_tag: str  # name in the serial schedule's once-per-shape library log
    b_kn: bool  # B is [K, N] (dX = dY @ W) rather than an nn.Linear weight [N, K]
    epilogue: Epilogue
    size_routed: bool = True  # the A-size cap and the FGEMM_NEVER / FGEMM_ANY_SIZE knobs apply
    unit_stride: bool = False  # A's inner stride must be 1 (the size-routed sites' A always is)
    warn_always: bool = False  # an unusable shape warns in every deterministic schedule, not only "ours"
    det_only: bool = False  # our kernel only in deterministic mode (the LM head)
    tuned_bias: bool = False  # a tuned library bias-GEMM entry keeps the fast path on the library
    max_rows: int | None = None  # fixed rows-per-launch cap
    shape_warning: str = "GEMM {tag} K={k} N={n} (needs K % 64 == 0, K >= 256, N % 8 == 0)"
    align_warning: str = "GEMM {tag} with an operand not 16-byte aligned"


# the sites the A-size cap does not route: taken at any size (row-chunked where needed)
_ANY = {"size_routed": False, "unit_stride": True, "warn_always": True}
# rows per launch of the LM-head GEMMs on the hand-written kernel: its buffer descriptors take
# 32-bit byte offsets, and [rows, 50304] bf16 must stay below 2 GiB
_HEAD = {**_ANY, "det_only": True, "max_rows": 16384}

FWD = GemmSite("fwd", "fwd", False, Epilogue.BIAS, tuned_bias=True)
FWD_GELU = GemmSite("fwd_gelu", "fc fwd", False, Epilogue.BIAS_GELU)
FWD_GELU_GD = GemmSite("fc fwd + GELU'", "fc fwd", False, Epilogue.BIAS_GELU_GD, **_ANY)
DX = GemmSite("dx", "dX", True, Epilogue.BIAS)
DX_GELU = GemmSite("dx_gelu", "MLP-projection dX", True, Epilogue.DGELU)
DX_GD = GemmSite("MLP-projection dX * gelu'", "MLP-projection dX", True, Epilogue.MUL, **_ANY)
# preconditions of its own (head dim 64, seq_len | M, 64 | N) and a fallback site: see route()
DX_ATTN = GemmSite("dx_attn", "attention out-projection dX", True, Epilogue.ATTN_DELTA)
HEAD_LOGITS = GemmSite("LM-head logits", "LM-head logits", False, Epilogue.BIAS, **_HEAD)
HEAD_DX = GemmSite("LM-head dX", "LM-head dX", True, Epilogue.BIAS, **_HEAD,
                   shape_warning="LM-head dX K={k} N={n}", align_warning="LM-head dX K={k} N={n}")

# Where the fused GEMM pays in a real step (same-box A/B, docs/performance.md): GPT-2 XL micro-batch
# 16 (A operands 52 MB) +3 %; GPT-2 124M at 64K-128K tokens per step (A 100-600 MB) -1.4 % although
# each GEMM alone is ahead of hipBLASLt at 64K: its persistent, statically scheduled 160 KiB-LDS
# workgroups start late on CUs still draining the previous kernel.  Above this many A bytes the
# engine stays on hipBLASLt.
FGEMM_MAX_A_BYTES = int(float(os.environ.get("LLMTRAIN_FGEMM_MAX_A_MB", "64")) * 2**20)  # A/B knob
# Ops that stay on the library GEMM at every size (outside deterministic mode's "ours" schedule)
FGEMM_NEVER = frozenset(t for t in os.environ.get("LLMTRAIN_FGEMM_NEVER", "").split(",") if t)
# Ops that take the fused GEMM at any A size.  dx_gelu: the MLP-projection dX with GELU backward +
# fc-bias grad in the epilogue replaces a hipBLASLt GEMM plus a full [M, 4d] read-modify pass, and
# wins in the whole 124M step (same-box, micro-batch 128: +0.9 %, 994.9k/995.5k vs 985.8k/986.8k
# tok/s).  dx_attn: the attention out-projection dX with the backward's delta rows and the V-bias
# column sums in the epilogue (deletes the delta pass; same-box mb 128: 1,076.3k vs 1,074.5k tok/s,
# profiles/r3/ab_dx_attn_any_size_mb128.txt).  Adding the plain dX GEMMs (-0.4 %) or the forward
# GEMMs (-1.6 %) at this size loses: hipBLASLt's 256x256 kernels run 1.1-1.3 PF on these shapes
# against 0.86-1.14 PF for ours (profiles/r3/fgemm_wide_v2_ab_m131k.log).  With non-temporal output
# stores at this size, fc + bias + GELU on ours beats hipBLASLt + the GELU pass alone (0.725 vs
# 0.808 ms) but runs 0.86 ms per call inside the step and the step loses 0.4-1.0 % (qkv forward
# too: -1.2 %; profiles/r3/nt/), so those stay on hipBLASLt.
FGEMM_ANY_SIZE = frozenset(os.environ.get("LLMTRAIN_FGEMM_ANY", "dx_gelu,dx_attn").split(","))  # A/B knob


class Route(NamedTuple):
    ours: bool  # the hand-written kernel (else the library)
    warning: str | None  # a deterministic promise this decision breaks
    site: GemmSite  # the site to run: DX for a DX_ATTN call whose heads are not 64 wide


def route(
    site: GemmSite, *, m: int, k: int, n: int, a_bytes: int, aligned: bool, unit_stride: bool, has_bias: bool,
    policy: str, tuned_bias: bool, seq_len: int = 0, head_dim: int = 64, allow_ours: bool = True,
) -> Route:
    """Which GEMM a call of ``site`` runs on.  ``aligned``: every operand handed in starts on 16
    bytes; ``policy``: :func:`llmtrain.ops.policy.gemm_policy`; ``tuned_bias``: the shipped
    TunableOp table holds this bias-GEMM shape; ``allow_ours`` False (LLMTRAIN_FUSED_GEMM=0, or
    operands that are not bf16 on a GPU) keeps every site on the library.

    A deterministic run promises the fixed-order kernel for every GEMM in the "ours" schedule and
    for the ``warn_always`` sites in "serial" too; a shape or placement outside what the kernel
    takes (K % 64 == 0, K >= 256, N % 8 == 0, 16-byte aligned operands) runs on hipBLASLt instead,
    whose split / Stream-K solutions may combine partial sums in completion order, and the route
    says so in ``warning`` instead of failing silently."""
    if site is DX_ATTN and head_dim != 64:
        # the epilogue's per-head row dots are 64 columns wide: a plain dX GEMM (fixed-order kernel
        # where the shape allows, e.g. the reference presets' d = 256 / 384); attn_bwd forms delta itself
        site = DX
    if not allow_ours or (site.det_only and policy == "fast") or (site is DX_ATTN and (m % seq_len or n % 64)):
        return Route(False, None, site)
    broken = policy == "ours" or (site.warn_always and policy != "fast")
    if not (k % 64 == 0 and k >= 256 and n % 8 == 0):
        return Route(False, site.shape_warning.format(tag=site.tag, k=k, n=n) if broken else None, site)
    capped = (a_bytes > FGEMM_MAX_A_BYTES and site.tag not in FGEMM_ANY_SIZE) or site.tag in FGEMM_NEVER
    if site.size_routed and policy != "ours" and capped:
        return Route(False, None, site)
    if not aligned or (site.unit_stride and not unit_stride):
        return Route(False, site.align_warning.format(tag=site.tag, k=k, n=n) if broken else None, site)
    # a tuned library entry was timed against our kernel when the table was made (_library_tuned_bias_gemm)
    return Route(not (site.tuned_bias and tuned_bias and has_bias and policy == "fast"), None, site)


# The hand-written GEMM's buffer descriptors and tile offsets are 32-bit byte offsets: every [M, K]
# operand and [M, N] output must stay below 2 GiB (the binding refuses larger ones).  Larger GEMMs run
# as row chunks (GPT-2 124M at micro-batch >= ~342, XL's d_ff = 6400 past ~168K rows), each chunk a
# whole number of sequences for the attention-delta epilogue.
OFFSET_LIMIT = 2**31


def row_chunks(m, k, n, epilogue, seq_len=0, *, offset_limit=OFFSET_LIMIT, max_rows=None) -> list[tuple[int, int]]:
    """Row ranges ``[r0, r1)`` of an ``[m, k] x [k, n]`` GEMM small enough for the kernel's 32-bit
    offsets (and a site's ``max_rows``); one ``(0, m)`` range where the whole GEMM fits."""
    align = 256 * seq_len if epilogue == Epilogue.ATTN_DELTA else 256
    rows = max(align, (offset_limit - 1) // (2 * max(k, n)) // align * align)
    if max_rows is not None:
        rows = min(rows, max_rows)
    if m <= rows:
        return [(0, m)]
    return [(r0, min(m, r0 + rows)) for r0 in range(0, m, rows)]


def run_gemm(site: GemmSite, a, b, bias=None, u=None, dbias=None, *, seq_len=0, out=None, offset_limit=OFFSET_LIMIT):
    """``gemm_fused`` of ``site`` over :func:`row_chunks` -> ``(C, C2 | delta | None)``.  A GEMM
    that fits is one launch.  Chunks of the plain epilogue are written in place into one ``[M, N]``
    output (``out``, else a new tensor); the other epilogues' chunk outputs are concatenated
    (``dbias`` accumulates across the launches)."""
    fused = hip_ops().gemm_fused
    m, k = a.shape
    n = b.shape[1] if site.b_kn else b.shape[0]
    epi = int(site.epilogue)
    chunks = row_chunks(m, k, n, site.epilogue, seq_len, offset_limit=offset_limit, max_rows=site.max_rows)
    if len(chunks) == 1:
        return tuple(fused(a, b, site.b_kn, epi, bias, u, dbias, seq_len, out))
    if site.epilogue == Epilogue.BIAS:
        out = torch.empty(m, n, dtype=a.dtype, device=a.device) if out is None else out
        for r0, r1 in chunks:
            fused(a[r0:r1], b, site.b_kn, epi, bias, None, None, seq_len, out[r0:r1])
        return out, None
    parts = [fused(a[r0:r1], b, site.b_kn, epi, bias, None if u is None else u[r0:r1], dbias, seq_len)
             for r0, r1 in chunks]
    return torch.cat([p[0] for p in parts]), None if parts[0][1] is None else torch.cat([p[1] for p in parts])


_WARNED: set[str] = set()


def _warn_once(what: str) -> None:
    if what not in _WARNED:
        _WARNED.add(what)
        warnings.warn(
            f"run.deterministic: {what} cannot take the fixed-order GEMM kernel and runs on hipBLASLt "
            "(bitwise run-to-run reproducibility of this GEMM is not guaranteed)", RuntimeWarning, stacklevel=4,
        )


def _det_fallback(what: str) -> None:
    """``what`` breaks the "ours" schedule's promise (every GEMM on our kernel) for a reason no
    route sees: say so once, as the routes' own warnings are."""
    if gemm_policy() == "ours":
        _warn_once(what)


def _det_library(what: str) -> None:
    """Serial deterministic schedule: ``what`` runs on a tuned hipBLASLt solution by design.  Those
    were bitwise reproducible in every repeat measured (GPT-2 124M at micro-batch 8 and 32, GPT-2 XL
    at 32; profiles/r4/det/, profiles/r5/det/), which pins no other shape: name each such GEMM once
    in the log, so a run on a
    new shape knows which of its GEMMs rest on that evidence (LLMTRAIN_DET_SCHEDULE=ours moves every
    one the kernel can take onto the fixed-order kernel)."""
    if what not in _WARNED:
        _WARNED.add(what)
        logging.getLogger(__name__).warning(
            "run.deterministic (serial schedule): %s runs on hipBLASLt; its reproducibility is measured "
            "for GPT-2 124M at micro-batch 8/32 and GPT-2 XL at 32 only", what,
        )


def _lib_mm(a: torch.Tensor, b_t: torch.Tensor, bias: torch.Tensor | None = None, *, op: str) -> torch.Tensor:
    """``a @ b_t (+ bias)`` on the library GEMM, logged once per shape in the serial schedule."""
    if a.is_cuda and gemm_policy() == "serial":
        _det_library(f"GEMM {op} M={a.shape[0]} K={a.shape[1]} N={b_t.shape[1]}")
    return torch.mm(a, b_t) if bias is None else torch.addmm(bias, a, b_t)


_TUNED_BIAS_GEMMS: set[tuple[int, int, int]] | None = None


def _library_tuned_bias_gemm(m: int, n: int, k: int) -> bool:
    """Whether the shipped TunableOp table (llmtrain/runtime/tuned/) holds a measured library
    solution for the bias GEMM ``[m, k] @ [n, k]^T + bias``: such shapes were timed against our
    kernel when the table was made (micro-batch 32: qkv 0.109 vs 0.116 ms, out 0.041 vs 0.053 ms,
    profiles/r4/mb32/) and stay on the library."""
    global _TUNED_BIAS_GEMMS
    if _TUNED_BIAS_GEMMS is None:
        from ..runtime.tuning import TUNED_TABLE, tuned_gemms_active

        if not tuned_gemms_active():  # not (yet) loaded in this process: nothing is routed by it
            return False
        shapes: set[tuple[int, int, int]] = set()
        if TUNED_TABLE.is_file():
            for line in TUNED_TABLE.read_text().splitlines():
                parts = line.split(",")
                if len(parts) >= 2 and parts[0] == "GemmAndBiasTunableOp_BFloat16_TN" and parts[1].startswith("tn_"):
                    dims = parts[1].split("_")
                    shapes.add((int(dims[2]), int(dims[1]), int(dims[3])))  # tn_{N}_{M}_{K}: (M, N, K)
        _TUNED_BIAS_GEMMS = shapes
    return (m, n, k) in _TUNED_BIAS_GEMMS


def _routed(site: GemmSite, a, b, bias=None, u=None, *, seq_len=0, head_dim=64, allow_ours=True) -> Route:
    """:func:`route` of a call with these operands (every one must be 16-byte aligned), its
    warning issued."""
    m, k = a.shape
    n = b.shape[1] if site.b_kn else b.shape[0]
    if site is DX_ATTN and head_dim != 64:
        u = None  # runs as the plain dX GEMM, which does not read O
    r = route(
        site, m=m, k=k, n=n, a_bytes=a.numel() * a.element_size(), unit_stride=a.stride(1) == 1,
        aligned=all(t is None or t.data_ptr() % 16 == 0 for t in (a, b, bias, u)), has_bias=bias is not None,
        tuned_bias=site.tuned_bias and bias is not None and _library_tuned_bias_gemm(m, n, k), policy=gemm_policy(),
        seq_len=seq_len, head_dim=head_dim, allow_ours=allow_ours and a.is_cuda and a.dtype == torch.bfloat16,
    )
    if r.warning is not None:
        _warn_once(r.warning)
    return r


def _elementwise(name: str, t: torch.Tensor, *args):
    """A bandwidth-bound op of the library forms below: its HIP kernel, or the CPU oracle."""
    return getattr(hip_ops() if t.is_cuda else ref, name)(t, *args)


def linear_fwd(x, w, bias=None, *, allow_ours: bool = True):
    """``x @ w^T + bias`` (nn.Linear forward, bf16 out).  GPU: the fused MFMA GEMM with the bias in
    its epilogue where the shape allows and the library has no measured solution for it, else
    hipBLASLt."""
    if _routed(FWD, x, w, bias, allow_ours=allow_ours).ours:
        return run_gemm(FWD, x, w, bias)[0]
    return _lib_mm(x, w.t(), bias, op=FWD.lib_tag)


def linear_fwd_gelu(x, w, bias=None, *, allow_ours: bool = True):
    """``u = x @ w^T + bias`` and ``g = gelu(u)`` (exact erf GELU of the bf16 ``u``, which the
    backward reads): on GPU the GELU rides in the GEMM epilogue, no separate pass over ``u``."""
    if _routed(FWD_GELU, x, w, bias, allow_ours=allow_ours).ours:
        return run_gemm(FWD_GELU, x, w, bias)
    u = _lib_mm(x, w.t(), bias, op=FWD_GELU.lib_tag)
    return u, _elementwise("gelu_fwd", u)


def linear_fwd_gelu_gd(x, w, bias=None, *, allow_ours: bool = True):
    """``gd = gelu'(u)`` and ``g = gelu(u)`` of ``u = x @ w^T + bias`` (the bf16 ``u``, as the
    backward would read it): the fc forward keeps the GELU derivative instead of the
    pre-activation, so the MLP-projection dX epilogue (:func:`linear_dx_gd`) multiplies by a stored
    value instead of evaluating erf per element.  GPU: one fused-GEMM epilogue at any size; shapes
    that kernel does not take form ``u`` on the library and the two maps with torch ops."""
    if _routed(FWD_GELU_GD, x, w, bias, allow_ours=allow_ours).ours:
        return run_gemm(FWD_GELU_GD, x, w, bias)
    u = _lib_mm(x, w.t(), bias, op=FWD_GELU_GD.lib_tag)
    return ref.gelu_grad(u), _elementwise("gelu_fwd", u)


def linear_dx_gd(dy, w, gd, dbias=None, *, allow_ours: bool = True):
    """``du = (dy @ w) * gd`` and ``dbias += colsum(du)`` with ``gd = gelu'(u)`` stored by
    :func:`linear_fwd_gelu_gd`: the MLP-projection data gradient and the GELU backward in one GEMM
    epilogue on GPU."""
    if _routed(DX_GD, dy, w, None, gd, allow_ours=allow_ours).ours:
        return run_gemm(DX_GD, dy, w, None, gd, dbias)[0]
    du = (_lib_mm(dy, w, op=DX_GD.lib_tag).float() * gd.float()).to(dy.dtype)
    if dbias is not None:
        _elementwise("colsum_accum", du, dbias)
    return du


def linear_dx(dy, w, *, allow_ours: bool = True):
    """``dy @ w`` (data gradient of nn.Linear with weight ``w [out, in]``)."""
    if _routed(DX, dy, w, allow_ours=allow_ours).ours:
        return run_gemm(DX, dy, w)[0]
    return _lib_mm(dy, w, op=DX.lib_tag)


def head_logits(h, w):
    """``logits = h @ w^T`` for the vocab-padded LM head ``w [Vp, d]``: hipBLASLt on the fast path;
    in deterministic mode (either schedule) row chunks of the hand-written fixed-order kernel,
    written in place into one ``[M, Vp]`` output.  The library's tuned solution for this shape is a
    Stream-K kernel (``SK3``), which combines partial tiles in completion order — the one library
    GEMM left in the serial schedule when its bitwise guarantee failed once
    (profiles/r5/det/pytest_gpu_serial_divergence.txt, docs/round6.md §2)."""
    if _routed(HEAD_LOGITS, h, w).ours:
        return run_gemm(HEAD_LOGITS, h, w)[0]
    return _lib_mm(h, w.t(), op=HEAD_LOGITS.lib_tag)


def head_dx(dlogits, w):
    """``dh = dlogits @ w`` (LM-head data gradient, ``w [Vp, d]``), row-chunked like
    :func:`head_logits` on our kernel.  Deterministic mode always takes our kernel here: this is the
    step's only GEMM with a 50304-deep reduction, where the library picks split / Stream-K
    solutions whose partial sums combine in completion order — the one run-to-run difference left
    in the serial schedule (bench/determinism_probe.py at micro-batch 8: the gradients first differ
    at ln_f, the head dX's output)."""
    if _routed(HEAD_DX, dlogits, w).ours:
        return run_gemm(HEAD_DX, dlogits, w)[0]
    return _lib_mm(dlogits, w, op=HEAD_DX.lib_tag)


def linear_dx_gelu_bwd(dy, w, u, dbias=None, *, allow_ours: bool = True):
    """``du = (dy @ w) * gelu'(u)`` and ``dbias += colsum(du)``: the data gradient of the MLP
    projection fused with the GELU backward and the fc bias gradient (one GEMM epilogue on GPU
    instead of a GEMM plus a full read-modify pass over the [M, d_ff] activations)."""
    if _routed(DX_GELU, dy, w, None, u, allow_ours=allow_ours).ours:
        return run_gemm(DX_GELU, dy, w, None, u, dbias)[0]
    return _elementwise("gelu_bwd", _lib_mm(dy, w, op=DX_GELU.lib_tag), u, dbias)


def linear_dx_attn(dy, w, att, seqlen: int, v_bias_grad=None, head_dim: int = 64, *, allow_ours: bool = True):
    """Data gradient of the attention output projection, ``dO = dy @ w``, plus the flash-attention
    backward's row constants ``delta[b, h, t] = sum_d dO * O`` (``att`` = the attention output O)
    and, when given, ``v_bias_grad += colsum(dO)`` (the V part of the qkv bias gradient, valid
    without attention dropout).  GPU: one fused GEMM epilogue (csrc/gemm_fused.hip, attention
    delta) replacing the separate pass that re-read dO and O.  Returns ``(dO, delta)``; ``delta``
    is None when that epilogue is not taken (the attention backward then computes it itself, and
    the caller must leave ``v_bias_grad`` to it)."""
    r = _routed(DX_ATTN, dy, w, None, att, seq_len=seqlen, head_dim=head_dim, allow_ours=allow_ours)
    if not r.ours:
        return _lib_mm(dy, w, op=r.site.lib_tag), None
    if r.site is DX:
        return run_gemm(DX, dy, w)[0], None
    return run_gemm(DX_ATTN, dy, w, None, att, v_bias_grad, seq_len=seqlen)


def wgrad_accum(dst, dy, x, *, bias=None) -> None:
    """``dst (fp32 [N, K]) += dy[M, N]^T @ x[M, K]`` and, with ``bias`` (fp32 ``[N]``),
    ``bias += colsum(dy)`` — the weight and bias gradients of an nn.Linear whose output gradient
    is ``dy`` (``dy`` may be a column slice with a larger row stride).  GPU: the split-K MFMA GEMM
    of csrc/gemm_wgrad_pp.hip with the bias column sums fused."""
    if dst.is_cuda:
        hip_ops().wgrad_gemm_pp(dy, x, dst, bias, 0, -1)
        return
    dst.addmm_(dy.t().float(), x.float())
    if bias is not None:
        ref.colsum_accum(dy, bias)
