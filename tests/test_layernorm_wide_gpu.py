"""The wide-row LayerNorm kernels (2048 < d <= 8192, one workgroup per row; csrc/layernorm.hip)
against the plain-PyTorch fp32 oracle ``llmtrain.ops.reference`` on the same device, with the
tolerances of the narrow kernels' tests in ``test_kernels_gpu.py`` (same reference, same
arithmetic), plus the persistent narrow forward's row-stride loop over several passes.

Shapes are the smallest at which the kernels can go wrong: the first width past the boundary
(2052 = one chunk beyond a full pass of a 256-thread workgroup), the 2.7B preset's width, a width
of each wider thread shape, and the maximum width ragged (8188) and full (8192)."""

from __future__ import annotations

import functools

import pytest
import torch

from llmtrain.ops import reference as ref

pytestmark = pytest.mark.gpu

WIDE = [(5, 2052), (37, 2560), (3, 4096), (9, 8188), (9, 8192)]
# Forward: a workgroup takes one row per pass and the grid is capped at 8 x CUs workgroups for
# d <= 4096 (2048 on an MI355X's 256 CUs; 4 x CUs above), so 16387 rows are 8 full passes and a
# last one of 3 rows.
FWD_STRIDE = (16387, 2052)
# Backward: one row per pass and a grid cap of 3 x CUs = 768 workgroups for d <= 3072 (2 x CUs up
# to 4096, 1 x CUs above), so 4099 rows are 5 full passes and a last one of 259 rows.
BWD_STRIDE = (4099, 2304)
# The narrow persistent forward (768 < d <= 2048) gives a wave one row per pass, 4 waves per
# workgroup, grid capped at 8 x CUs: 8192 rows per pass, so 16387 rows are 2 passes and 3 rows.
NARROW_STRIDE = (16387, 1600)


def hip():
    return torch.ops.llmtrain_hip


def _close(a, b, atol, rtol, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{what}: {bad} elements out of tolerance, max err {err.max().item():.3e}"


@functools.lru_cache(maxsize=8)
def _inputs(M, d, dev):
    """Random operands of one shape, made once and shared (read-only) by every test of that shape."""
    g = torch.Generator(device="cpu").manual_seed(M + d)
    t = {
        "x": torch.randn(M, d, generator=g),
        "delta": torch.randn(M, d, generator=g).to(torch.bfloat16),
        "w": 1 + 0.1 * torch.randn(d, generator=g),
        "b": 0.1 * torch.randn(d, generator=g),
        "dy": torch.randn(M, d, generator=g).to(torch.bfloat16),
        "dres": torch.randn(M, d, generator=g),
    }
    return {k: v.to(dev) for k, v in t.items()}


def _check_fwd(dev, M, d, with_delta, x_dt, delta_dt, y_dt, drop):
    t = _inputs(M, d, dev)
    x = t["x"].to(x_dt)
    delta = t["delta"].to(delta_dt) if with_delta else None
    seed = ref.dropout_site_seed(5, 3)
    xs, y, mu, rs = hip().add_layernorm_fwd(x, delta, t["w"], t["b"], 1e-5, y_dt, drop, seed)
    xs_r, y_r, mu_r, rs_r = ref.add_layernorm_fwd(x, delta, t["w"], t["b"], 1e-5, torch.float32, drop, seed)
    assert y.dtype == y_dt and y.shape == (M, d)
    if with_delta:
        assert xs.dtype == x_dt
        if x_dt == torch.bfloat16:
            assert torch.equal(xs, xs_r), "xs: not the reference's rounding"
        else:
            _close(xs, xs_r, 1e-6, 1e-6, "xs")
    _close(mu, mu_r, 1e-5, 1e-5, "mean")
    _close(rs, rs_r, 1e-4, 1e-4, "rstd")
    if y_dt == torch.bfloat16:
        _close(y, y_r, 2e-2, 1e-2, "y(bf16)")
    else:
        # fp32 y has no storage rounding: what the mean / rstd bounds above allow,
        # |w| * (|d mean| * rstd + |x - mean| * |d rstd|) <= 1.5 * (1e-5 + 6 * 1e-4) < 1e-3
        _close(y, y_r, 1e-3, 1e-3, "y(f32)")


BF, F32 = torch.bfloat16, torch.float32
# (with_delta, x dtype, delta dtype, y dtype, dropout)
FWD_CASES = [
    (False, F32, BF, BF, 0.0),
    (True, F32, BF, BF, 0.0),
    (True, F32, F32, F32, 0.2),
    (False, BF, BF, F32, 0.0),
    (True, BF, BF, BF, 0.2),
    (True, BF, F32, F32, 0.0),
    (True, F32, BF, BF, 0.2),
]


@pytest.mark.parametrize("M,d", WIDE)
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: f"delta{int(c[0])}-x{'bf' if c[1] == BF else 'f32'}-"
                         f"d{'bf' if c[2] == BF else 'f32'}-y{'bf' if c[3] == BF else 'f32'}-p{c[4]}")
def test_wide_add_layernorm_fwd(gpu_device, M, d, case):
    _check_fwd(gpu_device, M, d, *case)


@pytest.mark.parametrize("M,d", [FWD_STRIDE, NARROW_STRIDE])
@pytest.mark.parametrize("x_dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("drop", [0.0, 0.2])
def test_fwd_row_stride_passes(gpu_device, M, d, x_dt, drop):
    """More rows than the persistent forward's grid holds: several passes and a ragged last one,
    for the wide kernel and (NARROW_STRIDE) the one-wave-per-row kernel of 768 < d <= 2048."""
    _check_fwd(gpu_device, M, d, True, x_dt, BF, BF, drop)


@pytest.mark.parametrize("M,d", WIDE + [BWD_STRIDE])
@pytest.mark.parametrize("with_proj,lowp,drop", [(True, True, 0.0), (False, False, 0.0), (False, True, 0.0),
                                                 (True, True, 0.2), (False, True, 0.2)])
def test_wide_layernorm_bwd(gpu_device, M, d, with_proj, lowp, drop):
    """fp32 residual / gradient stream: dx, the bf16 (branch-dropout) copy, and dgamma / dbeta /
    dproj accumulated into non-zero buffers; an unused dproj is left bit-identical."""
    t = _inputs(M, d, gpu_device)
    x, w = t["x"], t["w"]
    _, _, mu, rs = ref.add_layernorm_fwd(x, None, w, torch.zeros_like(w), 1e-5, torch.float32)
    scale = torch.tensor(0.5, device=gpu_device)
    seed = ref.dropout_site_seed(7, 2)
    dw, db, dp = (torch.full((d,), 0.25, device=gpu_device) for _ in range(3))
    dw_r, db_r, dp_r = dw.clone(), db.clone(), dp.clone()
    dx, dx_lp = hip().layernorm_bwd(t["dy"], x, mu, rs, w, t["dres"], dw, db, scale, lowp,
                                    dp if with_proj else None, drop, seed)
    dx_r = ref.layernorm_bwd(t["dy"], x, mu, rs, w, t["dres"], dw_r, db_r, scale)
    br_r = ref._apply_dropout(dx_r, drop, seed)
    ref.colsum_accum(br_r, dp_r)
    _close(dx, dx_r, 1e-4, 1e-4, "dx")
    if lowp:
        assert dx_lp.dtype == torch.bfloat16
        _close(dx_lp, br_r, 2e-2, 1e-2, "dx_lp")
    _close(dw, dw_r, 1e-2, 1e-4, "dgamma")
    _close(db, db_r, 1e-2, 1e-4, "dbeta")
    if with_proj:
        _close(dp, dp_r, 2e-2, 1e-4, "dproj")
    else:
        assert torch.equal(dp, torch.full((d,), 0.25, device=gpu_device))


@pytest.mark.parametrize("M,d", WIDE + [BWD_STRIDE])
@pytest.mark.parametrize("mode", ["bf16_grad", "bf16"])
@pytest.mark.parametrize("drop", [0.0, 0.2])
def test_wide_layernorm_bf16_residual_streams(gpu_device, M, d, mode, drop):
    """The engine's bf16 residual options on wide rows: forward into a bf16 residual stream, backward
    with a bf16 gradient stream; without dropout the bf16 GEMM operand IS dx (one buffer)."""
    t = _inputs(M, d, gpu_device)
    res_dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, w, b = t["x"].to(res_dt), t["w"], t["b"]
    seed = ref.dropout_site_seed(5, 3)
    xs, y, mu, rs = hip().add_layernorm_fwd(x, t["delta"], w, b, 1e-5, torch.bfloat16, drop, seed)
    xs_r, y_r, mu_r, rs_r = ref.add_layernorm_fwd(x, t["delta"], w, b, 1e-5, torch.float32, drop, seed)
    assert xs.dtype == res_dt
    _close(xs, xs_r, 1e-6, 1e-6 if mode != "bf16" else 0.0, "xs")  # the same rounding
    _close(mu, mu_r, 1e-5, 1e-5, "mean")
    _close(rs, rs_r, 1e-4, 1e-4, "rstd")
    _close(y, y_r, 2e-2, 1e-2, "y")

    dres = t["dres"].to(torch.bfloat16)
    scale = torch.tensor(0.5, device=gpu_device)
    dw, db = torch.full((d,), 0.25, device=gpu_device), torch.full((d,), -0.5, device=gpu_device)
    dw_r, db_r = dw.clone(), db.clone()
    dx, dx_lp = hip().layernorm_bwd(t["dy"], xs, mu, rs, w, dres, dw, db, scale, True, None, drop, seed, True)
    dx_r = ref.layernorm_bwd(t["dy"], xs, mu, rs, w, dres, dw_r, db_r, scale, torch.float32)
    assert dx.dtype == torch.bfloat16
    _close(dx, dx_r, 1e-2, 8e-3, "dx (bf16 stream)")
    _close(dx_lp, ref._apply_dropout(dx.float(), drop, seed), 1e-2, 8e-3, "dx_lp")
    assert (dx_lp.data_ptr() == dx.data_ptr()) == (drop == 0.0)  # the operand is the stream itself
    _close(dw, dw_r, 1e-2, 1e-4, "dgamma")
    _close(db, db_r, 1e-2, 1e-4, "dbeta")


@pytest.mark.parametrize("M,d", [(37, 2560), BWD_STRIDE, (9, 8192)])
def test_wide_layernorm_bwd_deferred_params_batched(gpu_device, M, d):
    """Two wide LayerNorm backwards with their dgamma / dbeta partial rows reduced by ONE
    ln_param_reduce launch give exactly (bitwise) what the immediate per-LayerNorm reduce gives."""
    outs = {}
    for mode in ("immediate", "deferred"):
        dst, parts = [], []
        for k in range(2):
            gk = torch.Generator(device="cpu").manual_seed(100 + k)
            x = torch.randn(M, d, generator=gk).to(gpu_device)
            w = (1 + 0.1 * torch.randn(d, generator=gk)).to(gpu_device)
            _, _, mu, rs = ref.add_layernorm_fwd(x, None, w, torch.zeros(d, device=gpu_device), 1e-5, torch.float32)
            dy = torch.randn(M, d, generator=gk).to(gpu_device, torch.bfloat16)
            dw, db = torch.full((d,), 0.5, device=gpu_device), torch.full((d,), -0.5, device=gpu_device)
            if mode == "immediate":
                dx, _ = hip().layernorm_bwd(dy, x, mu, rs, w, None, dw, db, None, True, None)
            else:
                dx, _, pr = hip().layernorm_bwd_deferred(dy, x, mu, rs, w, None, dw, db, None, True)
                parts.append(pr)
                assert torch.equal(dw, torch.full((d,), 0.5, device=gpu_device))  # not yet reduced
            dst += [dw, db, dx]
        if parts:
            assert parts[0].shape == parts[1].shape and parts[0].shape[2] == d
            hip().ln_param_reduce(parts, [dst[0], dst[1], dst[3], dst[4]])
        outs[mode] = dst
    for a, b in zip(outs["immediate"], outs["deferred"]):
        assert torch.equal(a, b)
    assert not torch.equal(outs["immediate"][0], torch.full((d,), 0.5, device=gpu_device))


def test_wide_layernorm_bwd_is_reproducible(gpu_device):
    """Fixed summation order (no atomics): two runs of the multi-pass backward are bitwise equal."""
    M, d = BWD_STRIDE
    t = _inputs(M, d, gpu_device)
    x, w = t["x"], t["w"]
    _, _, mu, rs = ref.add_layernorm_fwd(x, None, w, torch.zeros_like(w), 1e-5, torch.float32)
    runs = []
    for _ in range(2):
        dw, db, dp = (torch.full((d,), 0.25, device=gpu_device) for _ in range(3))
        dx, dx_lp = hip().layernorm_bwd(t["dy"], x, mu, rs, w, t["dres"], dw, db, None, True, dp, 0.2, 11)
        runs.append((dw, db, dp, dx, dx_lp))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_layernorm_width_bound(gpu_device):
    """Past the widest kernel the ops raise, and the message names the bound."""
    M, d = 2, 8196
    x = torch.randn(M, d, device=gpu_device)
    w, b = torch.ones(d, device=gpu_device), torch.zeros(d, device=gpu_device)
    with pytest.raises(RuntimeError, match="8192"):
        hip().add_layernorm_fwd(x, None, w, b, 1e-5, torch.bfloat16)
    mu, rs = torch.zeros(M, device=gpu_device), torch.ones(M, device=gpu_device)
    dw, db = torch.zeros(d, device=gpu_device), torch.zeros(d, device=gpu_device)
    with pytest.raises(RuntimeError, match="8192"):
        hip().layernorm_bwd(x.to(torch.bfloat16), x, mu, rs, w, None, dw, db, None, False, None)
