"""Flash-attention kernels at head dims 72..120 (multiples of 8: GPT-3 2.7B's 80, 760M's 96) against
the INDEPENDENT oracle of tests/test_attention_gpu.py, re-implemented here: fp32 autograd of eager
attention on the same bf16 inputs, no kernel output fed into it, the same bounds.  These dims run
the 128-wide tiles with the dims at or past hd zero-filled at load time and never stored; a missing
zero-fill reads the NEXT head's data (or past the allocation for the last head of the last token),
so every case has H >= 2 with random data in all heads."""

from __future__ import annotations

import math

import pytest
import torch

from llmtrain import ops

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_device")]

MID_DIMS = (72, 80, 88, 96, 104, 112, 120)


def hip():
    return torch.ops.llmtrain_hip


def _oracle(qkv: torch.Tensor, B: int, T: int, H: int, key_valid: torch.Tensor | None, dout: torch.Tensor):
    """fp32 autograd: returns (out [B*T, H*hd], dqkv [B*T, 3*H*hd], live [B, T] rows with a valid key)."""
    hd = qkv.shape[1] // (3 * H)
    x = qkv.float().detach().requires_grad_(True)
    q, k, v = (t.transpose(1, 2) for t in x.view(B, T, 3, H, hd).unbind(dim=2))
    s = (q @ k.transpose(-2, -1)) / math.sqrt(hd)
    masked = torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu(1)[None, None]
    if key_valid is not None:
        masked = masked | ~key_valid.bool()[:, None, None, :]
    s = s.masked_fill(masked, torch.finfo(torch.float32).min)  # reference's mask value
    out = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * T, H * hd)
    live = (~masked).any(dim=-1)[:, 0].expand(B, T)  # [B, T]
    out.backward(dout.float())
    return out.detach(), x.grad.detach(), live


def _check(name: str, got: torch.Tensor, want: torch.Tensor, rows_dim_last: int, slack: float = 6e-2) -> None:
    got, want = got.float(), want.float()
    # tensor-wide: relative Frobenius error (bf16 operands, fp32 accumulation)
    rel = (got - want).norm() / want.norm().clamp_min(1e-12)
    print(f"{name}: relative error {rel:.3e}")
    assert rel < 1.5e-2, f"{name}: relative error {rel:.3e}"
    # per row (each token's vector): catches a single wrong row that a tensor-wide norm would hide
    g2, w2 = got.reshape(-1, rows_dim_last), want.reshape(-1, rows_dim_last)
    row_err = (g2 - w2).norm(dim=1)
    row_ref = w2.norm(dim=1)
    bad = row_err > 3e-2 * row_ref + slack * row_ref.mean()  # rows that cancel to ~0 (dq of query 0)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} rows off, first {bad.nonzero()[:4].flatten().tolist()}"


def _mask(B: int, T: int, kind: str | None, device) -> torch.Tensor | None:
    if kind is None:
        return None
    m = torch.ones(B, T, dtype=torch.long)
    m[0, T - T // 3 :] = 0  # right padding
    if B > 1:
        m[1, : T // 4 + 3] = 0  # left padding: those queries see no valid key
    if B > 2:
        m[2, 5] = 0
        m[2, T // 2 : T // 2 + 70] = 0  # holes, one spanning a 64-key tile boundary
    return m.to(device)


def _check_all(qkv, dout, out, lse, dqkv, dbias, B, T, H, hd, mask) -> None:
    out_r, dqkv_r, live = _oracle(qkv, B, T, H, mask, dout)
    live_rows = live.reshape(-1)
    _check("out", out[live_rows], out_r[live_rows], hd)
    if not bool(live_rows.all()):  # rows without a valid key: O = 0, lse = +inf
        assert torch.all(out[~live_rows] == 0)
        dead_lse = lse.permute(0, 2, 1).reshape(-1, H)[~live_rows]
        assert torch.all(torch.isinf(dead_lse) & (dead_lse > 0))
    a = dqkv.float().view(B * T, 3, H, hd)
    r = dqkv_r.view(B * T, 3, H, hd)
    for i, name in enumerate(("dq", "dk", "dv")):
        _check(name, a[:, i], r[:, i], hd)
    assert torch.isfinite(dqkv.float()).all()
    # fused qkv-bias gradient == column sums of the dqkv the kernel wrote
    torch.testing.assert_close(dbias, dqkv.float().sum(0), atol=2e-2 * dbias.abs().max().item() + 1e-3, rtol=1e-2)


CASES = [
    # B, T, H, hd, padding
    *[(2, 200, 3, hd, None) for hd in MID_DIMS],  # ragged T, two 128-key blocks, a partial last Q tile
    (3, 300, 4, 80, "mixed"),
    (3, 300, 4, 96, "mixed"),
    (2, 1024, 4, 80, None),  # 8 key blocks: the dQ reduce over many planes
    (1, 2, 2, 112, None),  # the smallest tiles
    (1, 70, 2, 72, None),
]


@pytest.mark.parametrize("B,T,H,hd,pad", CASES)
def test_attention_midhd_matches_autograd(gpu_device, B: int, T: int, H: int, hd: int, pad: str | None) -> None:
    g = torch.Generator(device="cpu").manual_seed(B * T + H + hd)
    d = H * hd
    qkv = torch.randn(B * T, 3 * d, generator=g).to(gpu_device, torch.bfloat16)
    mask = _mask(B, T, pad, gpu_device)
    km = None if mask is None else ops.attn_key_masks(mask)
    dout = torch.randn(B * T, d, generator=g).to(gpu_device, torch.bfloat16)
    if mask is not None:  # the engine zeroes the attention branch of padded queries: no gradient there
        dout = dout * mask.reshape(-1, 1).to(dout.dtype)

    out, lse = hip().attn_fwd(qkv, B, T, H, 0.0, 0, None if km is None else km[0])
    dbias = torch.zeros(3 * d, device=gpu_device)
    dqkv = hip().attn_bwd(dout, qkv, out, lse, B, T, H, 0.0, 0, dbias, None, None if km is None else km[1])
    assert out.shape == (B * T, d) and dqkv.shape == qkv.shape
    _check_all(qkv, dout, out, lse, dqkv, dbias, B, T, H, hd, mask)


@pytest.mark.parametrize("hd,B,T,H", [(80, 2, 200, 3), (96, 2, 200, 3)])
def test_attention_midhd_dropout(gpu_device, hd: int, B: int, T: int, H: int) -> None:
    """Probability dropout against fp32 autograd of eager dropout attention.  Only the keep mask is
    shared with the kernel (the counter hash of ``ops/reference.attn_dropout_keep``); the oracle forms
    its own softmax, lse, O and gradients from the bf16 inputs."""
    from llmtrain.ops import reference as ref

    g = torch.Generator(device="cpu").manual_seed(hd)
    qkv = torch.randn(B * T, 3 * hd * H, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * T, hd * H, generator=g).to(torch.bfloat16)
    p_drop, seed = 0.25, ref.dropout_site_seed(11, 8)
    out_g, lse_g = ops.attn_fwd(qkv.to(gpu_device), B, T, H, dropout=(p_drop, seed))
    dbias = torch.zeros(3 * hd * H, device=gpu_device)
    dq_g = ops.attn_bwd(dout.to(gpu_device), qkv.to(gpu_device), out_g, lse_g, B, T, H, dropout=(p_drop, seed),
                        qkv_bias_grad=dbias).cpu().float()

    keep = ref.attn_dropout_keep(seed, p_drop, B, H, T, torch.device("cpu"))  # [B, H, T, T]
    x = qkv.float().detach().requires_grad_(True)
    q, k, v = (t.transpose(1, 2) for t in x.view(B, T, 3, H, hd).unbind(dim=2))
    s = (q @ k.transpose(-2, -1)) / math.sqrt(hd)
    causal = torch.ones(T, T, dtype=torch.bool).triu(1)[None, None]
    s = s.masked_fill(causal, torch.finfo(torch.float32).min)
    lse_r = torch.logsumexp(s, dim=-1)  # the undropped normaliser the kernel stores
    _, dscale = ref.dropout_params(p_drop)  # 1 / keep probability of the 16-bit threshold
    probs = torch.where(keep, torch.softmax(s, dim=-1) * dscale, torch.zeros(()))
    out_r = (probs @ v).transpose(1, 2).reshape(B * T, H * hd)
    out_r.backward(dout.float())
    dq_r = x.grad

    torch.testing.assert_close(lse_g.cpu(), lse_r, atol=2e-3, rtol=2e-3)
    _check("out (dropout)", out_g.cpu(), out_r.detach(), hd)
    a, r = dq_g.view(B * T, 3, H, hd), dq_r.view(B * T, 3, H, hd)
    # dq of query 0 is exactly 0 in exact arithmetic; the kernel's delta comes from the bf16 O, whose
    # rounding the 1 / keep-probability scale amplifies (the slack of tests/test_attention_gpu.py)
    for i, name in enumerate(("dq", "dk", "dv")):
        _check(f"{name} (dropout)", a[:, i], r[:, i], hd, slack=0.15)
    want = dq_r.sum(dim=0)
    assert (dbias.cpu() - want).abs().max().item() < 2e-2 * want.abs().max().item()


def test_attention_midhd_reads_nothing_past_the_end(gpu_device) -> None:
    """qkv and dout are the leading parts of larger buffers whose tails are NaN, so the last head of
    the last token is followed directly by NaNs: a load of the tile's dims 80..127 that was not
    turned into zeros would bring them in (0 * NaN = NaN reaches every output of that head)."""
    B, T, H, hd = 2, 70, 2, 80
    g = torch.Generator(device="cpu").manual_seed(17)
    n_qkv, n_out, tail = B * T * 3 * H * hd, B * T * H * hd, 4096
    qkv_buf = torch.full((n_qkv + tail,), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    dout_buf = torch.full((n_out + tail,), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    qkv_buf[:n_qkv] = torch.randn(n_qkv, generator=g).to(gpu_device, torch.bfloat16)
    dout_buf[:n_out] = torch.randn(n_out, generator=g).to(gpu_device, torch.bfloat16)
    qkv = qkv_buf[:n_qkv].view(B * T, 3 * H * hd)
    dout = dout_buf[:n_out].view(B * T, H * hd)
    assert qkv.is_contiguous() and dout.is_contiguous() and qkv.data_ptr() == qkv_buf.data_ptr()

    out, lse = hip().attn_fwd(qkv, B, T, H, 0.0, 0, None)
    dbias = torch.zeros(3 * H * hd, device=gpu_device)
    dqkv = hip().attn_bwd(dout, qkv, out, lse, B, T, H, 0.0, 0, dbias, None, None)
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv), ("dbias", dbias)):
        assert torch.isfinite(t.float()).all(), f"{name} is not finite"
    _check_all(qkv.clone(), dout.clone(), out, lse, dqkv, dbias, B, T, H, hd, None)


def test_attention_midhd_zero_fill_is_inert(gpu_device) -> None:
    """Head 0's results do not depend on the other heads' values, bit for bit: the tile's dims
    96..127 of head 0 lie over head 1's first 32 dims in memory."""
    B, T, H, hd = 2, 200, 3, 96
    g = torch.Generator(device="cpu").manual_seed(23)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).to(gpu_device, torch.bfloat16)
    dout = torch.randn(B * T, H * hd, generator=g).to(gpu_device, torch.bfloat16)
    other = qkv.clone().view(B * T, 3, H, hd)
    other[:, :, 1:] = (3.0 * torch.randn(B * T, 3, H - 1, hd, generator=g)).to(gpu_device, torch.bfloat16)
    other = other.view(B * T, 3 * H * hd)
    assert torch.equal(other.view(B * T, 3, H, hd)[:, :, 0], qkv.view(B * T, 3, H, hd)[:, :, 0])
    res = []
    for x in (qkv, other):
        out, lse = hip().attn_fwd(x, B, T, H, 0.0, 0, None)
        dqkv = hip().attn_bwd(dout, x, out, lse, B, T, H, 0.0, 0, None, None, None)
        res.append((out.view(B * T, H, hd)[:, 0].clone(), lse[:, 0].clone(), dqkv.view(B * T, 3, H, hd)[:, :, 0].clone()))
    assert not torch.equal(res[0][0], torch.zeros_like(res[0][0]))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
