"""The fused engine at head dims 80 and 96 (the GPT-3 2.7B / 760M head shapes) on the GPU: bf16 loss
and gradients against fp32 autograd of the module path, with and without key-padding masks (the
bounds of tests/test_engine_gpu.py::test_fused_engine_covers_reference_presets), and a bitwise
repeat of one deterministic forward+backward at head dim 80."""

from __future__ import annotations

import copy

import pytest
import torch
import torch.nn.functional as F

from llmtrain import ops
from llmtrain.models.gpt import GPT

pytestmark = pytest.mark.gpu

# V, block, d, L, H, F
SHAPES = {
    "head_dim_80": (512, 128, 160, 2, 2, 640),
    "head_dim_96": (512, 128, 192, 2, 2, 768),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("padded", [False, True])
def test_fused_engine_covers_mid_head_dims(gpu_device, shape, padded):
    V, block, d, L, H, F_ = SHAPES[shape]
    torch.manual_seed(0)
    ref_model = GPT(vocab_size=V, block_size=block, d_model=d, n_layers=L, n_heads=H, d_ff=F_, dropout=0.0)
    ref_model = ref_model.to(gpu_device)
    assert ref_model.fused_supported("cuda")
    fused = copy.deepcopy(ref_model)
    engine = fused.prepare_runtime(compute_dtype=torch.bfloat16)
    B = 4
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, V, (B, block), generator=g).to(gpu_device)
    labels = torch.randint(0, V, (B, block), generator=g).to(gpu_device)
    mask = None
    if padded:
        mask = torch.ones(B, block, dtype=torch.long)
        mask[0, block - block // 3 :] = 0
        mask[1, : block // 4 + 1] = 0
        mask[2, block // 2] = 0
        mask = mask.to(gpu_device)

    logits = ref_model(ids, attention_mask=mask)
    per_tok = F.cross_entropy(logits.reshape(-1, V).float(), labels.reshape(-1), reduction="none")
    loss_ref = per_tok.mean() if mask is None else per_tok[mask.reshape(-1).bool()].mean()
    loss_ref.backward()
    engine.store.zero_grad()
    loss = fused.fused_loss(ids, labels, mask)
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-2 * max(1.0, abs(loss_ref.item()))
    worst = 0.0
    for (name, p), (_, q) in zip(fused.named_parameters(), ref_model.named_parameters()):
        num = (p.grad - q.grad).norm().item()
        den = q.grad.norm().item() + 1e-12
        worst = max(worst, num / den)
        assert num / den < 3e-2, f"{name}: relative grad error {num / den:.3e}"
    print(f"{shape} padded={padded}: worst relative grad error {worst:.2e}")


def test_fused_step_bitwise_reproducible_head_dim_80(gpu_device) -> None:
    """Two fused forward+backward passes from the same weights and batch under ``run.deterministic``
    give the same loss and the same flat gradient buffer bit for bit: at head dim 80 the
    out-projection dX takes the plain fixed-order GEMM and the attention kernels their 72..120 path
    (fixed-order dQ plane and bias-row sums)."""
    V, block, d, L, H, F_ = SHAPES["head_dim_80"]
    with ops.kernel_policy(True):
        torch.manual_seed(0)
        base = GPT(vocab_size=V, block_size=block, d_model=d, n_layers=L, n_heads=H, d_ff=F_, dropout=0.0)
        base = base.to(gpu_device)
        ids = torch.randint(0, V, (8, block), device=gpu_device)
        grads, losses = [], []
        for _ in range(2):
            m = copy.deepcopy(base)
            engine = m.prepare_runtime(compute_dtype=torch.bfloat16)
            m.train()
            torch.manual_seed(123)
            engine.store.zero_grad()
            loss = m.fused_loss(ids, torch.roll(ids, -1, dims=1))
            loss.backward()
            torch.cuda.synchronize()
            grads.append(engine.store.grad.clone())
            losses.append(loss.item())
    assert losses[0] == losses[1]
    assert torch.equal(grads[0], grads[1])
    assert torch.isfinite(grads[0]).all() and grads[0].abs().max().item() > 0
