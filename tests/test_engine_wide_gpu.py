"""The fused engine end to end above d_model 2048 (wide-row LayerNorm kernels, every other kernel
at a width it had not run at): the bf16 fused path against fp32 autograd of the module path, as
``test_fused_engine_covers_reference_presets`` does for the narrower shapes, with its bounds."""

from __future__ import annotations

import copy

import pytest
import torch
import torch.nn.functional as F

from llmtrain.models.gpt import GPT

pytestmark = pytest.mark.gpu

# two layers each: V, block, d, L, H, F
WIDE_SHAPES = {
    "d2304_hd128": (512, 128, 2304, 2, 18, 4608),
    "d2560_hd64": (512, 128, 2560, 2, 40, 2560),
}


@pytest.mark.parametrize("shape", sorted(WIDE_SHAPES))
@pytest.mark.parametrize("padded", [False, True])
def test_fused_engine_covers_wide_models(gpu_device, shape, padded):
    V, block, d, L, H, F_ = WIDE_SHAPES[shape]
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
    print(f"{shape} padded={padded}: loss {loss.item():.5f} vs {loss_ref.item():.5f}")
    assert abs(loss.item() - loss_ref.item()) < 1e-2 * max(1.0, abs(loss_ref.item()))
    worst = 0.0
    for (name, p), (_, q) in zip(fused.named_parameters(), ref_model.named_parameters()):
        num = (p.grad - q.grad).norm().item()
        den = q.grad.norm().item() + 1e-12
        worst = max(worst, num / den)
        assert num / den < 3e-2, f"{name}: relative grad error {num / den:.3e}"
    print(f"{shape} padded={padded}: worst relative grad error {worst:.2e}")
