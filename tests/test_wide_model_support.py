"""Which model widths the fused engine claims on the GPU (``GPT.fused_supported``), the error for
the ones it does not, and the 2.7B preset — all without allocating: models live on ``meta``."""

from __future__ import annotations

from pathlib import Path

import pytest
import torch

from llmtrain.config.loader import load_and_validate_config
from llmtrain.models.gpt import FUSED_MAX_D_MODEL, GPT, GPTAdapter
from llmtrain.runtime.device import RuntimePolicy, settle_fused_path

PRESET = Path(__file__).resolve().parents[1] / "configs" / "presets" / "gpt_2p7b_mi355x.yaml"


def _meta_gpt(d_model: int, n_heads: int) -> GPT:
    with torch.device("meta"):
        return GPT(vocab_size=64, block_size=16, d_model=d_model, n_layers=1, n_heads=n_heads, d_ff=4 * d_model,
                   dropout=0.0)


def test_fused_supported_width_bound() -> None:
    assert FUSED_MAX_D_MODEL == 8192
    assert _meta_gpt(2560, 20).fused_supported("cuda")  # head dim 128
    assert _meta_gpt(8192, 64).fused_supported("cuda")  # the widest LayerNorm row
    assert not _meta_gpt(8320, 65).fused_supported("cuda")  # head dim 128 too, only the width is past the bound
    assert _meta_gpt(8320, 65).fused_supported("cpu")


def test_uncovered_width_error_names_the_bound() -> None:
    cfg, _, _ = load_and_validate_config(str(PRESET))
    gpu = RuntimePolicy(device=torch.device("cuda", 0), compute_dtype=torch.bfloat16, use_fused=True)
    with pytest.raises(ValueError, match=rf"<= {FUSED_MAX_D_MODEL};"):
        settle_fused_path(gpu, cfg, supported=False)


def test_2p7b_preset_is_covered() -> None:
    cfg, _, _ = load_and_validate_config(str(PRESET))
    m = cfg.model
    assert (m.d_model, m.n_layers, m.n_heads, m.d_ff, m.block_size) == (2560, 32, 20, 10240, 1024)
    assert cfg.run.device == "cuda" and cfg.run.precision == "bf16" and m.dropout == 0.0
    with torch.device("meta"):
        model = GPTAdapter().build_model(cfg)
    assert model.fused_supported("cuda")
    assert 2.6e9 < sum(p.numel() for p in model.parameters()) < 2.8e9
