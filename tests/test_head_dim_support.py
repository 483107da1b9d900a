"""Which head dims the fused engine claims on the GPU (``GPT.fused_supported``): every multiple of 8
from 8 to 128 — the GPT-3 shapes' 80 and 96 included — and the published-shape 2.7B preset (32
heads of 80).  No allocation: models live on ``meta``."""

from __future__ import annotations

from pathlib import Path

import pytest
import torch

from llmtrain.config.loader import load_and_validate_config
from llmtrain.models.gpt import GPT, GPTAdapter

PRESETS = Path(__file__).resolve().parents[1] / "configs" / "presets"


def _meta_gpt(d_model: int, n_heads: int) -> GPT:
    with torch.device("meta"):
        return GPT(vocab_size=64, block_size=16, d_model=d_model, n_layers=1, n_heads=n_heads, d_ff=4 * d_model,
                   dropout=0.0)


@pytest.mark.parametrize("d_model,n_heads,hd", [
    (576, 8, 72), (2560, 32, 80), (704, 8, 88), (1536, 16, 96), (832, 8, 104), (1792, 16, 112), (960, 8, 120),
])
def test_fused_supported_head_dims_72_to_120(d_model: int, n_heads: int, hd: int) -> None:
    model = _meta_gpt(d_model, n_heads)
    assert model.d_model // model.n_heads == hd
    assert model.fused_supported("cuda")


@pytest.mark.parametrize("d_model,n_heads,hd", [(1088, 8, 136), (544, 8, 68), (1152, 8, 144), (32, 8, 4)])
def test_fused_unsupported_head_dims(d_model: int, n_heads: int, hd: int) -> None:
    model = _meta_gpt(d_model, n_heads)
    assert model.d_model // model.n_heads == hd
    assert not model.fused_supported("cuda")
    assert model.fused_supported("cpu")  # the CPU engine runs the reference ops: any shape


def test_fused_supported_unchanged_at_64_and_128() -> None:
    assert _meta_gpt(768, 12).fused_supported("cuda")  # 64
    assert _meta_gpt(2560, 20).fused_supported("cuda")  # 128
    assert _meta_gpt(256, 8).fused_supported("cuda")  # 32
    assert _meta_gpt(64, 8).fused_supported("cuda")  # 8


def test_gpt3_2p7b_preset_is_the_published_shape_and_covered() -> None:
    cfg, _, _ = load_and_validate_config(str(PRESETS / "gpt3_2p7b_mi355x.yaml"))
    m = cfg.model
    assert (m.d_model, m.n_layers, m.n_heads, m.d_ff, m.block_size) == (2560, 32, 32, 10240, 1024)
    assert m.d_model // m.n_heads == 80
    assert not m.extra.get("allow_module_fallback", False)
    with torch.device("meta"):
        model = GPTAdapter().build_model(cfg)
    assert model.fused_supported("cuda")
    # everything but the head count equals the 20 x 128 preset
    other, _, _ = load_and_validate_config(str(PRESETS / "gpt_2p7b_mi355x.yaml"))
    a, b = cfg.model.model_dump(), other.model.model_dump()
    assert a.pop("n_heads") == 32 and b.pop("n_heads") == 20
    assert a == b
    assert cfg.trainer.model_dump() == other.trainer.model_dump()
