"""Routing of the forward / dX GEMMs (llmtrain.ops.gemm.route, row_chunks): which kernel every
call site takes for a shape, placement, kernel policy and knob setting.  Pure functions, no GPU."""

from __future__ import annotations

import pytest

from llmtrain.ops import gemm
from llmtrain.ops.gemm import Epilogue

MIB = 2**20


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.setattr(gemm, "FGEMM_MAX_A_BYTES", 64 * MIB)
    monkeypatch.setattr(gemm, "FGEMM_ANY_SIZE", frozenset({"dx_gelu", "dx_attn"}))
    monkeypatch.setattr(gemm, "FGEMM_NEVER", frozenset())


def _route(site, m, k, n, policy="fast", **kw):
    args = {"a_bytes": 2 * m * k, "aligned": True, "unit_stride": True, "has_bias": False, "tuned_bias": False,
            "seq_len": 1024}
    args.update(kw)
    return gemm.route(site, m=m, k=k, n=n, policy=policy, **args)


# (site, (M, K, N), takes our kernel on the fast path)
FAST = [
    (gemm.FWD, (32768, 768, 2304), True),
    (gemm.FWD, (43690, 768, 2304), True),  # A = 67,107,840 B
    (gemm.FWD, (43691, 768, 2304), False),  # one row over the 64 MiB cap
    (gemm.FWD, (131072, 768, 2304), False),
    (gemm.DX_GELU, (131072, 3072, 768), True),  # any size
    (gemm.DX_ATTN, (131072, 768, 768), True),  # any size
    (gemm.FWD_GELU, (131072, 768, 3072), False),
    # the shape gate: K % 64 == 0, K >= 256, N % 8 == 0
    (gemm.DX, (4096, 192, 768), False),
    (gemm.DX, (4096, 320, 768), True),
    (gemm.DX, (4096, 256, 100), False),
    (gemm.DX, (4096, 256, 104), True),
]
SHAPE_GATED = {(192, 768), (256, 100)}


@pytest.mark.parametrize("site,mkn,ours", FAST, ids=lambda v: getattr(v, "tag", None) or str(v))
def test_fast_policy_table(site, mkn, ours):
    r = _route(site, *mkn)
    assert r.ours is ours and r.site is site and r.warning is None
    assert not _route(site, *mkn, aligned=False).ours  # an operand 8 bytes off 16-byte alignment
    # the "ours" schedule lifts the size cap (and nothing else)
    assert _route(site, *mkn, policy="ours").ours is (mkn[1:] not in SHAPE_GATED)
    assert _route(site, *mkn, policy="serial").ours is ours


def test_size_knobs(monkeypatch):
    big = (131072, 768, 2304)
    assert not _route(gemm.FWD, *big).ours and not _route(gemm.FWD, *big, policy="serial").ours
    monkeypatch.setattr(gemm, "FGEMM_ANY_SIZE", frozenset({"fwd"}))
    assert _route(gemm.FWD, *big).ours
    assert not _route(gemm.DX_GELU, 131072, 3072, 768).ours  # no longer listed
    monkeypatch.setattr(gemm, "FGEMM_MAX_A_BYTES", 0)
    assert not _route(gemm.DX, 4096, 768, 768).ours and _route(gemm.DX, 4096, 768, 768, policy="ours").ours
    # the gd sites and the head are not size-routed
    assert _route(gemm.FWD_GELU_GD, 131072, 768, 3072).ours and _route(gemm.DX_GD, 131072, 3072, 768).ours
    assert _route(gemm.HEAD_DX, 131072, 50304, 768, policy="serial").ours


def test_never_knob(monkeypatch):
    monkeypatch.setattr(gemm, "FGEMM_NEVER", frozenset({"fwd"}))
    assert not _route(gemm.FWD, 4096, 768, 2304).ours
    assert not _route(gemm.FWD, 4096, 768, 2304, policy="serial").ours
    assert _route(gemm.FWD, 4096, 768, 2304, policy="ours").ours
    assert _route(gemm.DX, 4096, 768, 2304).ours


def test_tuned_bias_rule():
    shape = (32768, 768, 2304)
    assert not _route(gemm.FWD, *shape, has_bias=True, tuned_bias=True).ours
    assert _route(gemm.FWD, *shape, has_bias=False, tuned_bias=True).ours
    assert _route(gemm.FWD, *shape, has_bias=True, tuned_bias=True, policy="serial").ours
    assert _route(gemm.FWD, *shape, has_bias=True, tuned_bias=True, policy="ours").ours
    assert _route(gemm.FWD_GELU, *shape, has_bias=True, tuned_bias=True).ours  # fwd only


@pytest.mark.parametrize("site,mkn", [(gemm.HEAD_LOGITS, (131072, 768, 50304)), (gemm.HEAD_DX, (131072, 50304, 768))])
def test_head_sites_take_our_kernel_in_deterministic_mode_only(site, mkn):
    assert not _route(site, *mkn).ours and _route(site, *mkn).warning is None
    assert _route(site, *mkn, policy="serial").ours and _route(site, *mkn, policy="ours").ours
    assert not _route(site, *mkn, policy="serial", unit_stride=False).ours  # a column slice of a wider tensor
    assert site.max_rows == 16384


def test_dx_attn_preconditions_and_fallback():
    r = _route(gemm.DX_ATTN, 4096, 256, 256, head_dim=32)  # re-routed as the plain dX site: delta=None
    assert r.ours and r.site is gemm.DX
    r = _route(gemm.DX_ATTN, 131072, 768, 768, head_dim=32)  # ... under that site's size cap
    assert not r.ours and r.site is gemm.DX
    r = _route(gemm.DX_ATTN, 4096 + 512, 768, 768, seq_len=1024)  # head dim 64 but M % seq_len != 0
    assert not r.ours and r.site is gemm.DX_ATTN and r.warning is None
    assert not _route(gemm.DX_ATTN, 4096, 768, 800).ours  # N % 64 != 0
    assert not _route(gemm.DX_ATTN, 4096 + 512, 768, 768, policy="ours").ours


def test_warning_only_when_a_promise_is_broken():
    bad = (4096, 192, 768)
    assert _route(gemm.DX, *bad).warning is None
    assert _route(gemm.DX, *bad, policy="serial").warning is None
    assert _route(gemm.DX, *bad, policy="ours").warning == "GEMM dx K=192 N=768 (needs K % 64 == 0, K >= 256, N % 8 == 0)"
    assert _route(gemm.DX, 4096, 768, 768, policy="ours", aligned=False).warning == (
        "GEMM dx with an operand not 16-byte aligned")
    assert _route(gemm.DX, 4096, 768, 768, policy="ours").warning is None
    # warn-always sites: the serial schedule promises them too
    assert _route(gemm.DX_GD, *bad).warning is None
    assert _route(gemm.DX_GD, *bad, policy="serial").warning == (
        "GEMM MLP-projection dX * gelu' K=192 N=768 (needs K % 64 == 0, K >= 256, N % 8 == 0)")
    assert _route(gemm.HEAD_LOGITS, *bad, policy="serial").warning.startswith("GEMM LM-head logits K=192 N=768 (needs")
    assert _route(gemm.HEAD_DX, *bad, policy="serial").warning == "LM-head dX K=192 N=768"
    assert _route(gemm.HEAD_DX, 4096, 50304, 768, policy="ours", aligned=False).warning == "LM-head dX K=50304 N=768"
    # the size cap and the NEVER knob break no promise
    assert _route(gemm.FWD, 131072, 768, 2304, policy="serial").warning is None


SITES = [gemm.FWD, gemm.FWD_GELU, gemm.FWD_GELU_GD, gemm.DX, gemm.DX_GELU, gemm.DX_GD, gemm.DX_ATTN,
         gemm.HEAD_LOGITS, gemm.HEAD_DX]


def test_sites_and_epilogues():
    assert [int(e) for e in Epilogue] == [0, 1, 2, 3, 4, 5]
    assert len({s.tag for s in SITES}) == len(SITES)
    assert {s.tag for s in SITES if s.size_routed} == {"fwd", "fwd_gelu", "dx", "dx_gelu", "dx_attn"}
    assert all(s.warn_always and s.unit_stride for s in SITES if not s.size_routed)
    assert [s for s in SITES if s.det_only] == [gemm.HEAD_LOGITS, gemm.HEAD_DX]


@pytest.mark.parametrize("policy", ["fast", "serial", "ours"])
def test_allow_ours_false_keeps_every_site_on_the_library(policy):
    for site in SITES:
        r = _route(site, 4096, 768, 768, policy=policy, allow_ours=False)
        assert not r.ours and r.warning is None


def test_row_chunks():
    assert gemm.row_chunks(350208, 768, 3072, Epilogue.BIAS) == [(0, 349440), (349440, 350208)]
    assert gemm.row_chunks(131072, 768, 768, Epilogue.ATTN_DELTA, 1024) == [(0, 131072)]
    head = gemm.row_chunks(131072, 768, 50304, Epilogue.BIAS, max_rows=gemm.HEAD_LOGITS.max_rows)
    assert head == [(16384 * i, 16384 * (i + 1)) for i in range(8)]
    ragged = gemm.row_chunks(40000, 50304, 768, Epilogue.BIAS, max_rows=gemm.HEAD_DX.max_rows)
    assert ragged == [(0, 16384), (16384, 32768), (32768, 40000)]
    # attention-delta chunks are whole sequences; a lowered limit chunks a small GEMM
    assert gemm.row_chunks(40960, 256, 256, Epilogue.ATTN_DELTA, 64, offset_limit=2 * 256 * 16384 + 1) == [
        (0, 16384), (16384, 32768), (32768, 40960)]
    assert gemm.row_chunks(1000, 256, 200, Epilogue.BIAS, offset_limit=2 * 256 * 256 + 1) == [
        (0, 256), (256, 512), (512, 768), (768, 1000)]
    assert gemm.row_chunks(0, 768, 768, Epilogue.BIAS) == [(0, 0)]  # still one (empty) launch
