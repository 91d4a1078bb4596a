"""CPU: the attention-map fixtures generated from the reference (tools/gen_attention_golden.py) are self-consistent, the pooled rows the
explanation API selects are the rows the reference's head pools, and the API's rejections fire before anything is launched."""
import ast

import numpy as np
import pytest
import torch

from conftest import golden

CASES = ["gaviko_t16_b2", "cfg1_linear_t16_b1", "dvpt_t16_b2_mean_p8", "deep_vpt_t16_b2", "cfg2_gaviko_b16_b4"]


def _model(z):
    from gaviko_amd.registry import build_model
    return build_model(ast.literal_eval(str(z["meta/cfg"])))


@pytest.mark.parametrize("case", CASES)
def test_fixture_invariants(case):
    z = golden("attn_" + case)
    B, H, Ts = int(z["meta/batch"]), int(z["meta/heads"]), [int(t) for t in z["meta/Ts"]]
    maps = [k for k in z.files if k.startswith(("pool/", "cls/"))]
    assert maps
    for k in maps:
        m = z[k].astype(np.float64)
        i = int(k.split("layer")[1])
        assert m.shape == (B, H, Ts[i]), k
        assert m.min() >= 0.0, k
        assert np.abs(m.sum(-1) - 1.0).max() < 1e-5, k          # a convex combination of rows of P: every head's map sums to 1
    if "rollout" in z.files:
        r = z["rollout"].astype(np.float64)
        assert r.shape == (B, Ts[0]) and r.min() >= 0.0
        assert np.abs(r.sum(-1) - 1.0).max() < 1e-5
    floors = [float(z[k]) for k in z.files if k.startswith("floor/")]
    assert floors and max(floors) < 2e-2                          # the bf16 operand floor stays below the tests' base bound


@pytest.mark.parametrize("case", CASES)
def test_pool_rows_match_reference_head(case):
    from gaviko_amd import explain
    z = golden("attn_" + case)
    eng = _model(z)._engine()
    assert list(eng.Ts) == [int(t) for t in z["meta/Ts"]]
    want = [int(r) for r in z["meta/pool_rows"]]
    for i in range(eng.depth):
        r0, R = explain._pool_range(eng, i)
        assert list(range(r0, r0 + R)) == (list(range(eng.Ts[i])) if want == [-1] else want)


def test_patch_grid_layout():
    from gaviko_amd import explain
    z = golden("attn_gaviko_t16_b2")
    model = _model(z)
    eng = model._engine()
    rel = torch.arange(2 * eng.T, dtype=torch.float32).reshape(2, eng.T)
    g = explain.patch_grid(model, rel)
    assert g.shape == (2,) + tuple(eng.grid)
    assert float(g[1, 0, 0, 0]) == eng.T + eng.row_off                 # first patch row of sample 1: after the prompts and the CLS row
    assert float(g[0, -1, -1, -1]) == eng.row_off + eng.N - 1
    with pytest.raises(Exception, match="patch_grid"):
        explain.patch_grid(model, rel[:, :-1])


def test_rejections_before_launch():
    from gaviko_amd import explain
    from gaviko_amd.lib import GavikoHipError
    model = _model(golden("attn_gaviko_t16_b2"))
    x = torch.zeros(1, 1, 120, 160, 160)
    with pytest.raises(GavikoHipError, match="HIP device"):
        explain.attention_maps(model, x)
    with pytest.raises(GavikoHipError, match="HIP device"):
        explain.attention_rollout(model, x)
    for which in ("local", "gpa"):
        with pytest.raises(GavikoHipError, match="global self-attention"):
            explain.attention_maps(model, x, attention=which)
    model.set_precision("fp32")
    with pytest.raises(GavikoHipError, match="fp32"):
        explain.attention_maps(model, x)
    with pytest.raises(GavikoHipError, match="fp32"):
        explain.attention_rollout(model, x)
    deep = _model(golden("attn_deep_vpt_t16_b2"))
    with pytest.raises(GavikoHipError, match="deep VPT"):
        explain.attention_rollout(deep, x)
