"""CPU: the attention-relevance fixtures generated from the reference (tools/gen_relevance_golden.py) are self-consistent, the API's
rejections fire before anything is launched, and the two ops wrappers reach exactly their kernels."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import golden
from test_kernel_coverage import PKG, _module_reach

CASES = ["gaviko_t16_b2", "cfg1_linear_t16_b1", "dvpt_t16_b2_mean_p8", "cfg2_gaviko_b16_b4"]


def _model(z):
    from gaviko_amd.registry import build_model
    return build_model(ast.literal_eval(str(z["meta/cfg"])))


def _w_pool(z):
    B, T = int(z["meta/batch"]), int(z["meta/Ts"][0])
    rows = [int(r) for r in z["meta/pool_rows"]]
    w = np.zeros((B, T))
    if rows == [-1]:
        w[:] = 1.0 / T
    else:
        w[:, rows] = 1.0 / len(rows)
    return w


@pytest.mark.parametrize("case", CASES)
def test_fixture_invariants(case):
    z = golden("relv_" + case)
    B, H, Ts = int(z["meta/batch"]), int(z["meta/heads"]), [int(t) for t in z["meta/Ts"]]
    L = len(Ts)
    assert len(set(Ts)) == 1
    w = _w_pool(z)
    floors = {k: float(z[k]) for k in z.files if k.startswith("floor/")}
    for tag in ("argmax", "alt"):
        r = z[f"relevance/{tag}"].astype(np.float64)
        assert r.shape == (B, Ts[0]), tag
        assert (r >= w - 1e-7).all(), tag                            # the identity term: r >= w_pool elementwise
        assert (r - w).max() > 0.0, tag
        for kind in ("operand", "weights"):
            assert f"floor/{kind}/relevance/{tag}" in floors
        assert z[f"meta/target_{tag}"].shape == (B,)
    for i in (0, L - 1):
        m = z[f"gradmaps/argmax/layer{i}"].astype(np.float64)
        assert m.shape == (B, H, Ts[i]), i
        assert m.min() >= 0.0 and m.max() > 0.0, i
        for kind in ("operand", "weights"):
            assert f"floor/{kind}/gradmaps/argmax/layer{i}" in floors
    assert z["logits"].shape[0] == B
    assert (z["logits"].argmax(1) == z["meta/target_argmax"]).all()
    assert (z["meta/target_argmax"] != z["meta/target_alt"]).all()
    # another class gives another map: the added parts differ by more than 10 x the larger floor of the two relevances
    a, b = z["relevance/argmax"].astype(np.float64) - w, z["relevance/alt"].astype(np.float64) - w
    rfloor = max(v for k, v in floors.items() if "/relevance/" in k)
    assert np.abs(a - b).max() / np.abs(a).max() > 10 * rfloor
    assert float(z["meta/dA_dev"]) < 1e-5                             # dA = dO . V^T against attend(...).grad
    assert max(floors.values()) < 2e-2, floors                        # every floor stays below the tests' base bound


def test_rejections_before_launch():
    from gaviko_amd import explain
    from gaviko_amd.lib import GavikoHipError
    model = _model(golden("relv_gaviko_t16_b2"))
    x = torch.zeros(1, 1, 120, 160, 160)
    for fn in (explain.attention_relevance, explain.attention_gradmaps):
        with pytest.raises(GavikoHipError, match="HIP device"):
            fn(model, x)
        for bad in (5, -1, True, 1.5, torch.tensor([0, 1]), torch.tensor([7]), torch.tensor([0.0])):
            with pytest.raises(GavikoHipError, match="target"):
                fn(model, x, target=bad)
        with pytest.raises(GavikoHipError, match="expected img"):
            fn(model, x[:, :, :-1])
        with pytest.raises(GavikoHipError, match="expected img"):
            fn(model, x[0])
        with pytest.raises(GavikoHipError, match="float32"):
            fn(model, x.double())
    with pytest.raises(GavikoHipError, match="rows"):
        explain.attention_gradmaps(model, x, rows=model._engine().T)
    with pytest.raises(GavikoHipError, match="rows"):
        explain.attention_gradmaps(model, x, rows="cls")
    model.set_precision("fp32")
    for fn in (explain.attention_relevance, explain.attention_gradmaps):
        with pytest.raises(GavikoHipError, match="fp32"):
            fn(model, x)
    deep = _model(golden("attn_deep_vpt_t16_b2"))
    with pytest.raises(GavikoHipError, match="deep VPT"):
        explain.attention_relevance(deep, x)
    with pytest.raises(GavikoHipError, match="HIP device"):           # the per-layer maps cover deep VPT: only the device is missing here
        explain.attention_gradmaps(deep, x)


def test_wrappers_reach_their_kernels():
    from gaviko_amd import ops
    assert callable(ops.attention_gradcolsum) and callable(ops.relevance_step)
    reach = _module_reach(os.path.join(PKG, "ops.py"))
    assert reach["attention_gradcolsum"] == {"gvk_attention_gradcolsum_bf16"}
    assert reach["relevance_step"] == {"gvk_relevance_step"}
    host = _module_reach(os.path.join(PKG, "explain.py"), reach)
    assert host["attention_rollout"] >= {"gvk_attention_colsum_bf16", "gvk_rollout_step"}      # the existing maps keep their kernels
    assert not host["attention_rollout"] & {"gvk_attention_gradcolsum_bf16", "gvk_relevance_step"}
