"""CPU: the stored MWSA / GPA probability fixtures (tests/golden/gmaps_*.npz, tools/gen_gaviko_maps_golden.py) are consistent with
the window mask fixtures and with themselves, and the host functions reject what they document before touching a device."""
import ast

import numpy as np
import pytest

from conftest import golden

CASES = ["gaviko_t16_b2", "gaviko_t16_b2_k366_p8", "gaviko_t16_b2_lat16", "gaviko_t16_b1_share2", "cfg2_gaviko_b16_b4"]


def _ends(z):
    L = int(z["meta/depth"])
    return (0, L - 1)


@pytest.mark.parametrize("case", CASES)
def test_contents(case):
    z = golden("gmaps_" + case)
    L, P, B = int(z["meta/depth"]), int(z["meta/num_prompts"]), int(z["meta/batch"])
    N = int(np.prod(z["meta/grid"]))
    layers = [int(i) for i in z["meta/layers"]]
    assert layers == (list(range(L)) if case != "cfg2_gaviko_b16_b4" else [0, L - 1])
    assert [int(q) for q in z["meta/rows"]][0] == 0 and len(z["meta/rows"]) == 2
    for i in layers:
        for k in ("local/all", "gpa/global_mean", "gpa/local_mean", "gpa/fused_mean"):
            assert z[f"{k}/layer{i}"].shape == (B, N) and z[f"{k}/layer{i}"].dtype == np.float32
            assert f"floor/{k}/layer{i}" in z.files
        assert z[f"gpa/importance/layer{i}"].shape == (B, P) and z[f"gpa/global_weight/layer{i}"].shape == (B,)
    nb = len(z["meta/block_prompts"])
    for i in _ends(z):
        for k in ("gpa/global", "gpa/local", "gpa/fused"):
            assert z[f"{k}/layer{i}"].shape == (B, nb, N)
    assert z["local_rollout"].shape == (B, N) and "floor/local_rollout" in z.files
    assert float(z["meta/softmax_dev"]) < 1e-6                      # float32 softmax of the reference against the float64 recomputation


@pytest.mark.parametrize("case", CASES)
def test_local_rows_follow_the_window_mask(case):
    z = golden("gmaps_" + case)
    lk = [int(v) for v in z["meta/window"]]
    allow = np.unpackbits(golden(f"mwsa_mask_{lk[0]}{lk[1]}{lk[2]}")["allow"], axis=1)[:, :1000].astype(bool)   # True = mask 0
    for i in _ends(z):
        for q in (int(v) for v in z["meta/rows"]):
            row = z[f"local/row{q}/layer{i}"].astype(np.float64)
            assert np.abs(row.sum(-1) - 1.0).max() < 1e-6
            assert ((row != 0) == allow[q][None, :]).all(), (case, i, q)
        # the mean over all query rows sums to 1 as well, and every key is inside somebody's window
        allm = z[f"local/all/layer{i}"].astype(np.float64)
        assert np.abs(allm.sum(-1) - 1.0).max() < 1e-6 and (allm > 0).all()


@pytest.mark.parametrize("case", CASES)
def test_fusion_identity_and_rollout(case):
    z = golden("gmaps_" + case)
    P = int(z["meta/num_prompts"])
    sel = [int(p) for p in z["meta/block_prompts"]]
    for i in _ends(z):
        g, l, f = (z[f"gpa/{k}/layer{i}"].astype(np.float64) for k in ("global", "local", "fused"))
        imp = z[f"gpa/importance/layer{i}"].astype(np.float64)[:, sel, None]
        gw = z[f"gpa/global_weight/layer{i}"].astype(np.float64)[:, None, None]
        assert np.abs(f - imp * (gw * g + (1 - gw) * l)).max() < 1e-6 * np.abs(f).max()
        assert (g[:, :, :P + 1] == 0).all() and (g[:, :, P + 1:] > 0).all()       # the double slice (gaviko.py:161,107)
        assert np.abs(g.sum(-1) - 1.0).max() < 1e-5 and np.abs(l.sum(-1) - 1.0).max() < 1e-5
        assert ((imp > 0) & (imp < 1)).all() and ((gw > 0) & (gw < 1)).all()
    for i in (int(v) for v in z["meta/layers"]):
        fm = z[f"gpa/fused_mean/layer{i}"].astype(np.float64)
        imp = z[f"gpa/importance/layer{i}"].astype(np.float64)
        assert np.abs(fm.sum(-1) - imp.mean(-1)).max() < 1e-6
    r = z["local_rollout"].astype(np.float64)
    assert np.abs(r.sum(-1) - 1.0).max() < 1e-6 and (r > 0).all()


def test_host_rejections_without_a_device():
    """Everything that does not need a launch is rejected on a CPU box too: a non-GAViKO model, a CPU input, bad rows / layer / start."""
    import torch
    from gaviko_amd import explain
    from gaviko_amd.lib import GavikoHipError
    from gaviko_amd.registry import build_model
    z = golden("gmaps_gaviko_t16_b2")
    cfg = ast.literal_eval(str(z["meta/cfg"]))
    model = build_model(cfg)
    x = torch.zeros((1, 1, 120, 160, 160))
    for fn in (explain.local_attention_maps, explain.gpa_attention_maps, explain.local_rollout):
        with pytest.raises(GavikoHipError, match="HIP device"):
            fn(model, x)
    with pytest.raises(GavikoHipError, match="query row"):
        explain.local_attention_maps(model, x, rows=1000)
    with pytest.raises(GavikoHipError, match="rows="):
        explain.local_attention_maps(model, x, rows="pool")
    with pytest.raises(GavikoHipError, match="layer="):
        explain.local_rollout(model, x, layer=12)
    with pytest.raises(GavikoHipError, match="start="):
        explain.local_rollout(model, x, start=[1.0])
    plain = build_model(ast.literal_eval(str(golden("attn_cfg1_linear_t16_b1")["meta/cfg"])))
    for fn in (explain.local_attention_maps, explain.gpa_attention_maps, explain.local_rollout):
        with pytest.raises(GavikoHipError, match="GAViKO models only"):
            fn(plain, x)
    # the global functions keep refusing the side-path attentions
    for which in ("local", "gpa"):
        with pytest.raises(GavikoHipError, match="global self-attention"):
            explain.attention_maps(model, x, attention=which)
