"""CPU: the feature fixtures (tools/gen_features_golden.py: the REFERENCE classes' head input and logits, and the per-layer CLS row and
patch-row mean of the oracle's streams) are rebuilt here from the oracle's taps with the documented row rule, which pins that rule --
deep VPT's shrinking sequence and DVPT's row 0 included -- on any machine.  Also the float64 numpy restatements of gvk_feature_topk,
gvk_knn_vote and gvk_class_means with their tie rules, which the GPU tests import, checked against sklearn where sklearn has no ties."""
import ast

import numpy as np
import pytest
import torch

import oracle
from conftest import golden
from gaviko_amd.utils import synth
from oracle import vit_ref

METHODS = ["gaviko", "linear", "deep_vpt", "dvpt"]


def load(method):
    g = golden(f"features_{method}_t16_b2")
    return g, ast.literal_eval(str(g["meta/cfg"])), int(g["meta/batch"])


# ------------------------------------------------------------------ float64 restatements (imported by the GPU tests)
def scores64(q, g, metric):
    """[Nq, Ng] float64: metric 'ip' q . g; 'l2' ||q||^2 + ||g||^2 - 2 q . g (as the kernel states it)."""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    s = q @ g.T
    if metric == "l2":
        s = (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2.0 * s
    return s


def topk64(q, g, k, metric="ip", exclude=None):
    """-> (idx int64 [Nq, k], score float64 [Nq, k]), best first ('ip': larger, 'l2': smaller); an exact tie goes to the lower bank
    index (a stable sort of the keys).  exclude [Nq]: one bank index per query that is skipped (-1: none)."""
    s = scores64(q, g, metric)
    key = -s if metric == "ip" else s.copy()
    if exclude is not None:
        for n, e in enumerate(np.asarray(exclude)):
            if e >= 0:
                key[n, e] = np.inf
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(s, order, 1)


def vote64(idx, score, labels, K, mode="uniform", temperature=0.07):
    """-> (probs float64 [Nq, K], pred int64 [Nq]).  uniform: votes / k; softmax: w_j = exp((score_j - score_0) / T), normalised, summed in
    rank order.  T is the fp32 value the kernel receives.  pred: np.argmax, the first (lowest) maximum."""
    idx, score, labels = np.asarray(idx), np.asarray(score, np.float64), np.asarray(labels)
    Nq, k = idx.shape
    probs = np.zeros((Nq, K))
    T = float(np.float32(temperature))
    for n in range(Nq):
        tot = 0.0
        for j in range(k):
            w = 1.0 if mode == "uniform" else float(np.exp((score[n, j] - score[n, 0]) / T))
            probs[n, labels[idx[n, j]]] += w
            tot += w
        probs[n] /= (k if mode == "uniform" else tot)
    return probs, probs.argmax(1)


def class_means64(x, labels, K):
    x, labels = np.asarray(x, np.float64), np.asarray(labels)
    mean, count = np.zeros((K, x.shape[1])), np.zeros(K, dtype=np.int64)
    for c in range(K):
        sel = labels == c
        count[c] = sel.sum()
        if count[c]:
            mean[c] = x[sel].sum(0) / count[c]
    return mean, count


# ------------------------------------------------------------------ the row rule, restated
def stream_rows(method, cfg, sd, x, taps):
    """(cls [B, C], patch rows [B, n_l, C]) of the global token stream ENTERING layer l, l = 0 .. depth (depth: the last layer's output),
    from the oracle's embedding output and its layer{i}.post_mlp taps.  cls: row 0 for [cls | ...] layouts, row P for [P prompts | cls |
    patches] (GAViKO, DVPT).  Patch rows: everything behind row_off = 1 (plain), 1 + P (VPT), P + 1 (GAViKO, DVPT) -- of the layer's OWN
    sequence: deep VPT rebuilds it as [cls | P new prompts | previous[:, 1 + prompt_dim:]] in front of every layer i > 0 (vpt.py:147-153)."""
    depth = vit_ref.mapping_vit(cfg["backbone"])[0]
    patch = (cfg["frame_patch_size"], cfg["image_patch_size"], cfg["image_patch_size"])
    P = cfg.get("num_prompts", 0)
    if method == "gaviko":
        e = taps["embed.global"]
        rows = [(e[:, P], e[:, P + 1:])]
    elif method == "dvpt":
        pos = sd["pos_embedding"]
        rows = [((sd["cls_token"] + pos[:, :1])[:, 0].expand(x.shape[0], -1), vit_ref.patch_embed(sd, "conv_proj.0", x, patch) + pos[:, 1:])]
    else:
        e = vit_ref.embed_tokens(sd, x, patch, "vision_transformer." if method == "deep_vpt" else "")
        rows = [(e[:, 0], e[:, 1:])]
    for l in range(1, depth + 1):
        t = taps[f"layer{l - 1}.post_mlp"]
        if method in ("gaviko", "dvpt"):
            rows.append((t[:, P], t[:, P + 1:]))
        elif method == "deep_vpt":
            rows.append((t[:, 0], t[:, 1 + (cfg["prompt_dim"] if l < depth else P):]))
        else:
            rows.append((t[:, 0], t[:, 1:]))
    return rows


def pooled_rows(method, cfg, final_norm):
    """The rows of the final LayerNorm the head pools -> [B, C] float64."""
    fn = final_norm.double()
    if method == "gaviko":
        return fn[:, : cfg["num_prompts"] + 1].mean(1)
    return fn.mean(1) if cfg.get("pool", "cls") == "mean" else fn[:, 0]


_RUNS = {}


def oracle_run(method):
    """One oracle forward per method, shared by the tests below."""
    if method not in _RUNS:
        g, cfg, B = load(method)
        sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(oracle.SHAPES[method](cfg)).items()}
        x = torch.from_numpy(synth.volumes(0, B))
        taps = {}
        with torch.no_grad():
            logits = oracle.FORWARD[method](sd, x, cfg, taps)
            rows = stream_rows(method, cfg, sd, x, taps)
        _RUNS[method] = (logits, taps, rows)
    return _RUNS[method]


@pytest.mark.parametrize("method", METHODS)
def test_oracle_pooled_rows_reproduce_the_head_input(method):
    g, cfg, B = load(method)
    dev = float(g["meta/oracle_dev"])
    assert dev <= 2e-5
    logits, taps, _ = oracle_run(method)
    pooled = pooled_rows(method, cfg, taps["final_norm"]).numpy()
    e_p = float(np.abs(pooled - g["pooled"]).max())
    e_l = float(np.abs(logits.double().numpy() - g["logits"]).max())
    print(f"features_{method}: pooled {e_p:.3e}, logits {e_l:.3e} (recorded oracle deviation {dev:.3e})")
    assert g["pooled"].shape == (B, 192) and g["pooled"].dtype == np.float32
    assert e_p <= max(dev, 1e-6) * 1.0000001 and e_l <= max(dev, 1e-6) * 1.0000001


@pytest.mark.parametrize("method", METHODS)
def test_layer_summaries_follow_the_row_rule(method):
    g, cfg, B = load(method)
    _, _, rows = oracle_run(method)
    depth = vit_ref.mapping_vit(cfg["backbone"])[0]
    assert g["cls"].shape == g["patch_mean"].shape == (depth + 1, B, 192) and g["cls"].dtype == np.float64
    cls = np.stack([c.double().numpy() for c, _ in rows])
    pm = np.stack([p.double().mean(1).numpy() for _, p in rows])
    assert [p.shape[1] for _, p in rows] == g["meta/patch_rows"].tolist()
    # the same fp32 oracle on the same inputs; only the BLAS threading of the machine may differ from the generator's
    assert np.abs(cls - g["cls"]).max() <= 2e-5 and np.abs(pm - g["patch_mean"]).max() <= 2e-5
    N = 1000
    if method == "deep_vpt":                                                      # quirk 16: 64 - 8 rows fewer in front of every layer i > 0
        assert g["meta/patch_rows"].tolist() == [N - 56 * l for l in range(depth)] + [N - 56 * (depth - 1)]
    else:
        assert g["meta/patch_rows"].tolist() == [N] * (depth + 1)
    if method == "dvpt":                                                          # row 0 is a prompt: the CLS row is row P, not the pooled row
        _, taps, _ = oracle_run(method)
        t = taps[f"layer{depth - 1}.post_mlp"].double().numpy()
        assert np.abs(t[:, 0] - g["cls"][depth]).max() > 1e-3 and np.abs(t[:, cfg["num_prompts"]] - g["cls"][depth]).max() <= 2e-5
    for k in ("pooled", "logits", "cls", "patch_mean"):
        assert 0.0 < float(g["floor/" + k]) < 5e-2, k


# ------------------------------------------------------------------ the restatements against sklearn
def test_topk64_matches_sklearn_brute_force():
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(1)
    q, g = rng.standard_normal((23, 48)), rng.standard_normal((301, 48))
    nn = NearestNeighbors(n_neighbors=7, algorithm="brute", metric="euclidean").fit(g)
    dist, ind = nn.kneighbors(q)
    idx, score = topk64(q, g, 7, "l2")
    assert np.array_equal(idx, ind)
    assert np.abs(np.sqrt(np.maximum(score, 0)) - dist).max() < 1e-10
    # normalised rows: the inner-product order is the euclidean order
    qn, gn = q / np.linalg.norm(q, axis=1, keepdims=True), g / np.linalg.norm(g, axis=1, keepdims=True)
    _, ind = NearestNeighbors(n_neighbors=7, algorithm="brute", metric="euclidean").fit(gn).kneighbors(qn)
    assert np.array_equal(topk64(qn, gn, 7, "ip")[0], ind)
    # leave-one-out on the bank: sklearn's kneighbors() without an argument skips the row itself
    _, ind = nn.kneighbors()
    assert np.array_equal(topk64(g, g, 7, "l2", exclude=np.arange(301))[0], ind)


def test_restated_tie_rules():
    g = np.array([[1.0, 0], [0, 1], [1, 0], [0, 1], [2, 0]])
    q = np.array([[1.0, 0]])
    idx, score = topk64(q, g, 4, "ip")
    assert idx.tolist() == [[4, 0, 2, 1]] and score.tolist() == [[2, 1, 1, 0]]
    idx, score = topk64(q, g, 3, "l2", exclude=[0])
    assert idx.tolist() == [[2, 4, 1]] and score.tolist() == [[0, 1, 2]]
    probs, pred = vote64(np.array([[0, 1, 2, 3, 4]]), np.zeros((1, 5)), np.array([2, 1, 2, 1, 0]), 3)     # a 2-2-1 vote: the lower class
    assert probs.tolist() == [[0.2, 0.4, 0.4]] and pred.tolist() == [1]
    mean, count = class_means64(g, np.array([0, 2, 0, 2, 0]), 3)
    assert count.tolist() == [3, 0, 2] and mean[1].tolist() == [0, 0] and np.allclose(mean[0], [4 / 3, 0])


def test_integer_case_has_ties_inside_the_top_11():
    """The first integer shape of tests/test_features_kernels_gpu.py exercises the tie rule: many queries have equal scores among their
    best 11."""
    from test_features_kernels_gpu import integer_case
    q, g = integer_case(37, 533, 1024, 0)
    s = np.sort(-scores64(q, g, "ip"), axis=1)[:, :11]
    tied = int((np.diff(s, axis=1) == 0).any(1).sum())
    print(f"integer case: {tied} of 37 queries have a tie inside their top 11")
    assert tied >= 10
