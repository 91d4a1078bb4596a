"""-m gpu: gaviko_amd.features on ViT-T/16 models -- embed against the reference fixtures of tools/gen_features_golden.py on both
precision paths, the bit-level promises (logits and pooled of the plain inference forward, layer subsets, chunk sizes, plan replay),
non-interference with a pending backward, the kNN / prototype probes end to end, and the documented errors."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import golden
from gaviko_amd import features
from gaviko_amd.lib import GavikoHipError
from test_features_golden import METHODS as FIXTURES
from test_features_golden import class_means64, scores64, topk64, vote64
from test_input_grad_gpu import GAVIKO, build, volumes

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("GAVIKO_FEATURES_REPORT")            # profiles/features_parity_report.txt is a copy of what this run writes there
BIT_METHODS = [("gaviko", dict(GAVIKO)), ("deep_vpt", dict(num_prompts=8, prompt_dim=64, prompt_dropout=0.0, freeze_vit=True, deep_prompt=True)),
               ("evp", dict(freeze_vit=True))]


def report(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("method", FIXTURES)
def test_embed_matches_reference_fixture_fp32_and_bf16(dev, method):
    """fp32 path: pooled, cls, patch_mean (and the logits) within 1e-5 of the tensor's largest element, the bound
    tests/test_model_gpu.py::test_fp32_path_vs_golden applies.  bf16 path: within max(1e-2, 1.25 x the fixture's recorded bf16 floor of that
    tensor), relative to the tensor's largest element (the rule of tests/test_model_gpu.py)."""
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    g = golden(f"features_{method}_t16_b2")
    cfg = dict(ast.literal_eval(str(g["meta/cfg"])), precision="fp32")
    B = int(g["meta/batch"])
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).eval()
    x = torch.from_numpy(synth.volumes(0, B)).to(dev)
    fails = []
    for prec in ("fp32", "bf16"):
        if prec == "bf16":
            m.set_precision("bf16")
        assert m._engine().fp32 == (prec == "fp32")
        e = features.embed(m, x, layers="all")
        assert e.layers == tuple(range(m._engine().depth + 1))
        for key, got in (("pooled", e.pooled), ("logits", e.logits), ("cls", e.cls), ("patch_mean", e.patch_mean)):
            want = g[key].astype(np.float64)
            assert tuple(got.shape) == want.shape and got.dtype == torch.float32
            err = float(np.abs(got.double().cpu().numpy() - want).max())
            scale = float(np.abs(want).max())
            tol = 1e-5 if prec == "fp32" else max(1e-2, 1.25 * float(g["floor/" + key]))
            report(f"{method} {prec} {key}: abs {err:.3e}  rel {err / scale:.3e}  (bound {tol:.3e}, floor {float(g['floor/' + key]):.3e})")
            if err / scale > tol:
                fails.append((prec, key, err / scale, tol))
    assert not fails, fails


@pytest.mark.parametrize("method,extra", BIT_METHODS, ids=[m for m, _ in BIT_METHODS])
def test_bit_level_promises(dev, method, extra):
    B = 2
    x, _ = volumes(B)
    m, cfg = build(method, extra, dev)
    m.eval()
    xd = x.to(dev)
    eng = m._engine()
    with torch.no_grad():
        direct = m(xd).clone()
    plain = features.embed(m, xd)
    assert plain.layers == () and plain.cls is None and plain.patch_mean is None
    assert torch.equal(plain.logits, direct)
    eng.eval_forward(xd)
    assert torch.equal(plain.pooled, eng.workspace(B, xd.device, False)["pooled"])
    full = features.embed(m, xd, layers="all")                                    # the last layer runs every row in this plan
    assert torch.equal(full.logits, direct) and torch.equal(full.pooled, plain.pooled)
    assert tuple(full.cls.shape) == tuple(full.patch_mean.shape) == (eng.depth + 1, B, eng.C)
    sub = features.embed(m, xd, layers=(0, 5, 12))
    assert sub.layers == (0, 5, 12)
    assert torch.equal(sub.cls, full.cls[[0, 5, 12]]) and torch.equal(sub.patch_mean, full.patch_mean[[0, 5, 12]])
    assert torch.equal(sub.logits, direct) and torch.equal(sub.pooled, plain.pooled)
    for _ in range(3):                                                            # past the eager warm-up: recorded, then replayed
        again = features.embed(m, xd, layers="all")
        for a, b in zip((again.pooled, again.logits, again.cls, again.patch_mean), (full.pooled, full.logits, full.cls, full.patch_mean)):
            assert torch.equal(a, b)
    # the prune setting of every other plan is as it was
    with torch.no_grad():
        assert torch.equal(m(xd), direct)


def test_chunk_sizes_are_bit_identical(dev):
    x, _ = volumes(5)
    m, cfg = build("gaviko", dict(GAVIKO), dev)
    m.eval()
    xd = x.to(dev)
    ref = features.embed(m, xd, layers=(0, 12), batch=1)
    for bs in (2, 3, None):
        e = features.embed(m, xd, layers=(0, 12), batch=bs)
        for a, b in zip((e.pooled, e.logits, e.cls, e.patch_mean), (ref.pooled, ref.logits, ref.cls, ref.patch_mean)):
            assert tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), bs


@pytest.mark.parametrize("method,extra", BIT_METHODS[:2], ids=[m for m, _ in BIT_METHODS[:2]])
def test_embed_leaves_flags_gradients_and_a_pending_backward_alone(dev, method, extra):
    B = 2
    x, y = volumes(B)
    m, cfg = build(method, extra, dev)
    xd, yd = x.to(dev), y.to(dev)
    eng = m._engine()
    flags = lambda: [(n, mod.training) for n, mod in m.named_modules()]          # noqa: E731
    before = flags()

    def step(between):
        for p in m.parameters():
            p.grad = None
        eng.workspace(B, xd.device, True)["seed"].fill_(4242)
        loss = torch.nn.functional.cross_entropy(m(xd), yd)
        if between:
            features.embed(m, xd, layers="all")
            features.embed(m, xd)
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    ref = [step(False) for _ in range(3)][-1]
    for _ in range(3):
        got = step(True)
        assert got.keys() == ref.keys() and len(ref) > 0
        for n in ref:
            assert torch.equal(got[n], ref[n]), n
    assert flags() == before and any(f for _, f in before)
    held = {n: (p.grad, p.grad.clone()) for n, p in m.named_parameters() if p.grad is not None}
    flat = eng._flat_grad["buf"].clone() if eng._flat_grad is not None else None
    features.embed(m, xd, layers=(3,))
    for n, p in m.named_parameters():
        if n in held:
            assert p.grad is held[n][0] and torch.equal(p.grad, held[n][1]), n
        else:
            assert p.grad is None, n
    if flat is not None:
        assert torch.equal(eng._flat_grad["buf"], flat)
    assert flags() == before


def test_knn_probes_end_to_end(dev):
    """12 synth volumes -> a FeatureBank with labels i % 3; leave-one-out kNN and nearest-prototype against the float64 restatements on the
    downloaded features, compared wherever float64 is clear of the fp32 worst-case bound (the gap rule of the kernel tests)."""
    N, K, k = 12, 3, 3
    x, _ = volumes(N)
    m, cfg = build("linear", {}, dev)
    m.eval()
    e = features.embed(m, x.to(dev), batch=4)
    labels = np.arange(N) % K
    bank = features.FeatureBank(e.pooled.shape[1], dev)
    bank.add(e.pooled[:8], labels[:8]).add(e.pooled[8:], torch.from_numpy(labels[8:]))
    assert len(bank) == N and bank.labels.dtype == torch.int32 and torch.equal(bank.features, e.pooled)
    C = bank.dim
    U = 2.0 ** -24
    fn = bank.normalized().cpu().numpy()
    for metric, rows in (("cosine", fn), ("l2", bank.features.cpu().numpy())):
        r = features.knn_classify(bank, bank, bank.labels, k, K, metric=metric, exclude_self=True)
        kind = "l2" if metric == "l2" else "ip"
        want_i, want_s = topk64(rows, rows, k + 1, kind, exclude=np.arange(N))
        bound = (C * U * (np.abs(rows).astype(np.float64) @ np.abs(rows).astype(np.float64).T)).max() * (3.0 if kind == "l2" else 1.0)
        gap_hi = np.abs(np.diff(want_s, axis=1))
        gap_lo = np.concatenate([np.full((N, 1), np.inf), gap_hi[:, :-1]], 1)
        clear = (gap_hi > 2 * bound) & (gap_lo > 2 * bound)
        got_i = r.idx.cpu().numpy()
        assert not (got_i == np.arange(N)[:, None]).any()
        assert np.array_equal(got_i[clear], want_i[:, :k][clear])
        s64 = scores64(rows, rows, kind)
        assert (np.abs(r.score.double().cpu().numpy() - np.take_along_axis(s64, got_i.astype(np.int64), 1)) <= bound).all()
        full = clear.all(1)
        report(f"knn end to end {metric}: {int(clear.sum())} of {N * k} neighbours and {int(full.sum())} of {N} votes compared (bound {bound:.3e})")
        want_p, want_c = vote64(want_i[:, :k], want_s[:, :k], labels, K, "uniform")
        assert np.array_equal(r.probs.cpu().numpy()[full], want_p.astype(np.float32)[full])
        assert np.array_equal(r.pred.cpu().numpy()[full], want_c[full])
        assert np.abs(r.probs.sum(1).cpu().numpy() - 1).max() < 1e-6
    # nearest prototype on the bank's own prototypes
    protos = features.prototypes(bank.features, bank.labels, K)
    want_m, want_c = class_means64(bank.features.cpu().numpy(), labels, K)
    assert protos.count.tolist() == want_c.tolist() == [4, 4, 4]
    assert np.abs(protos.mean.double().cpu().numpy() - want_m).max() <= 4 * U * np.abs(bank.features.cpu().numpy()).max()
    pred, score = features.nearest_prototype(bank.features, protos, metric="l2")
    pm = protos.mean.cpu().numpy()
    s64 = scores64(bank.features.cpu().numpy(), pm, "l2")
    f = bank.features.cpu().numpy()
    b2 = 3 * C * U * (np.abs(f).astype(np.float64) @ np.abs(pm).astype(np.float64).T).max()
    assert tuple(score.shape) == (N, K) and (np.abs(score.double().cpu().numpy() - s64) <= b2).all()
    srt = np.sort(s64, axis=1)
    sure = (srt[:, 1] - srt[:, 0]) > 2 * b2
    assert np.array_equal(pred.cpu().numpy()[sure], s64.argmin(1)[sure])
    # with an empty class: its column is NaN and it is never predicted
    p4 = features.prototypes(bank.features, bank.labels, K + 1)
    assert p4.count.tolist() == [4, 4, 4, 0] and torch.equal(p4.mean[3], torch.zeros(C, device=dev))
    pred4, score4 = features.nearest_prototype(bank.features, p4, metric="l2")
    assert torch.equal(pred4, pred) and bool(torch.isnan(score4[:, 3]).all()) and torch.equal(score4[:, :3], score)


def test_documented_errors(dev):
    x, _ = volumes(2)
    m, cfg = build("linear", {}, dev)
    m.eval()
    xd = x.to(dev)
    for f in (lambda: features.embed(m, x), lambda: features.embed(m, xd[:, :, :60]), lambda: features.embed(m, xd, layers=(13,)),
              lambda: features.embed(m, xd, layers=(5, 3)), lambda: features.embed(m, xd, layers="every"), lambda: features.embed(m, xd, batch=0),
              lambda: features.embed(m, xd.double()), lambda: m._engine().feature_forward(xd, (0, 0))):
        with pytest.raises(GavikoHipError):
            f()
    e = features.embed(m, xd, layers=(12,))
    assert tuple(e.cls.shape) == (1, 2, 192)
    for f in (lambda: features.FeatureBank(190, dev), lambda: features.FeatureBank(192, "cpu"),
              lambda: features.FeatureBank(192, dev).add(e.pooled.cpu()), lambda: features.FeatureBank(64, dev).add(e.pooled),
              lambda: features.knn(e.pooled, features.FeatureBank(192, dev), 1), lambda: features.knn(e.pooled, e.pooled, 3),
              lambda: features.knn(e.pooled, e.pooled, 2, exclude_self=True)):
        with pytest.raises(GavikoHipError):
            f()
    nb = features.knn(e.pooled, e.pooled, 1, exclude_self=True)
    assert nb.idx.flatten().tolist() == [1, 0]
