"""CPU: the uncertainty fixtures (tools/gen_uncertainty_golden.py: the REFERENCE classes in eval mode on the synth volumes under all 8 axis
flips, and the float64 predictive statistics of those logits) are reproduced by the oracle on volumes this file flips itself, and by a
plain float64 numpy restatement of the statistics gvk_predictive_stats is specified to write."""
import ast

import numpy as np
import pytest
import torch

import oracle
from conftest import golden
from gaviko_amd.utils import synth

METHODS = ["gaviko", "linear", "evp"]


def load(method):
    g = golden(f"uncertainty_tta_{method}_t16")
    return g, ast.literal_eval(str(g["meta/cfg"])), int(g["meta/batch"])


def stats64(logits):
    """The formulas of include/gaviko_hip.h (gvk_predictive_stats) in float64 numpy.  logits [B, S, K]."""
    z = np.asarray(logits, dtype=np.float64)
    B, S, K = z.shape
    e = np.exp(z - z.max(2, keepdims=True))
    p = e / e.sum(2, keepdims=True)
    mean = p.sum(1) / S

    def H(q):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(q > 0, -q * np.log(np.where(q > 0, q, 1.0)), 0.0).sum(-1)

    entropy, expected = H(mean), H(p).sum(1) / S
    votes = np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        for s in range(S):
            votes[b, int(np.argmax(z[b, s]))] += 1                                # np.argmax: the first maximum
    return {"probs": mean, "pred": np.argmax(mean, 1), "entropy": entropy, "expected_entropy": expected,
            "mutual_info": np.maximum(entropy - expected, 0.0), "std": np.sqrt(((p - mean[:, None]) ** 2).sum(1) / S), "votes": votes,
            "variation_ratio": 1.0 - votes.max(1) / S}


@pytest.mark.parametrize("method", METHODS)
def test_oracle_reproduces_the_reference_on_flipped_volumes(method):
    """Within the bound tests/test_oracle_vs_golden.py applies to logits (2e-5 absolute); the generator measured meta/oracle_dev."""
    g, cfg, B = load(method)
    assert float(g["meta/oracle_dev"]) < 2e-5
    assert g["flips"].tolist() == list(range(8)) and g["logits"].shape == (B, 8, cfg["num_classes"])
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(oracle.SHAPES[method](cfg)).items()}
    x = torch.from_numpy(synth.volumes(0, B))
    worst = 0.0
    for s, code in enumerate(g["flips"].tolist()):
        dims = [a + 2 for a in range(3) if code >> a & 1]
        xt = torch.flip(x, dims).contiguous() if dims else x
        with torch.no_grad():
            got = oracle.FORWARD[method](sd, xt, cfg, None).numpy()
        worst = max(worst, np.abs(got - g["logits"][:, s]).max())
    print(f"uncertainty_tta_{method}: oracle vs reference fixture, max |dlogit| = {worst:.3e}")
    assert worst < 2e-5
    # the flips matter: the members of one volume are not copies of each other
    assert np.abs(g["logits"] - g["logits"][:, :1]).max() > 1e-3


@pytest.mark.parametrize("method", METHODS)
def test_float64_restatement_reproduces_the_stored_statistics(method):
    g, cfg, B = load(method)
    want = stats64(g["logits"])
    for k, v in want.items():
        got = g["stats/" + k]
        if k in ("pred", "votes"):
            assert np.array_equal(got, v), k
        else:
            assert got.dtype == np.float64 and np.abs(got - v).max() < 1e-12, (k, np.abs(got - v).max())
    assert (g["stats/votes"].sum(1) == 8).all()
    assert (g["stats/mutual_info"] >= 0).all() and (g["stats/entropy"] <= np.log(cfg["num_classes"]) + 1e-12).all()
    assert np.abs(g["stats/probs"].sum(1) - 1).max() < 1e-12
