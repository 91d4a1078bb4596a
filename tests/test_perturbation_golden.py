"""CPU: the perturbation fixtures (tools/gen_perturbation_golden.py: the REFERENCE classes run on perturbed volumes built with numpy
indexing) are reproduced by the oracle on volumes this file perturbs itself, and the tie rule of the patch ranking is pinned."""
import ast

import numpy as np
import pytest
import torch

import oracle
from conftest import golden
from gaviko_amd.utils import synth

CASES = ["gaviko_t16_b2", "linear_t16_b2", "evp_t16_b2"]


def load(name):
    g = golden("perturb_" + name)
    cfg = ast.literal_eval(str(g["meta/cfg"]))
    return g, cfg, str(g["meta/method"]), int(g["meta/batch"])


def stable_rank(rel):
    """The inverse permutation of argsort(stable, descending), through the sort (the generator counts pairs instead)."""
    order = np.argsort(-rel, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(rel.shape[1]), order.shape), axis=1)
    return rank


def upsample(mask, grid, patch):
    m = torch.as_tensor(mask).view((mask.shape[0], 1) + tuple(grid))
    for ax, p in enumerate(patch):
        m = m.repeat_interleave(p, ax + 2)
    return m


@pytest.mark.parametrize("name", CASES)
def test_rank_rule_on_the_fixture_relevance(name):
    """rank[n] = #{m : rel[m] > rel[n]} + #{m < n : rel[m] == rel[n]} (counted pair by pair) == the stable descending argsort's inverse;
    the fixture's relevance has the ties and the block of exact zeros that make the rule matter."""
    g, cfg, method, B = load(name)
    rel = g["relevance"]
    N = rel.shape[1]
    assert (rel[:, : N // 8] == 0).all() and len(np.unique(rel)) <= 64            # ties everywhere
    idx = np.arange(N)
    pairs = (rel[:, None, :] > rel[:, :, None]).sum(2) + ((rel[:, None, :] == rel[:, :, None]) & (idx[None, None, :] < idx[None, :, None])).sum(2)
    rank = stable_rank(rel)
    assert (rank == pairs).all()
    assert (np.sort(rank, axis=1) == idx).all()                                   # a permutation
    zeros = rank[:, : N // 8]                                                     # the zero block: last in the order, in patch order
    assert (np.diff(zeros, axis=1) > 0).all()


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_on_perturbed_volumes(name):
    """Within the bound tests/test_oracle_vs_golden.py applies to logits (2e-5 absolute); the generator measured meta/oracle_dev."""
    g, cfg, method, B = load(name)
    assert float(g["meta/oracle_dev"]) < 2e-5
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(oracle.SHAPES[method](cfg)).items()}
    x = torch.from_numpy(synth.volumes(0, B))
    patch = (cfg["frame_patch_size"], cfg["image_patch_size"], cfg["image_patch_size"])
    grid = tuple(s // p for s, p in zip(x.shape[2:], patch))
    rank = stable_rank(g["relevance"])
    ks = g["ks"]
    fills = {"min": x.reshape(B, -1).amin(1).view(B, 1, 1, 1, 1).expand_as(x), "vol": torch.from_numpy(synth.volumes(100, 1)).expand_as(x)}

    def run(vol):
        with torch.no_grad():
            return oracle.FORWARD[method](sd, vol.contiguous(), cfg, None).numpy()

    worst = np.abs(run(x) - g["logits"]).max()
    for tag, fill in fills.items():
        for s in range(len(ks)):
            top = upsample(rank < ks[s], grid, patch)
            worst = max(worst, np.abs(run(torch.where(top, fill, x)) - g[f"deletion_{tag}"][:, s]).max())
            worst = max(worst, np.abs(run(torch.where(top, x, fill)) - g[f"insertion_{tag}"][:, s]).max())
    for w in range(len(g["occlusion_boxes"])):
        d0, d1, h0, h1, w0, w1 = g["occlusion_boxes"][w]
        m = np.zeros((B,) + grid, dtype=bool)
        m[:, d0:d1, h0:h1, w0:w1] = True
        worst = max(worst, np.abs(run(torch.where(upsample(m, grid, patch), fills["min"], x)) - g["occlusion_min"][:, w]).max())
    print(f"perturb_{name}: oracle vs reference fixture, max |dlogit| = {worst:.3e}")
    assert worst < 2e-5
    # the structure the curves promise: deletion at k = 0 is the plain volume, insertion at k = N too
    assert np.array_equal(g["deletion_min"][:, 0], g["logits"]) and np.array_equal(g["insertion_min"][:, -1], g["logits"])
    assert np.array_equal(g["deletion_min"][:, -1], g["insertion_min"][:, 0])
