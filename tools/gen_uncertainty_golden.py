#!/usr/bin/env python3
"""Generate tests/golden/uncertainty_tta_<method>_t16.npz by RUNNING THE REFERENCE classes (imported as tools/gen_golden.py does) in eval
mode on the B = 2 synth volumes under all 8 axis flips (torch.flip; member s of a volume is the flip whose code s = sum(1 << axis) over
(0, 1, 2) = (D, H, W)).

Volumes are not stored (synth regenerates them).  Each file holds the reference's logits [B, 8, K], the largest deviation of the oracle on
the same flipped volumes, and the float64 predictive statistics of those logits computed here with plain torch: mean member softmax, its
argmax, H[mean p], the mean member entropy, their difference clamped at 0, the population std, the members' argmax votes and the variation
ratio -- what gvk_predictive_stats is specified to write.

Only runs where the reference is present (the build container).  Usage:  python tools/gen_uncertainty_golden.py [method ...]
"""
from __future__ import annotations

import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from gaviko_amd.utils import synth  # noqa: E402
from gen_golden import BASE, GAVIKO, build_reference, import_reference  # noqa: E402

CASES = {
    "gaviko": dict(GAVIKO),
    "linear": {},
    "evp": dict(freeze_vit=True),
}
B = 2
FLIPS = [tuple(a for a in range(3) if code >> a & 1) for code in range(8)]


def stats64(logits):
    """logits [B, S, K] -> the float64 statistics, plain torch."""
    z = torch.as_tensor(logits).double()
    S, K = z.shape[1], z.shape[2]
    p = torch.softmax(z, dim=2)
    mean = p.mean(1)
    plogp = lambda q: torch.where(q > 0, -q * torch.log(q.clamp_min(1e-300)), torch.zeros_like(q))       # noqa: E731
    entropy = plogp(mean).sum(1)
    expected = plogp(p).sum(2).mean(1)
    votes = torch.nn.functional.one_hot(z.argmax(2), K).sum(1)
    return {"probs": mean, "pred": mean.argmax(1), "entropy": entropy, "expected_entropy": expected,
            "mutual_info": (entropy - expected).clamp_min(0), "std": p.std(1, unbiased=False), "votes": votes,
            "variation_ratio": 1.0 - votes.max(1).values.double() / S}


def run_case(mods, method, outdir):
    import oracle

    cfg = dict(BASE, backbone="vit-t16", method=method, **CASES[method])
    t0 = time.time()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            model = build_reference(mods, method, cfg)
        finally:
            os.chdir(cwd)
    sd = model.state_dict()
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    model.eval()
    osd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.from_numpy(synth.volumes(0, B))
    logits, dev = [], 0.0
    for axes in FLIPS:
        xt = torch.flip(x, [a + 2 for a in axes]).contiguous() if axes else x
        with torch.no_grad():
            ref = model(xt)
            orc = oracle.FORWARD[method](osd, xt, cfg, None)
        dev = max(dev, (orc - ref).abs().max().item())
        logits.append(ref.numpy().copy())
    logits = np.stack(logits, 1)                                                  # [B, 8, K]
    assert dev < 2e-5, dev
    out = {"meta/method": method, "meta/backbone": "vit-t16", "meta/batch": B, "meta/cfg": repr(dict(cfg)), "meta/oracle_dev": np.float64(dev),
           "flips": np.array([sum(1 << a for a in f) for f in FLIPS], dtype=np.int64), "logits": logits.astype(np.float32)}
    for k, v in stats64(logits).items():
        out["stats/" + k] = v.numpy()
    path = os.path.join(outdir, f"uncertainty_tta_{method}_t16.npz")
    np.savez_compressed(path, **out)
    print(f"uncertainty_tta_{method}_t16: oracle vs reference {dev:.3e}, entropy {out['stats/entropy']}, mutual_info {out['stats/mutual_info']}, "
          f"{os.path.getsize(path) / 1024:.1f} KiB, {time.time() - t0:.1f}s")


def main():
    outdir = os.path.join(ROOT, "tests", "golden")
    mods = import_reference()
    for n in sys.argv[1:] or list(CASES):
        run_case(mods, n, outdir)


if __name__ == "__main__":
    main()
