"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step returned (logits, loss, every trainable gradient), and two runs with
the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def run_bench(cwd, out):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backbone", "vit-t16", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                        "--no-roofline", "--dump-outputs", str(out)], env=env, cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_dump_outputs_are_the_last_timed_step(dev, tmp_path):
    from gaviko_amd.utils import synth
    a, b = tmp_path / "a", tmp_path / "b"
    line = run_bench(tmp_path, a)
    run_bench(tmp_path, b)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"logits.npy", "loss.npy", "grad.prompt_embeddings.npy", "grad.mlp_head.head.weight.npy"} <= set(names)
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    logits, loss = np.load(a / "logits.npy"), np.load(a / "loss.npy")
    assert logits.shape == (4, 5) and logits.dtype == np.float32 and np.isfinite(logits).all()
    # loss and logits come from the same step: the loss is the cross entropy of the dumped logits on the benchmark's labels
    want = torch.nn.functional.cross_entropy(torch.from_numpy(logits), torch.from_numpy(synth.labels(0, 4))).item()
    assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want))
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
