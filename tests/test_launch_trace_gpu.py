"""What a step launches, per method: one eager training step and one eval forward of every case of tools/launch_trace.py issue the entry
points, on the streams, with the arguments, pointers and cross-stream edges that tests/golden/launch_trace.json records.
tests/test_engine_manifest.py pins the static facts of the engine; this pins the order and the arguments of its launches.  A failure names
the first launch that differs."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

METHODS = ["gaviko", "linear", "fft", "bitfit", "adaptformer", "dvpt", "evp", "ssf", "melo", "deep_vpt", "shallow_vpt"]
DROPOUT = ["ssf", "adaptformer", "dvpt", "gaviko"]
CASES = (METHODS + [m + "_dropout" for m in DROPOUT] + ["deep_vpt_prompt_dropout", "shallow_vpt_prompt_dropout"]
         + [m + "_unfrozen" for m in ("adaptformer", "evp", "ssf", "dvpt", "gaviko")] + [m + "_unfrozen_dropout" for m in DROPOUT]
         + ["melo_layers", "gaviko_b16"])


def _tool():
    spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def committed():
    with open(os.path.join(GOLDEN, "launch_trace.json")) as f:
        packed = json.load(f)
    assert packed["window"] == _tool().WINDOW
    return _tool().unpack(packed)


def test_case_list_is_the_one_the_trace_was_written_for(committed):
    tool = _tool()
    assert tool.CASE_NAMES == CASES and list(committed) == CASES
    cfg = {c[0]: c[1:] for c in tool.CASES}
    assert [cfg[m] for m in METHODS] == [(m, {}, 2) for m in METHODS]               # all eleven registry methods at the manifest's defaults
    for m in DROPOUT:
        assert cfg[m + "_dropout"] == (m, {"dropout": 0.2, "emb_dropout": 0.1}, 2)
        assert cfg[m + "_unfrozen_dropout"] == (m, {"freeze_vit": False, "dropout": 0.2, "emb_dropout": 0.1}, 2)
    for m in ("deep_vpt", "shallow_vpt"):
        assert cfg[m + "_prompt_dropout"] == (m, {"prompt_dropout": 0.1}, 2)
    for m in ("adaptformer", "evp", "ssf", "dvpt", "gaviko"):
        assert cfg[m + "_unfrozen"] == (m, {"freeze_vit": False}, 2)
    assert cfg["melo_layers"] == ("melo", {"alpha": 8, "lora_layer": [0, 5, 11]}, 2)
    assert cfg["gaviko_b16"] == ("gaviko", {"backbone": "vit-b16"}, 1)


def test_committed_trace_is_not_vacuous(committed):
    for case, c in committed.items():
        assert c["n"] == len(c["order"]) > 200 and len(c["sha256"]) == 64, case
        assert len(c["digests"]) == 4 * -(-c["n"] // _tool().WINDOW), case
        fns = [s.split("@")[0] for s in c["order"]]
        assert fns[0] == "phase:train" and fns.count("phase:eval") == 1 and "gvk_head_bwd" in fns, case
        streams = {s.split("@")[1] for s in c["order"]}
        assert streams == ({"0", "1", "2"} if case.startswith("gaviko") else {"0"}), case      # GAViKO alone forks: the MWSA and GPA streams
        assert ("ev_wait" in fns) == case.startswith("gaviko"), case
    fns = lambda case: {s.split("@")[0] for s in committed[case]["order"]}
    assert "gvk_ssf_colgrad" in fns("ssf") and "gvk_dvpt_bwd" in fns("dvpt") and "gvk_evp_highpass" in fns("evp")
    assert "gvk_lora_merge_f32" in fns("melo") and "gvk_vpt_repack_bwd" in fns("deep_vpt") and "gvk_vpt_repack_bwd" not in fns("shallow_vpt")
    assert "gvk_prompt_up_fix_stats" in fns("gaviko_b16") and "gvk_prompt_up_fix_stats" not in fns("gaviko")
    assert committed["melo_layers"]["n"] < committed["melo"]["n"] and committed["ssf_unfrozen"]["n"] > committed["ssf"]["n"]
    count = lambda case, fn: [s.split("@")[0] for s in committed[case]["order"]].count(fn)
    for m in ("deep_vpt", "shallow_vpt"):
        assert count(m + "_prompt_dropout", "gvk_dropout_rows") > 0 and count(m, "gvk_dropout_rows") == 0, m
    for m in DROPOUT:
        # a frozen backbone keeps its nn.Dropout modules in eval (the classes' train() overrides): the rates reach no launch ...
        assert count(m + "_dropout", "gvk_dropout_rows") == 0 and committed[m + "_dropout"]["sha256"] == committed[m]["sha256"], m
        # ... an unfrozen one runs them: embedding dropout forward and backward, and a masked gradient per block of every layer
        live, base = m + "_unfrozen_dropout", m + "_unfrozen"
        assert count(base, "gvk_dropout_rows") == 0 and count(live, "gvk_dropout_rows") >= 2 + 2 * 12, m
        assert committed[live]["sha256"] != committed[base]["sha256"] and committed[live]["digests"] != committed[base]["digests"], m


def test_repeat_folding_round_trips():
    tool = _tool()
    seq = [0, 1, 2] + [3, 4, 5, 5, 5, 5, 6] * 12 + [7] + [3, 4, 5, 5, 5, 5, 6] * 3 + [8, 8]
    assert tool.unfold_repeats(tool.fold_repeats(seq)) == seq and len(json.dumps(tool.fold_repeats(seq))) < len(json.dumps(seq)) // 4
    s = {"a": {"n": len(seq), "order": [f"k{x}@0" for x in seq], "sha256": "x", "digests": ""},
         "b": {"n": len(seq), "order": [f"k{x}@1" for x in reversed(seq)], "sha256": "y", "digests": ""}}
    assert tool.unpack(json.loads(json.dumps(tool.pack(s)))) == s


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_step_launches_equal_committed_trace(dev, committed, case):
    tool = _tool()
    got = tool.summary(tool.generate({case})[case])
    diff = tool.first_difference(got, committed[case])
    assert diff is None, f"case {case!r} departs from tests/golden/launch_trace.json: {diff}"
