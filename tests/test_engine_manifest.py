"""CPU: every static fact of the engine, per method -- geometry attributes, feature flags, name queries, and the keys / nesting / shapes /
dtypes / non-zero fills of four workspaces -- equals tests/golden/engine_manifest.json, the record tools/engine_manifest.py wrote before the
per-kind ladders of Engine moved into engine_methods.py.  No kernel is launched (gaviko's training workspace asks the built library for
gvk_gpa_gate_param_count, as tests/test_abi.py loads it)."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

METHODS = ["gaviko", "linear", "fft", "bitfit", "adaptformer", "dvpt", "evp", "ssf", "melo", "deep_vpt", "shallow_vpt"]
CASES = METHODS + ["gaviko_b16", "gaviko_no_dhw", "gaviko_unfrozen", "gaviko_share2", "gaviko_fp32", "dvpt_mean", "deep_vpt_mean", "melo_layers",
                   "linear_fp32"]


def _tool():
    spec = importlib.util.spec_from_file_location("engine_manifest", os.path.join(ROOT, "tools", "engine_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def manifests():
    tool = _tool()
    with open(os.path.join(GOLDEN, "engine_manifest.json")) as f:
        want = tool.unpack(json.load(f))
    got = tool.unpack(json.loads(json.dumps(tool.pack(tool.generate()))))          # through the file form, as the committed records went
    return got, want


def _diff(a, b, path=""):
    """Paths at which two JSON values differ (dictionaries are descended into; anything else is compared whole)."""
    if isinstance(a, dict) and isinstance(b, dict):
        out = [] if list(a) == list(b) else [f"{path}: key order {list(a)} != committed {list(b)}"]
        for k in list(a) + [k for k in b if k not in a]:
            if k not in a or k not in b:
                out.append(f"{path}/{k}: " + ("gone, the committed file has it" if k not in a else "new, the committed file has none"))
            else:
                out += _diff(a[k], b[k], f"{path}/{k}")
        return out
    return [] if a == b else [f"{path}: {json.dumps(a)[:200]} != committed {json.dumps(b)[:200]}"]


def test_case_list_is_the_one_the_manifest_was_written_for(manifests):
    got, want = manifests
    assert _tool().CASE_NAMES == CASES
    assert list(got) == CASES and list(want) == CASES
    cfg = {c[0]: c for c in _tool().CASES}
    assert [cfg[m][1:] for m in METHODS] == [(m, {}, 2) for m in METHODS]           # all eleven registry methods at vit-t16, B = 2
    assert cfg["gaviko_b16"][1:] == ("gaviko", {"backbone": "vit-b16"}, 1)
    assert want["gaviko_b16"]["attrs"]["C"] == 768 and want["gaviko"]["attrs"]["C"] == 192
    assert want["gaviko_no_dhw"]["attrs"]["win"] == [21, 21, 21]
    assert want["gaviko_unfrozen"]["trainable_names"]["n"] == 442 and want["gaviko_share2"]["attrs"]["share"] == 2
    assert want["gaviko_fp32"]["attrs"]["fp32"] and want["linear_fp32"]["attrs"]["fp32"] and not want["gaviko"]["attrs"]["fp32"]
    assert want["dvpt_mean"]["pool_rows"] == [0, 51] and want["deep_vpt_mean"]["pool_rows"] == [0, want["deep_vpt_mean"]["attrs"]["Ts"][-1]]
    assert want["melo_layers"]["attrs"]["lora_layers"] == [0, 5, 11]
    assert want["deep_vpt"]["attrs"]["deep"] and not want["shallow_vpt"]["attrs"]["deep"]


def test_manifest_is_not_vacuous(manifests):
    got, _ = manifests
    fields = _tool().tensor_fields
    assert got["gaviko_b16"]["attrs"]["_fold_ln1"] is True and got["gaviko"]["attrs"]["_fold_ln1"] is False
    assert "fold_deps" in got["gaviko_b16"] and "fold_deps" not in got["gaviko"]
    for case, rec in got.items():
        w = rec["workspaces"]
        assert list(w) == ["eval", "train", "keep_attn", "feat"]
        assert len(w["train"]["slots"]) > len(w["eval"]["slots"]), case
        for tag, ws in w.items():
            assert ws["tensors"] > 0 and ws["distinct_ptrs"] == ws["tensors"], f"{case}/{tag}: two workspace slots alias"
            assert ws["keys"].split(",") == list(ws["slots"]), f"{case}/{tag}"
        seeds = [fields(w[tag]["slots"]["seed"]) for tag in ("eval", "train")]
        assert seeds[0][2] == seeds[1][2] == 1 and seeds[0][3] != seeds[1][3], case
    # the two bias columns of the K-concatenated fc2 operand: 2 ones per padded row, where the fusion is on
    _, shape, nnz, total = fields(got["gaviko"]["workspaces"]["train"]["slots"]["act"])
    assert nnz == 2 * shape[0] and total == float(nnz)
    assert fields(got["linear"]["workspaces"]["train"]["slots"]["act"])[2] == 0


@pytest.mark.parametrize("case", CASES)
def test_engine_static_facts_equal_committed_manifest(manifests, case):
    got, want = manifests
    diffs = _diff(got[case], want[case], case)
    assert not diffs, f"{len(diffs)} entries of case {case!r} differ from tests/golden/engine_manifest.json:\n" + "\n".join(diffs[:20])
