"""CPU: a static ledger of which exported kernel entry points a test calls directly.

The whole-model golden tests run every kernel, but only at a handful of shapes and within loose bf16 bounds; a kernel that is
subtly wrong can hide there.  This file parses the C ABI (include/gaviko_hip.h), maps every ops.py wrapper -- and every name of the
thin host modules below -- to the gvk_* symbols it reaches, and collects what the test files call.  The symbols no test reaches
must equal UNCOVERED exactly: a new kernel without a direct test fails here, and so does a kernel that gained one but is still listed.
A second ledger does the same for the GEMM descriptor: every ops.gemm_nt parameter the engine passes must be a keyword of a direct test.
"""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gaviko_hip.h")
PKG = os.path.join(ROOT, "gaviko_amd")
TESTS = os.path.join(ROOT, "tests")

# host modules whose names count as a direct call of the kernels they launch (each is a thin layer over ops / the library)
HOST_MODULES = ("losses", "metrics", "data", "optim", "explain")

# entry points that are neither kernels nor runtime: the error message, the device probe, queries of sizes and constants.
# (The launch-plan runtime gvk_plan_* and the fill / copy kernels behind gvk_memset_async / gvk_copy_async are NOT excluded: the ledger
# requires direct calls of them, which test_plan_runtime_gpu.py makes.)
EXCLUDED = {
    "gvk_last_error": "error message of the last failed call (read by lib.check)",
    "gvk_device_check": "device presence probe (lib.require_device)",
    "gvk_abi_version": "ABI version constant (test_abi)",
    "gvk_gemm_stat_parts": "size query",
    "gvk_attention_bwd_ws_bytes": "size query",
    "gvk_attention_bwd_status_offset": "size query",
    "gvk_param_grads_scratch": "size query",
    "gvk_gpa_gate_param_count": "size query",
    "gvk_minmax_partials": "size query",
}

# kernels that no test calls directly, each with the reason it is left out
UNCOVERED = {}


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    # function declarations only: a return type, the name, an opening parenthesis (struct typedef names never precede "(")
    return set(re.findall(r"^\s*(?:const\s+)?(?:int|int64_t|size_t|void|char)\s*\*?\s*(gvk_\w+)\s*\(", src, flags=re.M))


def _module_reach(path, ops_reach=None):
    """{top-level name: gvk_* symbols it reaches}: .gvk_* attributes in its body, ops.<wrapper> calls (when ops_reach is given) and the
    other top-level names of the same module it refers to, closed transitively."""
    tree = ast.parse(open(path).read())
    tops = {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    direct, refs = {}, {}
    for name, node in tops.items():
        syms, r = set(), set()
        for sub in ast.walk(node):
            if isinstance(sub, ast.Attribute):
                if sub.attr.startswith("gvk_"):
                    syms.add(sub.attr)
                elif ops_reach is not None and isinstance(sub.value, ast.Name) and sub.value.id == "ops":
                    syms |= ops_reach.get(sub.attr, set())
            elif isinstance(sub, ast.Name) and sub.id in tops and sub.id != name:
                r.add(sub.id)
        direct[name], refs[name] = syms, r
    reach = {}
    for name in tops:
        seen, todo, syms = {name}, [name], set()
        while todo:
            n = todo.pop()
            syms |= direct[n]
            for m in refs[n] - seen:
                seen.add(m)
                todo.append(m)
        reach[name] = syms
    return reach


def _test_references(path):
    """(module, name) pairs a test file uses: `mod.name` with mod imported from gaviko_amd, `from gaviko_amd.mod import name`,
    and ('lib', gvk_*) for direct library calls."""
    tree = ast.parse(open(path).read())
    aliases, used = {}, set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module == "gaviko_amd":
            for a in node.names:
                aliases[a.asname or a.name] = a.name
        elif isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("gaviko_amd."):
            mod = node.module.split(".", 1)[1]
            for a in node.names:
                used.add((mod, a.name))
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.startswith("gaviko_amd.") and a.asname:
                    aliases[a.asname] = a.name.split(".", 1)[1]
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            if node.attr.startswith("gvk_"):
                used.add(("lib", node.attr))
            elif isinstance(node.value, ast.Name) and node.value.id in aliases:
                used.add((aliases[node.value.id], node.attr))
    return used


def coverage():
    ops_reach = _module_reach(os.path.join(PKG, "ops.py"))
    reach = {"ops": ops_reach}
    for m in HOST_MODULES:
        reach[m] = _module_reach(os.path.join(PKG, m + ".py"), ops_reach)
    covered = set()
    for f in sorted(os.listdir(TESTS)):
        if f.startswith("test_") and f.endswith(".py"):
            for mod, name in _test_references(os.path.join(TESTS, f)):
                if mod == "lib":
                    covered.add(name)
                elif mod in reach:
                    covered |= reach[mod].get(name, set())
    return covered


def test_header_parse_is_sane():
    syms = header_symbols()
    assert len(syms) > 100
    for s in ("gvk_gemm_nt_bf16", "gvk_ssf_colgrad", "gvk_loss_fwd_bwd", "gvk_plan_replay", "gvk_attention_bwd_ws_bytes"):
        assert s in syms
    assert not any(s.endswith("_desc") or s.endswith("_job") or s.endswith("_outer") for s in syms)


def test_every_listed_symbol_exists():
    syms = header_symbols()
    assert not set(EXCLUDED) - syms, f"exclusions that are not exported: {sorted(set(EXCLUDED) - syms)}"
    assert not set(UNCOVERED) - syms, f"allow-list entries that are not exported: {sorted(set(UNCOVERED) - syms)}"
    assert not set(EXCLUDED) & set(UNCOVERED)


def test_wrappers_reach_the_library():
    ops_reach = _module_reach(os.path.join(PKG, "ops.py"))
    assert ops_reach["colsum_any"] == {"gvk_ssf_colgrad"}
    assert ops_reach["transpose_any"] == {"gvk_transpose_f32", "gvk_transpose_bf16"}
    assert ops_reach["to_operand"] >= {"gvk_cast_f32_bf16", "gvk_copy_async"}
    syms = header_symbols()
    for name, s in ops_reach.items():
        assert s <= syms, f"ops.{name} calls symbols the header does not export: {sorted(s - syms)}"


def test_uncovered_kernels_match_the_allow_list():
    kernels = header_symbols() - set(EXCLUDED)
    untested = kernels - coverage()
    new = sorted(untested - set(UNCOVERED))
    stale = sorted(set(UNCOVERED) - untested)
    assert not new, f"kernels with no direct test (add one, or list them in UNCOVERED with a reason): {new}"
    assert not stale, f"kernels listed in UNCOVERED that a test now calls (remove them from the list): {stale}"


# ---- the GEMM descriptor: every ops.gemm_nt parameter the engine passes is a keyword of some direct test --------------------------
# (the entry points gvk_gemm_nt_bf16 / gvk_gemm_nt_f32 are covered above by any one call; their features are what the engine composes)

# dict-valued names the engine splices into its GEMM calls with **: their keys come from the dict(...) literals assigned to them, and from
# the literals _panels returns (pk, top and bot carry a _panels(...) result or {})
PANEL_CARRIERS = {"pk", "top", "bot"}

# gemm_nt parameters the engine passes that no test passes directly, each with its reason
GEMM_PARAMS_UNCOVERED = {}


def _gemm_nt_parameters():
    tree = ast.parse(open(os.path.join(PKG, "ops.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "gemm_nt")
    return {a.arg for a in fn.args.args + fn.args.kwonlyargs}


def _dict_literal_keys(node):
    """keyword names of every dict(...) call inside an expression"""
    return {k.arg for sub in ast.walk(node) if isinstance(sub, ast.Call) and isinstance(sub.func, ast.Name) and sub.func.id == "dict"
            for k in sub.keywords if k.arg}


def _is_gemm_call(node, names):
    """a call of ops.gemm_nt, or of the engine's wrapper around it: self._gemm in the engine, eng._gemm in a method spec's hook"""
    if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name)):
        return False
    return (node.func.value.id, node.func.attr) in names


def engine_gemm_parameters():
    """gemm_nt parameter names the engine modules pass: keywords of self._gemm / eng._gemm / ops.gemm_nt calls, and the keys of the dict(...) literals
    behind every **name of those calls (looked up in the enclosing function; a spliced name with no literal must be a panel carrier)."""
    params = _gemm_nt_parameters()
    passed, unresolved = set(), set()
    for f in sorted(os.listdir(PKG)):
        if not (f.startswith("engine") and f.endswith(".py")):
            continue
        tree = ast.parse(open(os.path.join(PKG, f)).read())
        panel_keys = set()
        for fn in ast.walk(tree):
            if isinstance(fn, ast.FunctionDef) and fn.name == "_panels":
                for sub in ast.walk(fn):
                    if isinstance(sub, ast.Return) and sub.value is not None:
                        panel_keys |= _dict_literal_keys(sub.value)
        passed |= panel_keys
        for fn in ast.walk(tree):
            if not isinstance(fn, ast.FunctionDef) or fn.name == "_gemm":      # (the wrapper itself forwards **kw)
                continue
            assigned = {}
            for sub in ast.walk(fn):
                if isinstance(sub, ast.Assign):
                    for t in sub.targets:
                        if isinstance(t, ast.Name):
                            assigned.setdefault(t.id, set()).update(_dict_literal_keys(sub.value))
            for sub in ast.walk(fn):
                if not _is_gemm_call(sub, {("self", "_gemm"), ("eng", "_gemm"), ("ops", "gemm_nt")}):
                    continue
                for k in sub.keywords:
                    if k.arg is not None:
                        passed.add(k.arg)
                    elif isinstance(k.value, ast.Name) and (assigned.get(k.value.id) or k.value.id in PANEL_CARRIERS):
                        passed |= assigned.get(k.value.id, set())
                    else:
                        unresolved.add(f"{f}:{sub.lineno}")
    assert not unresolved, f"GEMM calls that splice something this ledger cannot read: {sorted(unresolved)}"
    return passed & params


def gemm_parameters_in_tests():
    """keywords of the ops.gemm_nt calls in the test files"""
    used = set()
    for f in sorted(os.listdir(TESTS)):
        if f.startswith("test_") and f.endswith(".py"):
            tree = ast.parse(open(os.path.join(TESTS, f)).read())
            for node in ast.walk(tree):
                if _is_gemm_call(node, {("ops", "gemm_nt")}):
                    used |= {k.arg for k in node.keywords if k.arg}
    return used


def test_engine_gemm_parameter_scan_is_sane():
    got = engine_gemm_parameters()
    assert got >= {"epilogue", "bias", "res", "aux", "ldo", "ldaux", "K", "drop_p", "aux_is_grad", "m_panels", "m_stride", "stat_part", "stat_pivot",
                   "ln_mean", "scale_cols", "rows_in"}
    assert "alg_k" not in got                                 # the engine wrapper's own argument, not a gemm_nt parameter


def test_every_gemm_parameter_the_engine_passes_has_a_direct_test():
    untested = engine_gemm_parameters() - gemm_parameters_in_tests()
    new = sorted(untested - set(GEMM_PARAMS_UNCOVERED))
    stale = sorted(set(GEMM_PARAMS_UNCOVERED) - untested)
    assert not new, f"ops.gemm_nt parameters the engine passes that no test passes (add a test, or list them in GEMM_PARAMS_UNCOVERED): {new}"
    assert not stale, f"parameters listed in GEMM_PARAMS_UNCOVERED that a test now passes, or the engine no longer does: {stale}"
