"""CPU: the C-ABI library loads and exports every symbol include/gaviko_hip.h declares; every struct of the header has a ctypes class in
gaviko_amd/lib.py with exactly its field order; every prototype has the argtypes (and return type) lib.py binds; lib.launch turns a call
into the library's calling convention (no compute calls -- no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "gaviko_hip.h")


def _header():
    return open(HEADER).read()


def _strip_comments(s):
    return re.sub(r"/\*.*?\*/", "", s, flags=re.S)


def test_library_exports_every_declared_symbol():
    from gaviko_amd import lib
    l = lib.load()
    src = _strip_comments(_header())
    decls = re.findall(r"\b(gvk_[a-z0-9_]+)\s*\(", src)
    assert len(decls) >= 20
    bound = set(lib.SIGNATURES) | set(lib.NO_STREAM)
    for name in sorted(set(decls)):
        assert hasattr(l, name), f"{name} declared in gaviko_hip.h but not exported by libgaviko_hip.so"
        assert name in bound, f"{name} has no ctypes signature in gaviko_amd/lib.py"
    assert l.gvk_abi_version() == lib.ABI_VERSION == 14


def test_ctypes_structs_match_header_field_order():
    from gaviko_amd import lib
    src = _strip_comments(_header())
    for cname, cls in lib.STRUCTS.items():
        m = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", src, flags=re.S)
        assert m, cname
        fields = []
        for stmt in m.group(1).split(";"):
            stmt = stmt.strip()
            if not stmt:
                continue
            typ = re.match(r"(const\s+)?(void|float|int32_t|uint64_t|int64_t|gvk_\w+)\s*(\*?)", stmt)      # (a gvk_* struct only behind a pointer)
            names = re.sub(r"^(const\s+)?(void|float|int32_t|uint64_t|int64_t|gvk_\w+)", "", stmt)
            for nm in names.split(","):
                nm = nm.strip()
                is_ptr = nm.startswith("*") or typ.group(3) == "*" and nm == names.split(",")[0].strip()
                fields.append((nm.lstrip("* ").strip(), "ptr" if "*" in nm or (typ.group(3) == "*" and nm == names.split(",")[0].strip()) else typ.group(2)))
        want = []
        for name, ct in cls._fields_:
            kind = {ctypes.c_void_p: "ptr", ctypes.c_int32: "int32_t", ctypes.c_float: "float", ctypes.c_uint64: "uint64_t", ctypes.c_int64: "int64_t"}[ct]
            want.append((name, kind))
        assert fields == want, f"{cname}: header {fields} != ctypes {want}"


def test_every_header_struct_is_registered():
    from gaviko_amd import lib
    declared = set(re.findall(r"typedef struct (gvk_\w+)", _strip_comments(_header())))
    assert len(declared) >= 21
    assert declared == set(lib.STRUCTS), f"header structs without a ctypes class: {sorted(declared - set(lib.STRUCTS))}; " \
                                         f"ctypes classes without a header struct: {sorted(set(lib.STRUCTS) - declared)}"


# scalar C types of the header -> (i signed / u unsigned / f floating, bytes)
SCALARS = {"int": ("i", 4), "int32_t": ("i", 4), "int64_t": ("i", 8), "long": ("i", ctypes.sizeof(ctypes.c_long)), "uint64_t": ("u", 8),
           "size_t": ("u", ctypes.sizeof(ctypes.c_size_t)), "float": ("f", 4), "double": ("f", 8)}


def _prototypes():
    """{function: (return type, [argument types])} of the header, a type being (base, is_pointer) with const and the argument name dropped."""
    src = re.sub(r"typedef struct \w+\s*\{.*?\}\s*\w+\s*;", " ", _strip_comments(_header()), flags=re.S)

    def typ(decl, named):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*" + (r"\w+" if named else ""), decl.strip())
        assert m, decl
        return m.group(1), m.group(2) == "*"

    protos = {}
    for ret, name, args in re.findall(r"([\w \t\*]+?)\b(gvk_\w+)\s*\(([^)]*)\)\s*;", src):
        args = [] if args.strip() in ("", "void") else args.split(",")
        assert name not in protos, name
        protos[name] = (typ(ret, False), [typ(a, True) for a in args])
    return protos


def _same_type(header, ct, structs):
    """Does the ctypes type `ct` describe the header type (base, is_pointer)?"""
    base, is_ptr = header
    code = getattr(ct, "_type_", None)
    if not is_ptr:                                # same class of number, same width
        kind = "i" if code in tuple("bhilq") else "u" if code in tuple("BHILQ") else "f" if code in ("f", "d") else None
        return (kind, ctypes.sizeof(ct)) == SCALARS[base]
    if base.startswith("gvk_"):                   # a descriptor: the registered class of exactly that struct
        return base in structs and ct is ctypes.POINTER(structs[base])
    if ct is ctypes.c_void_p or (ct is ctypes.c_char_p and base == "char"):
        return True
    return isinstance(code, type) and base in SCALARS and _same_type((base, False), code, structs)      # POINTER(scalar): an out-parameter


def test_prototype_parse_is_sane():
    from gaviko_amd import lib
    protos = _prototypes()
    assert len(protos) > 120
    assert not set(protos) & set(lib.STRUCTS) and not any(n.endswith(("_desc", "_job", "_outer")) for n in protos)
    assert protos["gvk_last_error"] == (("char", True), [])
    assert protos["gvk_scale_dev"] == (("int", False), [("float", True), ("float", True), ("int64_t", False), ("void", True)])
    assert protos["gvk_layernorm_bwd"][1] == [("gvk_ln_bwd_desc", True), ("void", True)]


def test_every_prototype_matches_its_argtypes():
    from gaviko_amd import lib
    bound = {**lib.NO_STREAM, **{name: (ctypes.c_int, args) for name, args in lib.SIGNATURES.items()}}
    protos = _prototypes()
    assert set(protos) == set(bound)
    for name, (ret, args) in sorted(protos.items()):
        res, argtypes = bound[name]
        assert _same_type(ret, res, lib.STRUCTS), f"{name}: returns {ret} in the header, {res} in lib.py"
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments in the header, {len(argtypes)} in lib.py"
        for k, (h, ct) in enumerate(zip(args, argtypes)):
            assert _same_type(h, ct, lib.STRUCTS), f"{name}: argument {k} is {h} in the header, {ct} in lib.py"
        if name in lib.SIGNATURES:
            assert args[-1] == ("void", True), f"{name}: SIGNATURES is for the entry points that take the stream last"


def test_same_type_tells_types_apart():
    """The comparison itself: width, signedness, pointer-ness and the struct behind a pointer each make a difference."""
    from gaviko_amd import lib
    S = lib.STRUCTS
    assert _same_type(("int", False), ctypes.c_int32, S) and not _same_type(("int", False), ctypes.c_int64, S)
    assert _same_type(("int64_t", False), ctypes.c_int64, S) and not _same_type(("int64_t", False), ctypes.c_uint64, S)
    assert _same_type(("uint64_t", False), ctypes.c_uint64, S) and not _same_type(("uint64_t", False), ctypes.c_int, S)
    assert _same_type(("float", False), ctypes.c_float, S) and not _same_type(("float", False), ctypes.c_double, S)
    assert not _same_type(("int", False), ctypes.c_void_p, S) and not _same_type(("float", True), ctypes.c_float, S)
    assert _same_type(("float", True), ctypes.c_void_p, S) and _same_type(("float", True), ctypes.POINTER(ctypes.c_float), S)
    assert not _same_type(("float", True), ctypes.POINTER(ctypes.c_double), S) and not _same_type(("float", True), ctypes.c_char_p, S)
    assert _same_type(("gvk_head_desc", True), ctypes.POINTER(lib.HeadDesc), S)
    assert not _same_type(("gvk_head_desc", True), ctypes.POINTER(lib.LossDesc), S) and not _same_type(("gvk_head_desc", True), ctypes.c_void_p, S)


def test_launch_converts_arguments_and_checks_the_return_code(monkeypatch):
    import torch
    from gaviko_amd import lib
    calls = []

    class Stub:
        def gvk_colsum(self, *args):
            calls.append(args)
            return 0

        def gvk_scale_f32(self, *args):
            return 7

        def gvk_last_error(self):
            return b"stub says no"

    monkeypatch.setattr(lib, "_lib", Stub())
    monkeypatch.setattr(lib, "stream_ptr", lambda: 0x5eed)
    t = torch.zeros(4)
    ref = ctypes.byref(ctypes.c_int(3))
    assert lib.launch.gvk_colsum(t, None, ref, 5, 2.5) is None
    assert calls == [(t.data_ptr(), None, ref, 5, 2.5, 0x5eed)]                    # tensor -> pointer, the rest as given, the stream last
    assert type(calls[0][3]) is int and type(calls[0][4]) is float
    with pytest.raises(lib.GavikoHipError, match=r"gvk_scale_f32 failed \(rc=7\): stub says no"):
        lib.launch.gvk_scale_f32(t, 1.0, 4)
    with pytest.raises(AttributeError):
        lib.launch.gvk_no_such_symbol(t)
    with pytest.raises(AttributeError):                                           # size queries and the plan runtime take no stream
        lib.launch.gvk_plan_size(0)
    with pytest.raises(AttributeError):                                           # declared, but looked up on the library at call time
        lib.launch.gvk_copy_async(t, t, 16)
    monkeypatch.setattr(Stub, "gvk_copy_async", lambda self, *args: calls.append(args) or 0, raising=False)
    lib.launch.gvk_copy_async(t, t, 16)
    assert calls[-1] == (t.data_ptr(), t.data_ptr(), 16, 0x5eed)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from gaviko_amd import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(lib.GavikoHipError):
        lib.load()


def test_no_device_fails_loudly():
    import torch
    from gaviko_amd import lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(lib.GavikoHipError):
        lib.require_device()
