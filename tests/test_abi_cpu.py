"""The C-ABI library builds for gfx950 without a GPU, loads, and exports every symbol that
include/mssvt_hip.h declares (no compute calls here: there is no GPU in this container)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "mssvt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mssvt_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_declared_abi():
    from mssvt_amd import build
    path = build.build()
    lib = ctypes.CDLL(path)
    names = declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "libmssvt_hip.so does not export %s" % n
    lib.mssvt_hip_status_string.restype = ctypes.c_char_p
    assert lib.mssvt_hip_abi_version() >= 100
    assert lib.mssvt_hip_status_string(0) == b"ok"
    assert b"bad argument" in lib.mssvt_hip_status_string(-1)
    lib.mssvt_hash_workspace_ints.restype = ctypes.c_longlong
    assert lib.mssvt_hash_workspace_ints(1000, 2) >= 1000


def test_every_declared_entry_point_gets_its_argument_types():
    """mssvt_amd._lib declares argtypes / restype of every entry point from the header (callers then hand plain ints,
    floats and addresses to ctypes): every declared symbol must be covered, with one ctypes type per parameter and the
    return type the header states."""
    from mssvt_amd import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "mssvt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    rets = {"long long": ctypes.c_longlong, "const char *": ctypes.c_char_p}
    seen = {r: 0 for r in rets}
    for name in declared_symbols():
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        m = re.search(r"\b(int|long long|const char \*)\s*%s\s*\(([^;{]*?)\)\s*;" % name, src, flags=re.S)
        assert m is not None, name
        params = m.group(2).strip()
        want = 0 if params in ("", "void") else params.count(",") + 1
        assert len(fn.argtypes) == want, (name, len(fn.argtypes), want)
        if m.group(1) in rets:
            assert fn.restype is rets[m.group(1)], (name, fn.restype)
            seen[m.group(1)] += 1
    assert seen["long long"] >= 10 and seen["const char *"] >= 1, seen
    assert lib.mssvt_ffn_packed_bytes(128, 256) == 2 * 2 * 128 * 256 * 2  # plain ints in, long long out
    assert lib.mssvt_hip_status_string(0) == b"ok"


def test_missing_header_is_an_error_and_nothing_is_cached(monkeypatch):
    from mssvt_amd import _lib
    _lib.lib()  # the library is built
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    try:
        _lib.lib()
    except _lib.MssvtHipError as e:
        assert "no_such_header.h" in str(e)
    else:
        raise AssertionError("a missing header must raise")
    assert _lib._lib is None


def test_call_refuses_a_function_without_argument_types(monkeypatch):
    """An exported function the header does not declare has no argtypes: a plain-int address handed to it would be cut
    to 32 bits, so _lib.call refuses it before calling."""
    from mssvt_amd import _lib
    name = "mssvt_hip_abi_version"
    calls = []

    class Undeclared(object):
        argtypes = None

        def __call__(self, *args):
            calls.append(args)
            return 0

    monkeypatch.setattr(_lib.lib(), name, Undeclared())
    monkeypatch.delitem(_lib._fns, name, raising=False)
    try:
        _lib.call(name)
    except _lib.MssvtHipError as e:
        assert name in str(e)
    else:
        raise AssertionError("an undeclared function must be refused")
    assert not calls and name not in _lib._fns
    monkeypatch.undo()
    fn = getattr(_lib.lib(), name)  # the same with the real function object
    monkeypatch.setattr(fn, "argtypes", None)
    monkeypatch.delitem(_lib._fns, name, raising=False)
    try:
        _lib.call(name)
    except _lib.MssvtHipError:
        pass
    else:
        raise AssertionError("an undeclared function must be refused")
    assert name not in _lib._fns


def test_package_passes_plain_values_only():
    """One calling convention: no scalar or address of the package is wrapped in a ctypes object (host arrays and byref
    out-parameters are the only ctypes values), and the names of the second convention are gone."""
    import glob
    patterns = [r"ctypes\.c_(int|float|longlong)\(", r"c_void_p\(.*data_ptr", r"TYPED|ptr_fast|_NULL", r"^_i ="]
    for path in sorted(glob.glob(os.path.join(ROOT, "mssvt_amd", "*.py"))):
        for no, line in enumerate(open(path), 1):
            for pat in patterns:
                assert not re.search(pat, line), "%s:%d matches %s" % (os.path.basename(path), no, pat)


def header_parameter_counts():
    src = open(os.path.join(ROOT, "include", "mssvt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for name, params in re.findall(r"\b(mssvt_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_every_literal_call_site_passes_the_header_parameter_count():
    """Each `_lib.call("<name>", ...)` of the package names a declared entry point and passes as many arguments as the
    header has parameters.  Calls with a starred argument or a computed name cannot be counted here: there are 13 (11
    starred, 2 computed names), and that number only grows on purpose."""
    import ast
    import glob
    counts = header_parameter_counts()
    checked, skipped = 0, []
    for path in sorted(glob.glob(os.path.join(ROOT, "mssvt_amd", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call"
                    and isinstance(node.func.value, ast.Name) and node.func.value.id == "_lib" and node.args):
                continue
            where = "%s:%d" % (os.path.basename(path), node.lineno)
            first = node.args[0]
            if not (isinstance(first, ast.Constant) and isinstance(first.value, str)) or \
                    any(isinstance(a, ast.Starred) for a in node.args) or node.keywords:
                skipped.append(where)
                continue
            assert first.value in counts, "%s: %s is not declared in the header" % (where, first.value)
            assert len(node.args) - 1 == counts[first.value], (where, first.value, len(node.args) - 1, counts[first.value])
            checked += 1
    print("call sites: %d checked, %d skipped" % (checked, len(skipped)))
    assert checked >= 79, checked
    assert len(skipped) <= 13, skipped


def test_argument_errors_are_status_codes_not_exits():
    from mssvt_amd import build
    lib = ctypes.CDLL(build.build())
    null = ctypes.c_void_p(0)
    i = ctypes.c_int
    # null pointers / bad sizes are rejected before any HIP call
    assert lib.mssvt_build_mapping_with_hash(i(8), i(8), i(8), i(10), i(0), i(1), null, null, null, null, null) == -1
    assert lib.mssvt_group_features(i(0), i(1), i(1), i(1), null, null, null, null, null, null) == -1
    assert lib.mssvt_three_nn(i(1), i(0), i(1), null, null, null, null, null) == -1


def test_product_has_no_oracle_import_and_fails_loudly_without_library(monkeypatch):
    import mssvt_amd
    pkg = os.path.dirname(mssvt_amd.__file__)
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            txt = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in txt and "from oracle" not in txt, fn
    from mssvt_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmssvt_hip.so")
    try:
        _lib.lib()
    except _lib.MssvtHipError as e:
        assert "no CPU fallback" in str(e).replace("\n", " ") or "not built" in str(e)
    else:
        raise AssertionError("missing library must raise")


def test_pybind_stand_ins_cover_every_call_of_the_reference_python(golden_dir):
    """Every `mssvt_ops_cuda.<f>(...)` / `pointnet2.<f>(...)` call in the reference's own op files that the path uses
    must exist in the stand-in modules with the same number of positional parameters (the calls and their argument
    counts as recorded from the reference tree: tests/golden/reference_op_calls.json)."""
    import importlib
    import inspect
    import json
    with open(os.path.join(golden_dir, "reference_op_calls.json")) as f:
        calls = json.load(f)["calls"]
    modules = {"mssvt_ops_cuda": "mssvt_amd.mssvt_ops_compat", "pointnet2": "mssvt_amd.pointnet2_compat"}
    assert {c["module"] for c in calls} == set(modules)
    off_path = {"ball_query_wrapper", "three_interpolate_wrapper", "three_interpolate_grad_wrapper"}
    seen = 0
    for c in calls:
        modname, name = modules[c["module"]], c["function"]
        mod = importlib.import_module(modname)
        assert hasattr(mod, name), "%s.%s missing" % (modname, name)
        if name in off_path:
            continue
        params = inspect.signature(getattr(mod, name)).parameters
        assert len(params) == c["positional_args"], "%s: %d parameters, the reference passes %d" % (
            name, len(params), c["positional_args"])
        seen += 1
    assert seen >= 10
