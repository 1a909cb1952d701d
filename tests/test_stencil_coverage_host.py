"""CPU tests of the stencil kernel tests' own bookkeeping (no GPU):
* the ctypes mirrors of ShArgs, CglArgs and Sh1dArgs in tests/stencil_abi.py equal the struct bodies of csrc/ops.h field by field --
  names, order, C types, default member values (a mangled launcher name encodes the struct's name, not its layout);
* every mangled launcher name resolves in the built library (a changed signature fails here first);
* the coverage table of test_gpu_stencil_exact.py names exactly the kernel launch expressions of csrc/stencil.hip, and only tests
  that exist -- a new kernel variant cannot land without a test that reaches it.
"""
import ctypes
import os
import re

import pytest

import stencil_abi
import test_gpu_stencil_exact as gs
from test_vecops_coverage_host import launch_expressions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc")
STENCIL = os.path.join(CSRC, "stencil.hip")

C_DEFAULTS = {"0.0": 0.0, "0": 0, "false": False, "nullptr": "nullptr"}


def parse_struct(src, name):
    """[(field, C type, default or None)] of `struct name { ... };` as declared: comments stripped, `int nx, ny;` split up."""
    body = re.search(r"struct %s \{(.*?)\n\};" % name, src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"((?:const )?(?:int|double|bool)\*?) (.+)", decl)
        assert m, f"{name}: a declaration this parser does not know: {decl!r}"
        for item in m.group(2).split(","):
            field, _, dflt = item.partition("=")
            out.append((field.strip(), m.group(1), C_DEFAULTS[dflt.strip()] if dflt.strip() else None))
    return out


def test_parser_reads_the_declaration_forms_of_ops_h():
    src = "struct T {   // c; omment\n    int a, b;   // x\n    double c = 0.0;\n    const double* p = nullptr;\n    bool q = false;\n};\n"
    assert parse_struct(src, "T") == [("a", "int", None), ("b", "int", None), ("c", "double", 0.0),
                                      ("p", "const double*", "nullptr"), ("q", "bool", False)]


@pytest.mark.parametrize("name", sorted(stencil_abi.STRUCTS))
def test_ctypes_mirror_equals_the_struct_of_ops_h(name):
    declared = parse_struct(open(os.path.join(CSRC, "ops.h")).read(), name)
    table = stencil_abi.STRUCTS[name]
    nulls = stencil_abi.NULL_DEFAULTS.get(name, ())
    mirror = [(f, t, "nullptr" if f in nulls else d) for f, t, d in table]
    assert [(f, t) for f, t, _ in declared] == [(f, t) for f, t, _ in mirror]
    for (f, _, want), (_, _, got) in zip(declared, mirror):      # 0 == 0.0 == False in Python: compare the types too
        assert want == got and type(want) is type(got), (f, want, got)
    cls = getattr(stencil_abi, name)
    assert [(f, c) for f, c in cls._fields_] == [(f, stencil_abi.CTYPES[t]) for f, t, _ in declared]
    # the constructor sets the default member values
    obj = cls()
    for f, _, d in declared:
        if d == "nullptr":
            assert not getattr(obj, f)
        elif d is not None:
            assert getattr(obj, f) == d and type(getattr(obj, f)) is type(d)
    with pytest.raises(TypeError):
        cls(no_such_field=1)


def test_every_launcher_symbol_resolves():
    from bk_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [m for m in stencil_abi.LAUNCHERS if not hasattr(lib, m)]
    assert not missing, f"launchers whose mangled name (signature) changed: {missing}"
    stencil_abi.Launchers(lib)                   # binds every one


def test_launcher_table_covers_every_launcher_of_stencil_hip():
    src = open(STENCIL).read()
    defined = set(re.findall(r"^(?:int|bool) (\w+)\(bk_ctx\* ctx", src, flags=re.M))
    bound = {name for name, _, _ in stencil_abi.LAUNCHERS.values()} - {"jvp_axpy_dot"}
    assert defined == bound, (sorted(defined - bound), sorted(bound - defined))


def test_constants_match_the_sources():
    src = open(STENCIL).read()
    assert re.search(r"constexpr int TX = (\d+), TY = (\d+);", src).groups() == (str(stencil_abi.TX), str(stencil_abi.TY))
    assert f"n >= ((size_t)1 << {stencil_abi.NT_POINTS.bit_length() - 1})" in src
    assert f"if (grid > {stencil_abi.DPARAM_GRID_CAP}) grid = {stencil_abi.DPARAM_GRID_CAP};" in src
    common = open(os.path.join(CSRC, "common.h")).read()
    blocks = int(re.search(r"constexpr int kRedBlocks = (\d+);", common).group(1))
    vals = int(re.search(r"constexpr int kPartialVals = (\d+);", common).group(1))
    assert blocks * vals == stencil_abi.K_PARTIAL_DOUBLES


def test_coverage_table_matches_stencil_hip():
    exprs = launch_expressions(open(STENCIL).read())
    assert len(exprs) == len(set(exprs)) == 12, exprs
    table = set(gs.COVERAGE)
    assert set(exprs) == table, dict(untested=sorted(set(exprs) - table), stale=sorted(table - set(exprs)))
    tests = {name for name in dir(gs) if name.startswith("test_")}
    for expr, ids in gs.COVERAGE.items():
        assert ids, expr
        unknown = [t for t in ids if t not in tests]
        assert not unknown, (expr, unknown)
    # the two-waves-per-SIMD fused instantiations are reached by tests that set jvp_fd_waves = 2
    for expr in ("sh_stream_kernel<true, true, true, 2>", "sh_stream_kernel<true, false, true, 2>"):
        assert "test_fused_lanczos_step_exact" in gs.COVERAGE[expr]
