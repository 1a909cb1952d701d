"""CPU tests of the Krylov kernel tests' own bookkeeping (no GPU):
* every mangled launcher name in tests/vecops_abi.py resolves in the built library (a changed signature fails here first);
* the coverage table of test_gpu_vecops_exact.py names exactly the kernel launch expressions of csrc/vecops.hip, and only
  tests that exist -- a new kernel variant cannot land without a test that reaches it.
"""
import ctypes
import os
import re

import pytest

import test_gpu_vecops_exact as gv
import vecops_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECOPS = os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc", "vecops.hip")


def launch_expressions(src):
    """The kernel expression of every hipLaunchKernelGGL(...) as written: `(name<args>)` with its parentheses stripped, or a bare
    name up to the first comma.  Template arguments are kept verbatim, including macro parameters (KB, UU, NR5)."""
    src = re.sub(r"//[^\n]*", "", src)
    out = []
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*", src):
        i = m.end()
        if src[i] == "(":
            depth, j = 0, i
            while True:
                depth += {"(": 1, ")": -1}.get(src[j], 0)
                if depth == 0:
                    break
                j += 1
            expr = src[i + 1:j]
        else:
            expr = re.match(r"[^,]+", src[i:]).group(0)
        out.append(" ".join(expr.split()))
    return out


def test_every_launcher_symbol_resolves():
    from bk_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [m for m in vecops_abi.LAUNCHERS if not hasattr(lib, m)]
    assert not missing, f"launchers whose mangled name (signature) changed: {missing}"
    vecops_abi.Launchers(lib)                    # binds every one


def test_launcher_table_covers_every_launcher():
    """Every bk::v_* launcher vecops.hip defines is in the table (by its unmangled name)."""
    src = open(VECOPS).read()
    defined = set(re.findall(r"^(?:int|bool) (v_[a-z0-9_]+)\(", src, flags=re.M))
    bound = {name for name, _, _ in vecops_abi.LAUNCHERS.values()}
    assert defined == bound, (sorted(defined - bound), sorted(bound - defined))


def test_extractor_sees_macro_forms():
    exprs = set(launch_expressions(open(VECOPS).read()))
    for must in ["block_dots_kernel<8, true, 2, true, NR5>", "multidot_c_kernel<KB, 8, true>", "absmax_kernel",
                 "multiaxpy_kernel<KB, 2, true, true, 2, true>", "reduce_stage2_dev"]:
        assert must in exprs, must


def test_coverage_table_matches_vecops():
    exprs = set(launch_expressions(open(VECOPS).read()))
    table = set(gv.COVERAGE)
    assert exprs == table, dict(untested=sorted(exprs - table), stale=sorted(table - exprs))
    tests = {name for name in dir(gv) if name.startswith("test_")}
    for expr, ids in gv.COVERAGE.items():
        assert ids, expr
        unknown = [t for t in ids if t not in tests]
        assert not unknown, (expr, unknown)


def template_defaults(src):
    """kernel name -> its template parameters as (name, default or None), from the `template <...> __global__ void name(` heads."""
    out = {}
    src = re.sub(r"//[^\n]*", "", src)
    for m in re.finditer(r"template <([^>]*)>\s*__global__ void(?: __launch_bounds__\([^)]*\))? (\w+)\(", src):
        params = []
        for p in m.group(1).split(","):
            name, _, dflt = p.partition("=")
            params.append((name.split()[-1], dflt.strip().replace("sstep::kR", str(vecops_abi.SSTEP_KR)) or None))
        out[m.group(2)] = params
    return out


def expression_matches(expr, inst, defaults):
    """Does the launch expression `expr` as written (macro parameters KB / UU stand for any bucket, NR5 = 5; omitted arguments take
    the template's defaults) denote the traced instantiation `inst`?"""
    name_e, _, args_e = expr.partition("<")
    name_i, _, args_i = inst.partition("<")
    if name_e != name_i:
        return False
    ae = [a.strip() for a in args_e.rstrip(">").split(",")] if args_e else []
    ai = [a.strip() for a in args_i.rstrip(">").split(",")] if args_i else []
    params = defaults.get(name_e, [])
    for j, got in enumerate(ai):
        want = ae[j] if j < len(ae) else params[j][1]
        if want in ("KB", "UU"):
            continue
        if (want == "NR5" and got != "5") or (want != "NR5" and want != got):
            return False
    return True


def test_every_covered_expression_was_launched_on_the_gpu():
    """profiles/vecops_kernels_traced.txt: the instantiations the kernel tracer recorded while the GPU module ran."""
    src = open(VECOPS).read()
    defaults = template_defaults(src)
    traced = [line.split("\t")[0] for line in open(os.path.join(ROOT, "profiles", "vecops_kernels_traced.txt"))
              if line.strip() and not line.startswith("#")]
    missing = [e for e in gv.COVERAGE if not any(expression_matches(e, t, defaults) for t in traced)]
    assert not missing, f"in the coverage table but never launched: {missing}"
    unexplained = [t for t in traced if not any(expression_matches(e, t, defaults) for e in gv.COVERAGE)]
    assert not unexplained, unexplained
