"""CPU test: include/bkhip.h declares the entry points of the spectral flow and the shooting functional (csrc/flow.hip,
csrc/shooting.hip) and the ctypes binding carries each with the arity of its declaration.  No compute calls."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["bk_flow_create", "bk_flow_destroy", "bk_flow_evolve", "bk_flow_jvp", "bk_flow_coefficients", "bk_flow_transform_paths",
           "bk_flow_stats", "bk_shooting_create", "bk_shooting_destroy", "bk_shooting_set_section", "bk_shooting_get_section",
           "bk_shooting_update_section", "bk_shooting_residual", "bk_shooting_jvp", "bk_shooting_op_create", "bk_shooting_op_apply",
           "bk_shooting_op_stats", "bk_shooting_transform_paths", "bk_shooting_solve", "bk_shooting_monodromy_create"]


def _declarations():
    src = open(os.path.join(ROOT, "include", "bkhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bk_(?:flow|shooting)_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_flow_and_shooting_entries():
    decl = _declarations()
    assert sorted(decl) == sorted(ENTRIES)


def test_binding_has_every_entry_with_the_arity_of_its_declaration():
    from bk_amd import _lib
    decl = _declarations()
    for name in ENTRIES:
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.I, name
        nargs = len([a for a in decl[name].split(",") if a.strip()])
        assert len(args) == nargs, (name, len(args), nargs)


def test_abi_version_is_unchanged():
    from bk_amd import _lib
    src = open(os.path.join(ROOT, "include", "bkhip.h")).read()
    assert re.search(r"#define\s+BK_ABI_VERSION\s+6\b", src) and _lib.BK_ABI_VERSION == 6


def test_shooting_module_is_exported_next_to_periodic_orbit():
    import bk_amd
    assert "shooting" in bk_amd.__all__ and "periodic_orbit" in bk_amd.__all__
