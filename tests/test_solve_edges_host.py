"""CPU test: the three solve-edge options (csrc/solver.hip, csrc/dct.hip) are documented where every context option is, in the
appendix table of DESIGN.md, with the names the sources read.  (That bk_palc_update is in both the header and the ctypes table is
tests/test_capi_symbols.py's comparison of the two.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ("gmres_check_nostore", "gmres_fuse_v0", "palc_fuse_update")


def test_options_are_in_the_design_appendix():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    appendix = txt.split("## Appendix: context options", 1)[1]
    for o in OPTIONS:
        assert re.search(r"^\| `%s` \(1\) \|" % o, appendix, flags=re.M), o


def test_options_are_read_by_the_sources_under_these_names():
    src = "".join(open(os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc", f)).read() for f in ("solver.hip", "dct.hip"))
    for o in OPTIONS:
        assert 'opt("%s", 1.0)' % o in src, o
