"""CPU tests of the bookkeeping around csrc/block_dots_wide.hip (no GPU): the coverage table of test_gpu_block_dots_wide.py names
exactly the kernel launch expressions of that file, and only tests that exist; the two context options of the change are in the
appendix table of DESIGN.md under the names the sources read; the new C entry is where the corrector's callers look for it."""
import os
import re

import test_gpu_block_dots_wide as gw
from test_vecops_coverage_host import launch_expressions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc")


def test_coverage_table_matches_block_dots_wide():
    exprs = set(launch_expressions(open(os.path.join(CSRC, "block_dots_wide.hip")).read()))
    table = set(gw.COVERAGE)
    assert exprs and exprs == table, dict(untested=sorted(exprs - table), stale=sorted(table - exprs))
    tests = {name for name in dir(gw) if name.startswith("test_")}
    for expr, ids in gw.COVERAGE.items():
        assert ids, expr
        unknown = [t for t in ids if t not in tests]
        assert not unknown, (expr, unknown)


def test_wide_slot_count_and_record():
    """NRW of the launch expressions is kBlockDotsWideNr = 6, and 8 x 6 + 21 values per workgroup fit the partial-sum record."""
    common = open(os.path.join(CSRC, "common.h")).read()
    nrw = int(re.search(r"constexpr int kBlockDotsWideNr = (\d+);", common).group(1))
    vals = int(re.search(r"constexpr int kPartialVals = (\d+);", common).group(1))
    assert nrw == 6 and 8 * nrw + nrw * (nrw + 1) // 2 <= vals
    src = open(os.path.join(CSRC, "block_dots_wide.hip")).read()
    assert "constexpr int NRW = kBlockDotsWideNr" in src
    assert "block_dots_wide.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_routing_keeps_the_five_slot_guard():
    src = open(os.path.join(CSRC, "vecops.hip")).read()
    assert 'nr > NR5 && nr <= kBlockDotsWideNr && kold > 4 && ctx->opt("block_dots_wide", 1.0) != 0.0' in src
    assert 'nr <= NR5 && kold > 4 && ctx->opt("block_dots_nr5", 1.0) != 0.0' in src


def test_options_are_in_the_design_appendix():
    appendix = open(os.path.join(ROOT, "DESIGN.md")).read().split("## Appendix: context options", 1)[1]
    assert re.search(r"^\| `block_dots_wide` \(1\) \|", appendix, flags=re.M)
    assert re.search(r"^\| `palc_entry_copy` \(0\) \|", appendix, flags=re.M)
    assert 'opt("palc_entry_copy", 0.0)' in open(os.path.join(CSRC, "solver.hip")).read()
