"""CPU tests of the DCT route tests' own bookkeeping (no GPU):
* every dct_* option the dispatch reads through ctx->opt("...") in csrc/dct.hip and csrc/dct_fast.hip is set by a case of
  tests/test_gpu_dct_routes.py or is excluded here with a reason -- a new option cannot land without a test or a stated reason;
* every shape of the route table is a shape on which tests/test_dct_reference.py pins the oracle (the one large shape is exempt);
* the table is well formed: every pass has a kernel, and the family lists name cases that exist.
"""
import os
import re

import test_dct_reference as ref
import test_gpu_dct_routes as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc")

# option (or prefix, ending in *) -> why the route table does not set it
EXCLUDED = {
    "dct_trace": "the diagnostic the route assertions read; every case sets it",
    "dct_lt": "experiment knob (lines per tile); the default 0 is the tested behaviour",
    "dct_stagger*": "experiment knobs (start offsets per pass); the defaults 0 are the tested behaviour",
    "dct_const_len": "tests/test_gpu_dct_const_len.py: bitwise A/B and kernel choice",
    "dct_x_turnaround": "tests/test_gpu_x_turnaround.py: bitwise A/B of the operator chain",
    "dct_gemm": "tests/test_gpu_parity.py and tests/test_gpu_dst_transforms.py: the three dense products against each other",
    "dct_fused_dot": "tests/test_gpu_eigensolve_at_size.py: MINRES through the spectral dot of the round trip",
    "dct_slab_emulate": "tests/test_distributed.py (tests/dist_worker.py): the slab cost model",
    "dct_slab_split": "tests/test_distributed.py (tests/dist_worker.py) and tests/test_gpu_slab_zsolve.py (one process plays every "
                      "rank): the slab z-solve's half passes",
    "dct_dist_*": "tests/test_distributed.py (tests/dist_worker.py): the distributed plan",
}


def option_keys():
    keys = set()
    for f in ("dct.hip", "dct_fast.hip"):
        keys |= set(re.findall(r'ctx->opt\("(dct_\w+)"', open(os.path.join(CSRC, f)).read()))
    return keys


def _excluded(key):
    return any(key == e or (e.endswith("*") and key.startswith(e[:-1])) for e in EXCLUDED)


def test_every_dct_option_is_in_the_matrix_or_excluded_with_a_reason():
    keys = option_keys()
    assert len(keys) >= 20, sorted(keys)                    # (the pattern still finds the reads)
    matrix = gr.option_matrix()
    missing = sorted(k for k in keys if k not in matrix and not _excluded(k))
    assert not missing, f"dct options without a route case or a stated exclusion: {missing}"
    both = sorted(k for k in matrix if _excluded(k))
    assert not both, f"options both tested and excluded: {both}"
    stale = sorted(k for k in matrix if k not in keys)
    assert not stale, f"options the route table sets but the sources no longer read: {stale}"
    assert all(EXCLUDED.values())


def test_every_option_of_the_matrix_can_be_restored():
    """Each option a case sets on the session's context has its default in DEFAULTS; the others run on a context of their own."""
    for k in gr.option_matrix():
        assert (k in gr.DEFAULTS) != (k in gr.OWN_CONTEXT), k


def test_every_shape_of_the_route_table_is_pinned_by_the_reference_test():
    """(64, 256, 256) is exempt: 4 M points, whose long-double dense products would take minutes; its oracle is the same scipy
    transform the reference test pins at N = 64 and N = 256 on the smaller shapes."""
    shapes = {c["dims"] for c in gr.CASES.values()} - {gr.BIG}
    assert shapes <= set(ref.DIMS), sorted(shapes - set(ref.DIMS))
    assert {gr.CASES[n]["dims"] for n in gr.FAMILIES} == set(ref.MODE_DIMS)


def test_the_route_table_is_well_formed():
    for name, c in gr.CASES.items():
        nd = len(c["dims"])
        assert len(c["routes"]) in (2 * nd - 1, 2 * nd) and set(c["routes"]) <= set("FGD"), name
        assert c["layout"] in ("al", "v", "o", "vo"), name
        seq = gr.pass_sequence(nd, len(c["routes"]))
        fused_axes = {a for (a, _), r in zip(seq, c["routes"]) if r == "F"}
        assert set(c["lt"]) <= fused_axes - {0} and set(c["lt"].values()) <= {32, 64, 128}, name
    assert set(gr.FAMILIES) <= set(gr.CASES)
    assert {"F", "G", "D"} == {r for n in gr.FAMILIES for r in gr.CASES[n]["routes"]}
