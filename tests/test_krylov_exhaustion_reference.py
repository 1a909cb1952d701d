"""The cases of tests/test_gpu_krylov_exhaustion.py are exhaustion cases: established on the reference alone (no GPU, writes nothing).

A solve "runs out of Krylov space" when its residual cannot meet the tolerance before step n and is at rounding level at step n.  For every
case the GPU test runs, the extended-precision Arnoldi process of tests/krylov_dense_ref.py must show

  * residual at step n - 1  >=  1e3 * tol,
  * residual at step n      <=  1e-3 * tol,

so that the tolerance sits three orders away from both neighbouring residuals and every count below is exact, not "+-1"; and the
step-by-step restatement and the block restatement of the oracle must report the same count wherever the library's block Arnoldi serves the
case.  A case that misses a condition is replaced in krylov_dense_ref (another draw or size), never skipped here.  The numbers the GPU test
takes from the oracle are committed as tests/golden/krylov_exhaustion.json (python tests/krylov_dense_ref.py --record); this test holds the
file against a fresh evaluation.
"""
import numpy as np
import pytest

import krylov_dense_ref as R

GMRES_CASES = R.all_gmres_cases()
_ID = lambda c: c.cid      # noqa: E731


@pytest.fixture(scope="module")
def golden():
    return R.golden()


def test_case_lists_cover_what_the_issue_names():
    assert len(R.A_SIDS) == 17 and len(R.A_CASES) == 34
    assert sorted(R.SYSTEMS[s].n for s in R.A_SIDS if s.startswith("sh1d")) == [2, 3, 5, 9, 17, 32, 33, 36, 40, 62, 63]
    assert sorted(R.SYSTEMS[s].n for s in R.B_SIDS) == [5, 33, 40, 63] and len(R.B_CASES) == 8
    assert R.F_CASE in R.A_CASES and R.F_CASE.n == 40
    assert all(R.Case(s) in R.A_CASES for s in R.G_FOLD_SIDS + R.G_CHUNK_SIDS)
    assert all(33 <= R.SYSTEMS[s].n <= 62 for s in R.G_CHUNK_SIDS)
    assert max(c.n for c in GMRES_CASES) <= 64
    assert len({c.cid for c in GMRES_CASES}) == len(GMRES_CASES)


def test_every_gpu_case_has_its_numbers_in_the_golden_file(golden):
    want = {c.cid for c in GMRES_CASES} | {label for label, _, _ in R.e_cases()} | {R.b_label(c) for c in R.B_CASES}
    assert set(golden) == want, (sorted(want - set(golden)), sorted(set(golden) - want))


@pytest.mark.parametrize("case", [c for c in GMRES_CASES if c not in (R.C_TIGHT_CASE, R.G_INSIDE_CASE)], ids=_ID)
def test_gmres_case_is_an_exhaustion_case(case, golden):
    n = case.n
    before, at = R.certify(case)
    assert before >= 1e3, (case.cid, before)
    assert at <= 1e-3, (case.cid, at)
    o = R.oracle_gmres(case)
    assert all(o["converged"].values()), o
    c = o["counts"]
    if "krylovkit" in c:
        assert c["krylovkit"] == n + 2          # one application for the initial residual, n Arnoldi steps, one explicit check
        if case.blocks:
            assert c["block"] == c["krylovkit"], c
    for name in ("iterativesolvers", "krylovjl"):
        if name in c:
            assert c[name] == n, c
    g = golden[case.cid]
    assert g["n"] == n and g["counts"] == c, (g, c)
    # the recorded true residuals are the oracle's: a float64 computation, equal up to the BLAS at hand -- within a factor 2
    ref = R.reference(case)
    for name, v in o["true_residual"].items():
        assert v <= 1.5 * ref.tol, (name, v / ref.tol)
        assert 0.5 * g["true_residual"][name] <= v <= 2.0 * g["true_residual"][name], (name, v, g["true_residual"][name])


@pytest.mark.parametrize("case", R.B_CASES, ids=_ID)
def test_what_the_oracle_does_with_a_tolerance_that_cannot_be_met(case, golden):
    """Group B on the oracle: at rtol = 1e-17 KrylovKit's restatement uses its 3 cycles up unconverged (every cycle exhausts the space and
    fails the explicit check: 3 (n + 1) + 1 applications or a few less).  The IterativeSolvers restatement clamps its restart length to n, so
    its first cycle ends at step n with an estimate still above the tolerance, and it reports ``converged`` at the end of the second, after
    2 n iterations, on the estimate alone.  The library does not clamp and is NOT expected to give these counts (test_gpu_krylov_exhaustion:
    B_OUTCOMES); what the two share is that the estimate-stopping flavor claims convergence at a breakdown."""
    n = case.n
    o = R.oracle_unattainable(case)
    ok, nops = o["outcome"]["krylovkit"]
    assert not ok and 2 * (n + 1) < nops <= 3 * (n + 1) + 1, o
    assert o["outcome"]["iterativesolvers"] == [True, 2 * n], o
    g = golden[R.b_label(case)]
    assert g["n"] == n and g["outcome"] == o["outcome"], (g, o)
    for name, v in o["true_residual"].items():
        assert v <= 1e-8, (name, v)
        assert 0.5 * g["true_residual"][name] <= v <= 2.0 * g["true_residual"][name], (name, v, g["true_residual"][name])


def test_option_defaults_the_gpu_module_puts_back_are_the_library_s():
    """tests/test_gpu_krylov_exhaustion.py puts an option back to the value it read, and to DEFAULTS where the option was never set on the
    context: those constants must be the defaults the library's sources give at the places that read the options."""
    import glob
    import os
    import re

    import test_gpu_krylov_exhaustion as T
    src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(R.ROOT, "bifurcationkit.jl_amd", "csrc", "*.h*"))))
    for key, value in T.DEFAULTS.items():
        found = re.findall(r'opt\("%s", (-?[0-9.]+)\)' % key, src)
        assert found and all(float(v) == value for v in found), (key, value, found)


def test_group_c_keeps_exactly_the_certified_candidates():
    passed = []
    for sid in R.C_CANDIDATE_SIDS:
        marks = [R.certify(c) for c in R.c_cases(sid)]
        if all(b >= 1e3 and a <= 1e-3 for b, a in marks):
            passed.append(sid)
    assert tuple(passed) == R.C_SIDS
    assert sum(s.startswith("sh-") for s in passed) >= 2 and sum(s.startswith("cglp-") for s in passed) >= 1


def test_tight_tolerance_case_is_where_the_block_restatement_needs_a_second_cycle(golden):
    """(4,3,3) with the DCT preconditioner at rtol = 1e-12: the space still runs out at step n, the step-by-step restatement takes n + 2
    applications, the block restatement fails its explicit check and starts a second cycle."""
    case = R.C_TIGHT_CASE
    before, at = R.certify(case)
    assert before >= 1e3 and at <= 1e-3, (before, at)
    o = R.oracle_gmres(case)
    assert all(o["converged"].values())
    c = o["counts"]
    assert c["krylovkit"] == case.n + 2 == 38
    assert c["block"] > c["krylovkit"] + 2, c                 # a second cycle, not a step more
    assert golden[case.cid]["counts"] == c


def test_the_case_that_ends_inside_a_block_ends_at_step_n_minus_one(golden):
    """Group G's fold case: the tolerance sits between the residuals at steps n - 2 and n - 1 with more than 5 % on either side (both are
    O(1) numbers far from rounding), so every restatement stops at step n - 1 = 4: 6 applications in the KrylovKit count."""
    case = R.G_INSIDE_CASE
    ref = R.reference(case)
    res = R.gmres_residuals_mp(ref.A, ref.rhs)
    n = case.n
    assert res[n - 2] >= 1.05 * ref.tol and res[n - 1] <= 0.95 * ref.tol, (res[n - 2] / ref.tol, res[n - 1] / ref.tol)
    o = R.oracle_gmres(case)
    assert all(o["converged"].values())
    assert o["counts"] == dict(krylovkit=n + 1, block=n + 1, iterativesolvers=n - 1, krylovjl=n - 1) == golden[case.cid]["counts"]


@pytest.mark.parametrize("label,kind,case", R.e_cases(), ids=[e[0] for e in R.e_cases()])
def test_symmetric_case_is_an_exhaustion_case(label, kind, case, golden):
    n = case.n
    _, _, J = R.state(case.sid)
    assert np.array_equal(J, J.T)
    ref = R.reference(case)
    if label.endswith("spd"):
        assert np.linalg.eigvalsh(ref.A).min() >= 0.999          # (lambda_max + 1) I - J: smallest eigenvalue 1
    before, at = R.certify(case)       # MINRES minimises the same residual as GMRES; CG's residual is never below it
    assert before >= 1e3 and at <= 1e-3, (label, before, at)
    o = R.oracle_symmetric(kind, case)
    assert o["converged"] and o["count"] == n, o
    assert golden[label]["counts"] == {kind: n} and golden[label]["n"] == n
    assert o["true_residual"] <= 1.5 * ref.tol


@pytest.mark.parametrize("case", [R.Case("sh1d-5"), R.Case("sh1d-33", 0.3, 0.9), R.Case("sh1d-63"), R.Case("cgl-4x4", 0.3, 0.9),
                                  R.Case("sh-4x3x3", 0.0, 1.0, "pl_kk"), R.Case("cglp-3x3", 0.3, 0.9, "pl_is"),
                                  R.Case("sh1d-33", form="bordered"), R.Case("sh-3x3", form="bordered_pl")], ids=_ID)
def test_refined_dense_solve_agrees_with_the_mpmath_solve(case):
    """The dense solution the GPU tests measure errors against (float64 LU + longdouble refinement) next to mpmath's LU at 50 digits."""
    ref = R.reference(case)
    xm = R.solve_mp(ref.A, ref.rhs)
    d = np.asarray(ref.x - xm, dtype=np.float64)
    cond = ref.norm2 / ref.sigma_min
    assert np.linalg.norm(d) <= 4.0 * case.n * R.EPSLD * cond * float(np.linalg.norm(np.asarray(xm, dtype=np.float64)))
    assert ref.residual(ref.x) <= 64 * case.n * R.EPSLD * ref.norm2 * float(np.linalg.norm(np.asarray(xm, dtype=np.float64)))
