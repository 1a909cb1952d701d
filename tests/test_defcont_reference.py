"""CPU tests of the deflated-continuation restatement (tests/defcont_ref.py) and of the host side of
bk_amd.deflated_continuation: the counter-based uniform against integer arithmetic and its first two moments, the loop on the
reference's scalar test problem against its closed-form solutions, the loop on 16 x 16 Swift-Hohenberg against the oracle's F,
the defaults of DefCont, and the C boundary."""
import math
import os

import numpy as np
import pytest

import defcont_ref as R
import multicontinuation_ref as MC

TOL = 1e-10


# ------------------------------------------------------------------------------------------ 1: the hash
HASH_CASES = [(0, 0), (0, 1), (1, 0), (2024, 12345), (2 ** 64 - 1, 0), (2 ** 64 - 1, 2 ** 40 + 7), (0x9E3779B97F4A7C15, 2 ** 31),
              (123456789, 2 ** 31 - 1), (7, 2 ** 32), (7, 2 ** 32 + 1), (42, 2 ** 53), (42, 2 ** 63 - 2), (5, 255), (5, 256), (5, 257),
              (2 ** 63, 4097), (2 ** 33 + 1, 1 << 22), (987654321987654321, 3), (31337, 65535), (31337, 65536)]


def test_hash_matches_integer_arithmetic():
    """Twenty (seed, index) pairs -- small, at the 2^31 / 2^32 / 2^53 / 2^63 boundaries, seeds up to 2^64 - 1 -- in NumPy uint64
    arithmetic against Python integers reduced mod 2^64, exactly; the value lies in [0, 1) and is a multiple of 2^-53; the driver's
    own seed derivation equals the restatement's; three values are pinned as literals."""
    from bk_amd import deflated_continuation as DC
    for seed, g in HASH_CASES:
        u = float(R.hash_u01(seed, np.array([g], dtype=np.uint64))[0])
        assert u == R.hash_u01_int(seed, g), (seed, g)
        assert 0.0 <= u < 1.0 and (u * 2.0 ** 53).is_integer()
    for seed, b, c in [(0, 0, 0), (2024, 3, 17), (2 ** 64 - 1, 40, 749)]:
        assert DC.derive_seed(seed, b, c) == R.derive_seed(seed, b, c) < 2 ** 64
    assert len({R.derive_seed(2024, b, c) for b in range(40) for c in range(50)}) == 2000
    assert [R.hash_u01_int(s, g) for s, g in HASH_CASES[:3]] == HASH_LITERALS
    x = np.array([0.25, -1.0, 3.0])
    assert np.array_equal(R.perturb(x, -3.5, 9, 100), x + np.float64(-3.5) * np.array([R.hash_u01_int(9, 100 + i) for i in range(3)]))


# U(0, 0) is splitmix64's first output for seed 0, 0xE220A8397B1DCDAF, shifted right by 11
HASH_LITERALS = [0.8833108082136426, 0.43152799704850997, 0.5665615751722809]


def test_hash_moments_and_distinct_values():
    """2^20 consecutive indices: mean within 5 standard errors of 1/2 (sigma / sqrt(n), sigma^2 = 1/12), variance within 5 standard
    errors of 1/12 (the variance of (U - 1/2)^2 is 1/180), no value twice; the same for a second seed and a distant offset."""
    n = 1 << 20
    for seed, off in [(2024, 0), (1, 2 ** 40)]:
        u = R.hash_u01(seed, np.uint64(off) + np.arange(n, dtype=np.uint64))
        assert abs(u.mean() - 0.5) <= 5 * math.sqrt(1 / 12 / n)
        assert abs(np.mean((u - 0.5) ** 2) - 1 / 12) <= 5 * math.sqrt(1 / 180 / n)
        assert np.unique(u).size == n


def test_pieces_with_offsets_equal_the_whole():
    x = np.linspace(-1, 1, 1001)
    whole = R.perturb(x, 0.1, 77, 12345)
    parts = np.concatenate([R.perturb(x[a:b], 0.1, 77, 12345 + a) for a, b in [(0, 1), (1, 400), (400, 1001)]])
    assert np.array_equal(whole, parts)


# ------------------------------------------------------------------------------------------ 2: the scalar problem
SCALAR = dict(p0=0.3, ds=-0.002, p_min=-0.8, max_steps=800, tol=TOL, max_iterations=15, max_branches=6, power=2, alpha=0.001,
              norm=R.norminf)
OFFSETS = [0.3, -0.3, 0.6, -0.1, 0.15]         # the deterministic perturbation: call k adds OFFSETS[k % 5]


def _near_closed_form(run, roots):
    return max(min(abs(u[0] - q) for q in roots(p)) for b in run["branches"] for p, u in zip(b["param"], b["states"]))


@pytest.mark.filterwarnings("ignore:invalid value encountered")        # |M| |F| = inf x 0 on a deflated state
def test_scalar_problem_identity_perturbation_follows_two_branches():
    """F2 of test/continuation/simple_continuation.jl:408-414, roots {0, 0.05}, DeflationOperator(2, 0.001), ds = -0.002, p from
    0.3 to -0.8, max_branches = 6, the default identity perturbation: every seek starts on a deflated state (M infinite), so no
    branch appears -- 2 branches; u = 0 is followed over all 550 steps; every recorded point is within 1e-8 of a closed-form root
    at its parameter."""
    F, J, roots = R.scalar_problem()
    kw = {k: v for k, v in SCALAR.items() if k != "p0"}
    run = R.deflated_continuation(F, J, [np.array([0.0]), np.array([0.05])], SCALAR["p0"], **kw)
    assert len(run["branches"]) == 2
    b0 = run["branches"][0]
    assert len(b0["param"]) == 550 and b0["active"] and all(u[0] == 0.0 for u in b0["states"])
    assert abs(b0["param"][-1] - (-0.8)) < 1e-12
    assert all(s["reason"] == 1 and s["itnewton"] == 0 for s in run["seeks"]) and run["seeks"]
    worst = _near_closed_form(run, roots)
    print(f"identity: worst distance to a closed-form root {worst:.3e}; branch lengths {[len(b['param']) for b in run['branches']]}")
    assert worst <= 1e-8


def test_scalar_problem_offset_perturbation_finds_four_of_five_roots():
    """The same down to p = 0.18 (60 steps; the five roots exist and are simple on that stretch) with the offsets above: at
    p = 0.2 at least 4 of the 5 closed-form roots are held by a branch, and every recorded point is within 1e-8 of one."""
    F, J, roots = R.scalar_problem()
    count = [0]

    def offset(x, p, id):
        count[0] += 1
        return x + OFFSETS[(count[0] - 1) % len(OFFSETS)]

    kw = {k: v for k, v in SCALAR.items() if k != "p0"}
    kw.update(max_steps=60, perturb_solution=offset)
    run = R.deflated_continuation(F, J, [np.array([0.0]), np.array([0.05])], SCALAR["p0"], **kw)
    at = [u[0] for b in run["branches"] for p, u in zip(b["param"], b["states"]) if abs(p - 0.2) < 1e-9]
    held = [q for q in roots(0.2) if any(abs(a - q) <= 1e-8 for a in at)]
    worst = _near_closed_form(run, roots)
    print(f"offset: {len(run['branches'])} branches, roots held at p = 0.2: {sorted(held)} of {sorted(roots(0.2))}; worst {worst:.3e}")
    assert len(roots(0.2)) == 5 and len(held) >= 4
    assert worst <= 1e-8
    assert len(run["branches"]) > 2


# ------------------------------------------------------------------------------------------ 3: Swift-Hohenberg 16 x 16
def test_sh_finds_disconnected_branches_below_the_branch_point():
    """16 x 16 SH (nu = 1.3) from u = 0 at l* - 0.035, ds = 0.01, 8 steps, max_branches = 12: the trivial branch has all 8 points;
    at the first parameter value (< l*) at least 2 non-trivial branches; every recorded point a zero of the oracle's F to tol in
    the inf-norm; the states at one parameter value pairwise >= tol apart in the inf-norm."""
    c, run = MC.sh_case(2), R.sh_run()
    p1 = c["p"] - R.SH_RUN["back"] + R.SH_RUN["ds"]
    assert p1 < c["p"]
    b0 = run["branches"][0]
    assert len(b0["param"]) == 8 and all(n == 0.0 for n in b0["normu"])
    first = [b for b in run["branches"][1:] if b["param"][0] == b0["param"][0]]
    assert abs(b0["param"][0] - p1) < 1e-14 and len(first) >= 2 and all(b["normu"][0] > 0.5 for b in first)
    worst = max(R.norminf(c["F"](u, p)) for b in run["branches"] for p, u in zip(b["param"], b["states"]))
    assert worst < TOL
    for p in b0["param"]:
        states = [u for b in run["branches"] for q, u in zip(b["param"], b["states"]) if q == p]
        assert R.pairwise_min_inf(states) >= TOL
    print(f"SH 16 x 16: {len(run['branches'])} branches, {len(first)} non-trivial at l = {p1:.4f} < l* = {c['p']:.4f} with |u|_inf "
          f"{sorted(round(b['normu'][0], 3) for b in first)}; {sum(b['active'] for b in run['branches'])} active at the end; worst |F| {worst:.2e}")


# ------------------------------------------------------------------------------------------ 4: host side of the driver
def test_defcont_defaults_and_refusals():
    """The reference's defaults (src/DeflatedContinuation.jl:14-33); stop_plain follows alpha; an operator without roots raises
    as the reference does (:226-228)."""
    from bk_amd import continuation as Cn
    from bk_amd import deflated_continuation as DC
    from bk_amd import hip
    a = DC.DefCont()
    assert (a.max_branches, a.seek_every_step, a.max_iter_defop, a.stop_plain) == (100, 1, 5, None)
    x = object()
    assert a.perturb_solution(x, 0.1, 3) is x and a.accept_solution(x, 0.1) is True
    op = hip.DeflationOperator(2, 1.0, [], autodiff=True)
    a.update_deflation_op(op, x, 0.1)
    assert op.roots == [x]
    for empty in (None, hip.DeflationOperator(2, 1.0, [], autodiff=True)):
        with pytest.raises(ValueError, match="at least one guess"):
            DC.deflated_continuation(None, DC.DefCont(deflation_operator=empty), Cn.ContinuationPar())
    with pytest.raises(ValueError, match="autodiff"):
        DC.deflated_continuation(None, DC.DefCont(deflation_operator=hip.DeflationOperator(2, 1.0, [x])), Cn.ContinuationPar())
    with pytest.raises(ValueError, match="normC"):
        DC.deflated_continuation(None, DC.DefCont(deflation_operator=op), Cn.ContinuationPar(), normC=lambda v: 0.0)
    import bk_amd
    assert "deflated_continuation" in bk_amd.__all__


# ------------------------------------------------------------------------------------------ 5: the C boundary
def test_library_exports_the_defcont_entries():
    """The three entries are declared in the header with their reference lines, bound by ctypes and exported by the built library;
    the result struct has the layout of the header; the ABI version stays."""
    import ctypes
    import re

    from bk_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bkhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    nargs = dict(bk_deflation_dist=7, bk_vec_perturb=6, bk_defcont_seek=19)
    for name, k in nargs.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == k, name
        assert name in _lib.SIGNATURES and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == k, name
    assert "src/DeflatedContinuation.jl:269-286" in hdr and "examples/SH2d-fronts.jl:181" in hdr
    S = _lib.DefContSeekResult
    fields = re.search(r"typedef struct \{([^}]*)\} bk_defcont_seek_result;", src).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in S._fields_]
    assert ctypes.sizeof(S) == 6 * 4 + 4 * 8 and S.M.offset == 24
    assert re.search(r"#define\s+BK_ABI_VERSION\s+6\b", hdr) and _lib.BK_ABI_VERSION == 6
    mk = open(os.path.join(root, "bifurcationkit.jl_amd", "csrc", "Makefile")).read()
    assert "defcont.hip" in mk and "-ffp-contract=off" in mk
