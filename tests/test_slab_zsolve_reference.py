"""CPU pins of the long-double reference of the slab z-solve (tests/slab_zsolve_ref.py) and of the bookkeeping of
tests/test_gpu_slab_zsolve.py (no GPU):

* its tridiagonal solves against the spectral form of the same inverse, dense and in long double (dct_dense_ref.cosine_matrix);
* its Woodbury path against its exact inverse -- in long double the identity holds to the restatement's float64 error scaled by
  the ratio of the two machine precisions (2^-11);
* oracle/slab_zsolve.py (slab_zsolve, slab_zsolve_split) and its exact_zsolve against it, on the line sets of the GPU tests -- the
  float64 restatement's own error per (h, s), which the GPU tests use as the yardstick;
* the capacitance matrix against K = G^-1 + U' B^-1 U built from explicit dense B_r^-1 and explicit u, w vectors, M = B + U G U'
  itself, and K nu = U' B^-1 f for the nu of the reference;
* mutations: a wrong plane order in G_bt, a dropped (-1)^m in C and a round-robin owner map each make the matching check fail;
  a TRANSPOSED E does not, and cannot: with equal slabs E is symmetric (test_the_coupling_block_is_symmetric);
* the two definitions of SlabK (dct.hip, dct_slab.hip) agree field for field with each other and with the mirror of
  tests/slab_abi.py, DctSlabHalf (ops.h) with its mirror; every mangled name resolves; kSlabMaxFaces is the mirror's;
* the two table fill functions (host code) against long-double formulas.

Measured here (worst over the shapes below, per line, relative to the line's max|x|), per (h, s) in the order of HS_CASES:
tridiagonal against dense 9.1e-19, 1.9e-18, 8.3e-18, 9.6e-19, 2.3e-17; the reference's Woodbury path against its exact inverse 5.6e-19,
8.1e-17, 5.2e-14, 2.1e-18, 1.3e-12; the float64 restatement 7.5e-16, 4.9e-13, 4.7e-11, 4.7e-15, 4.1e-9 (both forms alike) and its
exact_zsolve at most 2.6e-15.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import slab_abi
import slab_zsolve_ref as zr
from dct_dense_ref import cosine_matrix
from oracle import slab_zsolve as osz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc")
LD = np.longdouble
EPS = zr.EPS

# (nx, ny, nl, R) -- shapes of the GPU tests' whole solves small enough for the dense long-double products
SHAPES = [(48, 2, 8, 16), (12, 4, 16, 3), (16, 4, 64, 2), (16, 5, 16, 5)]
# the float64 restatement's error per line allowed here: 4 eps times the condition ((1 + 8a)^2 + s) / s of the line's system at its
# worst c -- what a float64 solve may leave; the figures measured are in the module docstring
RESTATEMENT_BOUND = {(h, s): 4 * EPS * ((1 + 8 / h ** 2) ** 2 + s) / s for h, s in zr.HS_CASES}
FLOOR = 256 * EPS


@functools.lru_cache(maxsize=None)
def _case(shape, hs):
    nx, ny, nl, R = shape
    h, s = hs
    a = 1.0 / (h * h)
    lam0, lam1, c, ks = zr.line_set(nx, ny, h, nl * R)
    F = np.random.default_rng(nl * 100 + R).standard_normal((nl * R, c.size))
    xe = zr.exact_zsolve(F, c, s, a)
    return a, c, F, xe, np.abs(xe).max(axis=0)


def _per_line(x, ref, scale):
    return (np.abs(x - ref).max(axis=0) / scale).astype(float)


def _restatement(shape, hs):
    """max over the lines of the error of the two float64 forms, and of the oracle's exact_zsolve."""
    a, c, F, xe, sc = _case(shape, hs)
    R, s = shape[3], hs[1]
    e = np.zeros((3, c.size))
    for l in range(c.size):
        for i, x in enumerate((osz.slab_zsolve(F[:, l], c[l], s, R, a), osz.slab_zsolve_split(F[:, l], c[l], s, R, a),
                               osz.exact_zsolve(F[:, l], c[l], s, a))):
            e[i, l] = float(np.abs(x - xe[:, l]).max() / sc[l])
    return e.max(axis=1)


@pytest.mark.parametrize("hs", zr.HS_CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_against_dense_spectral_form_and_restatement(shape, hs):
    """The ruler is finer than what it measures: the reference's two errors stay below 1 % of max(restatement's error, 256 eps) -- the
    yardstick of the GPU tests -- and the restatement stays within the figures it was studied at."""
    a, c, F, xe, sc = _case(shape, hs)
    nz, s = F.shape[0], hs[1]
    T = cosine_matrix(nz, LD)
    sym = (c.astype(LD)[None, :] + zr.lam_neumann(nz, a)[:, None]) ** 2 + LD(s)
    dense = T.T @ ((T @ F.astype(LD)) / sym)
    e_dense = _per_line(xe, dense, sc).max()
    xs, _ = zr.slab_zsolve(F, c, s, shape[3], a)
    e_wood = _per_line(xs, xe, sc).max()
    r_gather, r_split, r_exact = _restatement(shape, hs)
    print(f"slab_ref {shape} h={hs[0]:.4f} s={hs[1]}: tridiagonal-dense {e_dense:.2e} woodbury-exact {e_wood:.2e} "
          f"restatement {r_gather:.2e} / {r_split:.2e} exact_zsolve {r_exact:.2e}")
    yard = max(r_gather, r_split, FLOOR)
    assert e_dense <= 1e-2 * yard and e_wood <= 1e-2 * yard, (e_dense, e_wood, yard)
    assert max(r_gather, r_split) <= RESTATEMENT_BOUND[hs], (r_gather, r_split)
    assert r_exact <= 64 * EPS, r_exact


# ------------------------------------------------------------------------------------------------- K from explicit dense pieces
def _dense_pieces(c, s, nl, R, a):
    """Per line, everything explicit in long double: M[nz][nz], B (block diagonal), U[nz][2 (R - 1)], G (block diagonal), B^-1."""
    nz, L, nf = nl * R, c.size, R - 1
    cl, al = c.astype(LD), LD(a)

    def op(n):                                   # (c I + D_n)^2 + s I, [n][n][line]
        Dn = np.zeros((n, n), dtype=LD)
        for k in range(n):
            Dn[k, k] = -2 * al if 0 < k < n - 1 else -al
            if k + 1 < n:
                Dn[k, k + 1] = Dn[k + 1, k] = al
        T = Dn[:, :, None] + np.eye(n, dtype=LD)[:, :, None] * cl
        return np.einsum("ijl,jkl->ikl", T, T) + np.eye(n, dtype=LD)[:, :, None] * LD(s)
    M, Br = op(nz), op(nl)
    Bri = zr.solve_lines(Br, np.repeat(np.eye(nl, dtype=LD)[:, :, None], L, axis=2))
    B, Bi = np.zeros_like(M), np.zeros_like(M)
    for r in range(R):
        B[r * nl:(r + 1) * nl, r * nl:(r + 1) * nl] = Br
        Bi[r * nl:(r + 1) * nl, r * nl:(r + 1) * nl] = Bri
    U, G, Gi = np.zeros((nz, 2 * nf, L), dtype=LD), np.zeros((2 * nf, 2 * nf, L), dtype=LD), np.zeros((2 * nf, 2 * nf, L), dtype=LD)
    for i in range(nf):
        p = (i + 1) * nl - 1
        q = p + 1
        U[p - 1, 2 * i], U[p, 2 * i], U[q, 2 * i], U[q + 1, 2 * i] = al, cl - al, -(cl - al), -al          # u
        U[p, 2 * i + 1], U[q, 2 * i + 1] = 1, -1                                                          # w
        G[2 * i:2 * i + 2, 2 * i:2 * i + 2] = np.array([[0, -al], [-al, 2 * al * al]], dtype=LD)[:, :, None]
        Gi[2 * i:2 * i + 2, 2 * i:2 * i + 2] = np.array([[-2, -1 / al], [-1 / al, 0]], dtype=LD)[:, :, None]
    return M, B, Bi, U, G, Gi


@pytest.mark.parametrize("hs", zr.HS_CASES)
@pytest.mark.parametrize("nl,R", [(8, 2), (8, 3), (8, 5), (16, 3)])
def test_capacitance_matrix_against_explicit_dense_pieces(nl, R, hs):
    """M = B + U G U' entry by entry; K of the reference (spectral sums A, C, the face maps, D0 / E / E' placement) equals
    G^-1 + U' B^-1 U with B_r^-1 from Gaussian elimination; K nu = U' B^-1 f for the reference's nu.  Bounds: M = B + U G U' to
    2^-60 of the largest entry per line (sums of a few products); K to 16 x 2^-64 times the condition ((1 + 8a)^2 + s) / s of B_r, which is
    what the elimination's B_r^-1 carries, relative to the largest entry of K per line; the residual of nu within the same figure of
    the componentwise size |K| |nu| + |g|."""
    h, s = hs
    a = 1.0 / (h * h)
    _, _, c, _ = zr.line_set(12, 2, h, nl * R)
    M, B, Bi, U, G, Gi = _dense_pieces(c, s, nl, R, a)
    ugu = np.einsum("ipl,pql,jql->ijl", U, G, U)
    assert (np.abs(M - B - ugu).max(axis=(0, 1)) <= 2.0 ** -60 * np.abs(M).max(axis=(0, 1))).all()
    Kd = Gi + np.einsum("pil,pql,qjl->ijl", U, Bi, U)
    D0, E = zr.reduced_blocks(c, s, nl, a)
    K = zr.assemble_K(D0, E, R)
    tol = 16 * 2.0 ** -64 * ((1 + 8 * a) ** 2 + s) / s
    err = (np.abs(K - Kd).max(axis=(0, 1)) / np.abs(Kd).max(axis=(0, 1))).astype(float)
    print(f"slab_ref K nl={nl} R={R} h={h:.4f} s={s}: {err.max():.2e} (bound {tol:.2e})")
    assert (err <= tol).all(), err.max()
    F = np.random.default_rng(7).standard_normal((nl * R, c.size))
    _, mid = zr.slab_zsolve(F, c, s, R, a)
    g = np.einsum("pil,pql,ql->il", U, Bi, F.astype(LD))
    res = np.abs(np.einsum("ijl,jl->il", Kd, mid["nu"]) - g)
    den = np.einsum("ijl,jl->il", np.abs(Kd), np.abs(mid["nu"])) + np.abs(g)
    assert (res <= tol * den).all(), float((res / den).max())
    # a wrong plane order in G_bt or a dropped (-1)^m is seen here (C enters E only, and with one face there is no coupling block)
    for flaw in (["planes", "sign"] if R >= 3 else []):
        Kf = zr.assemble_K(*zr.reduced_blocks(c, s, nl, a, flaw), R)
        assert ((np.abs(Kf - Kd).max(axis=(0, 1)) / np.abs(Kd).max(axis=(0, 1))).astype(float) > tol).any(), flaw


# --------------------------------------------------------------------------------------------------------------------- mutations
@pytest.mark.parametrize("flaw", ["planes", "sign"])
@pytest.mark.parametrize("hs", zr.HS_CASES)
def test_a_broken_reference_disagrees_with_the_restatement(hs, flaw):
    """With the face planes of G_bt paired in the wrong order or C's (-1)^m dropped the reference leaves the restatement (and the exact inverse) by far more than the
    restatement's bound on some line; unbroken it agrees (test_reference_against_dense_spectral_form_and_restatement)."""
    shape = (12, 4, 16, 3)
    a, c, F, xe, sc = _case(shape, hs)
    xs, _ = zr.slab_zsolve(F, c, hs[1], shape[3], a, flaw=flaw)
    e = _per_line(xs, xe, sc)
    rest = np.array([np.abs(osz.slab_zsolve(F[:, l], c[l], hs[1], shape[3], a) - xs[:, l]).max() / sc[l] for l in range(c.size)])
    print(f"slab_ref flaw {flaw} h={hs[0]:.4f} s={hs[1]}: against exact {e.max():.2e}, against the restatement {float(rest.max()):.2e}")
    assert e.max() > 1e3 * RESTATEMENT_BOUND[hs] and rest.max() > 1e3 * RESTATEMENT_BOUND[hs]


@pytest.mark.parametrize("hs", zr.HS_CASES)
def test_the_coupling_block_is_symmetric(hs):
    """E = P_bot' G_bt P_top = -P_top' [[C11, C01], [C01, C00]] P_top for equal slabs: E' = E, so transposing E in the reference (or in
    the device's recurrence, which forms tr2(E)) changes the solution by rounding only -- there is no orientation to get wrong."""
    shape = (12, 4, 16, 3)
    a, c, F, xe, sc = _case(shape, hs)
    D0, E = zr.reduced_blocks(c, hs[1], shape[2], a)
    A, _ = zr.face_green(c, hs[1], shape[2], a)
    Pt, Pb = zr.face_maps(c, a)
    # E cancels from terms of this size: the alternating sums C from summands that add up to A00, A11, then the products with a, c - a
    size = np.broadcast_to(np.maximum(A[0, 0], A[1, 1]), A.shape)
    terms = np.einsum("pil,pql,qjl->ijl", np.abs(Pb), size, np.abs(Pt)).max(axis=(0, 1))
    assert (np.abs(E[0, 1] - E[1, 0]) <= 2.0 ** -60 * terms).all()
    xs, _ = zr.slab_zsolve(F, c, hs[1], shape[3], a, flaw="E")
    assert _per_line(xs, xe, sc).max() <= 1e-2 * max(_restatement(shape, hs)[0], FLOOR)


def test_owner_layout_and_its_mutation():
    """[owner][4][Lr] with owner = line // Lr, written out index by index; the round-robin deal is another layout."""
    R, Lr = 3, 16
    x = np.arange(4 * R * Lr, dtype=float).reshape(4, R * Lr)
    want = np.empty((R, 4, Lr))
    for line in range(R * Lr):
        for q in range(4):
            want[line // Lr, q, line % Lr] = x[q, line]
    assert np.array_equal(zr.to_owners(x, R), want) and np.array_equal(zr.from_owners(want), x)
    assert not np.array_equal(zr.to_owners(x, R, flaw="owner"), want)
    # the restatement's face data, dealt to the owners and collected again, is the reference's right-hand side
    nl, hs = 16, zr.HS_CASES[1]
    a, c, F, xe, sc = _case((12, 4, nl, R), hs)
    _, mid = zr.slab_zsolve(F, c, hs[1], R, a)
    got = np.stack([zr.from_owners(zr.to_owners(mid["parts"][r], R)) for r in range(R)])
    assert np.array_equal(zr.face_rhs(got), mid["g"])
    # (1e-9: the float64 local solves of the restatement on the benchmark's mesh; a wrong slot is an error of order one)
    Yo = osz.local_solve(F[:, 5].reshape(R, nl), c[5], hs[1], nl, a)
    _, _, Pt, Pb = osz.reduced_blocks(c[5], hs[1], nl, a)
    go = np.concatenate([Pt.T @ Yo[i, nl - 2:] + Pb.T @ Yo[i + 1, :2] for i in range(R - 1)])
    assert np.abs(go - mid["g"][:, 5]).max() <= 1e-9 * np.abs(go).max()


# ------------------------------------------------------------------------------------------------------------ structs and symbols
def parse_struct(src, name):
    """[(field, C type, default or None)] of `struct name { ... };`: comments stripped, `int nx, ny;` split up."""
    body = re.search(r"struct %s \{(.*?)\n\};" % name, src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    defaults = {"0.0": 0.0, "0": 0, "false": False, "nullptr": "nullptr"}
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"((?:const )?(?:int|size_t|double|bool)\*?) (.+)", decl)
        assert m, f"{name}: a declaration this parser does not know: {decl!r}"
        for item in m.group(2).split(","):
            field, _, dflt = item.partition("=")
            out.append((field.strip(), m.group(1), defaults[dflt.strip()] if dflt.strip() else None))
    return out


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_two_slabk_definitions_and_the_mirror_agree():
    a, b = parse_struct(_src("dct.hip"), "SlabK"), parse_struct(_src("dct_slab.hip"), "SlabK")
    assert a == b, (a, b)
    assert a == slab_abi.SLAB_K
    assert [(f, t) for f, t in slab_abi.SlabK._fields_] == [(f, slab_abi.CTYPES[t]) for f, t, _ in a]
    with pytest.raises(TypeError):
        slab_abi.SlabK(no_such_field=1)


def test_dct_slab_half_mirror_equals_ops_h():
    declared = parse_struct(_src("ops.h"), "DctSlabHalf")
    assert [(f, t) for f, t, _ in declared] == [(f, t) for f, t, _ in slab_abi.DCT_SLAB_HALF]
    for (f, _, want), (_, _, got) in zip(declared, slab_abi.DCT_SLAB_HALF):      # 0 == 0.0 == False in Python: compare the types too
        assert want == got and type(want) is type(got), (f, want, got)
    assert [(f, t) for f, t in slab_abi.DctSlabHalf._fields_] == [(f, slab_abi.CTYPES[t]) for f, t, _ in declared]
    obj = slab_abi.DctSlabHalf()                 # zero-initialised = every default member value
    for f, _, d in declared:
        assert not getattr(obj, f), f


def test_constants_match_the_sources():
    assert f"constexpr int kSlabMaxFaces = {slab_abi.K_SLAB_MAX_FACES};" in _src("dct_slab.hip")
    assert "P.R - 1 > kSlabMaxFaces" in _src("dct_slab.hip")       # the launcher's own guard


def _lib():
    from bk_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    return ctypes.CDLL(_lib.LIB_PATH)


def test_every_launcher_symbol_resolves():
    lib = _lib()
    missing = [m for m in slab_abi.LAUNCHERS if not hasattr(lib, m)]
    assert not missing, f"launchers whose mangled name (signature) changed: {missing}"
    slab_abi.Launchers(lib)


# --------------------------------------------------------------------------------------------------------------------- the tables
def table_errors(fn, nl, az):
    """Worst error of the filled tables in units of eps: lam_loc relative to the entry; phi and the twiddles relative to the
    entry's amplitude (s_m, 1) -- an oscillating entry next to a zero of the cosine carries the absolute rounding of its argument,
    which is what the transforms and the spectral sums see."""
    lam, phi = fn.slab_tables(nl, az)
    tw = fn.twiddle_table(nl)
    lam_ref, phi_ref = zr.lam_neumann(nl, az), zr.basis_planes01(nl)
    tw_ref, used = zr.twiddles(nl)
    assert lam[0] == 0.0 and tw.shape == tw_ref.shape and np.isfinite(tw).all() and np.isfinite(lam).all() and np.isfinite(phi).all()
    assert (tw[~used] == 0.0).all()                                                        # the padding slots
    e_lam = float((np.abs(lam[1:] - lam_ref[1:]) / np.abs(lam_ref[1:])).max() / EPS)
    amp = np.sqrt(LD(2) / LD(nl)) * np.ones(nl, dtype=LD)
    amp[0] = np.sqrt(LD(1) / LD(nl))
    e_phi = float((np.abs(phi - phi_ref) / amp).max() / EPS)
    e_tw = float(np.abs(tw - tw_ref).max() / EPS)
    return e_lam, e_phi, e_tw


@pytest.mark.parametrize("h", [1.0, zr.H_BENCH, 0.0625])
@pytest.mark.parametrize("nl", [8, 64, 512])
def test_table_fill_functions_against_long_double(nl, h):
    """4 ulp (tests/test_gpu_slab_zsolve.py runs the same check on the library the GPU tests load)."""
    e = table_errors(slab_abi.Launchers(_lib()), nl, 1.0 / (h * h))
    print(f"slab tables nl={nl} h={h:.4f}: lam_loc {e[0]:.2f} phi {e[1]:.2f} twiddles {e[2]:.2f} eps")
    assert max(e) <= 4.0, e
