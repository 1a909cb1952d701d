"""Long-double restatement of the slab z-solve of the distributed Swift-Hohenberg preconditioner (csrc/dct_slab.hip, the slab half
passes of csrc/dct_fast.hip), vectorised over the (kx, ky) lines: helper of test_slab_zsolve_reference.py and
test_gpu_slab_zsolve.py.  No GPU, no scipy.  The derivation is oracle/slab_zsolve.py's:

    M = (c I + D)^2 + s I  on all nz planes,   B = blockdiag_r((c I + D_nl)^2 + s I),   M = B + U G U',
    M^-1 f = B^-1 (f - U nu),   K nu = U' B^-1 f,   K = G^-1 + U' B^-1 U   (block tridiagonal, R - 1 block rows of 2 x 2),

with c = 1 + lam_x + lam_y per line, D the Neumann-ghost second difference scaled by a = 1 / h_z^2, and per face p | q = p + 1
w = e_p - e_q, u = a e_{p-1} + (c - a)(e_p - e_q) - a e_{q+1}, G = [[0, -a], [-a, 2 a^2]].

Every solve with M or B_r here is a pair of complex tridiagonal eliminations, ((T + i sqrt(s))(T - i sqrt(s)))^-1 with T = c I + D,
in long double: O(n) per line, so a line of 2048 planes costs what it should.  It never meets the DCT: the device kernels and
the float64 NumPy restatement (both spectral) are judged by arithmetic of another kind.  The face Green's functions A, C of the
capacitance matrix are the spectral sums of the device kernel, in long double; test_slab_zsolve_reference.py pins them to the
explicit dense B_r^-1.  Arrays carry the lines on the LAST axis; c is the float64 value the kernels form, (1 + lam0[ix]) + lam1[iy].

`flaw` (None in every use but the mutation tests of test_slab_zsolve_reference.py) breaks one thing on purpose: "E" transposes the
coupling block, "planes" pairs the face planes of G_bt in the wrong order, "sign" drops the (-1)^m of C, "owner" deals the lines out
to the owners round-robin instead of in blocks.  With equal slabs E is SYMMETRIC -- P_bot is minus P_top with its rows reversed, so
E = -P_top' S P_top with S = [[C11, C01], [C01, C00]] -- and "E" changes nothing beyond rounding: the orientation of E / E' in the
block-Thomas recurrence is not observable, which test_slab_zsolve_reference.py records.
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
H_BENCH = 2.0 * np.pi / 32                      # mesh width of the benchmark's cell
HS_CASES = [(1.0, 1.0), (H_BENCH, 1.0), (0.0625, 1.0), (1.0, 0.05), (0.0625, 0.05)]        # (h, s)


def _pi():
    return np.arccos(LD(-1))


def lam_neumann(n, a):
    """Eigenvalues -4 a sin^2(pi k / 2n) of the Neumann-ghost second difference on n planes (long double)."""
    sn = np.sin(_pi() * np.arange(n).astype(LD) / LD(2 * n))
    return -(LD(4) * LD(a)) * sn * sn


def basis_planes01(nl):
    """phi[z][m] = s_m cos(pi (2z + 1) m / 2nl), z = 0, 1: the orthonormal DCT-II basis of one slab at its first two planes."""
    m = np.arange(nl).astype(LD)
    sk = np.where(np.arange(nl) == 0, np.sqrt(LD(1) / LD(nl)), np.sqrt(LD(2) / LD(nl)))
    return np.stack([sk * np.cos(_pi() * LD(2 * z + 1) * m / LD(2 * nl)) for z in (0, 1)])


def twiddles(N):
    """The table of dct_twiddle_fill, by name: w[j] = exp(-2 pi i j / N), j < N/2, and e[k] = exp(-i pi k / 2N), k <= N/2, as
    (re, im) pairs in long double; the slot of entry j is j + j // 16 (one padding slot, zero, per 16 entries), e after w.
    Returns the table and the mask of the doubles that hold an entry."""
    twi = lambda j: j + (j >> 4)
    twl, ewl = twi(N >> 1), twi(N >> 1) + 1
    t, used = np.zeros(2 * (twl + ewl), dtype=LD), np.zeros(2 * (twl + ewl), dtype=bool)
    for j in range(N // 2):
        t[2 * twi(j)], t[2 * twi(j) + 1] = np.cos(2 * _pi() * LD(j) / LD(N)), -np.sin(2 * _pi() * LD(j) / LD(N))
        used[2 * twi(j):2 * twi(j) + 2] = True
    for k in range(N // 2 + 1):
        t[2 * (twl + twi(k))], t[2 * (twl + twi(k)) + 1] = np.cos(_pi() * LD(k) / LD(2 * N)), -np.sin(_pi() * LD(k) / LD(2 * N))
        used[2 * (twl + twi(k)):2 * (twl + twi(k)) + 2] = True
    return t, used


# ------------------------------------------------------------------------------------------------------- solves with M and B_r
def _tridiag_solve(diag, off, F):
    """Thomas elimination of the complex symmetric tridiagonal systems (diag[k, line] on the diagonal, the real scalar `off` beside
    it) for F[k, rhs, line].  No pivoting: Im(diag) = +-sqrt(s) keeps the sign through the recurrence, so |pivot| >= sqrt(s)."""
    n = F.shape[0]
    d = np.empty_like(diag)
    y = F.astype(CLD)
    d[0] = diag[0]
    for k in range(1, n):
        w = off / d[k - 1]
        d[k] = diag[k] - w * off
        y[k] -= w * y[k - 1]
    y[n - 1] /= d[n - 1]
    for k in range(n - 2, -1, -1):
        y[k] = (y[k] - off * y[k + 1]) / d[k]
    return y


def neumann_solve(F, c, s, a):
    """((c I + D_n)^2 + s I)^-1 F along axis 0 of F[n, ..., line], D_n = a tridiag(1, -2, 1) with the Neumann-ghost corners -a."""
    F = np.asarray(F)
    n, L = F.shape[0], F.shape[-1]
    F3 = F.astype(LD).reshape(n, -1, L)
    a, c = LD(a), np.asarray(c).astype(LD)
    t = np.empty((n, L), dtype=LD)
    t[:] = c - 2 * a
    t[0] = t[n - 1] = c - a
    sq = np.sqrt(LD(s))
    y = _tridiag_solve(t + 1j * sq, a, F3)
    x = _tridiag_solve(t - 1j * sq, a, y)
    return x.real.reshape(F.shape)


def exact_zsolve(F, c, s, a):
    """The exact global inverse on F[nz, ..., line]."""
    return neumann_solve(F, c, s, a)


def local_solve(F, c, s, a):
    """B^-1 on F[R, nl, ..., line]: the same operator closed at every slab face."""
    return np.stack([neumann_solve(F[r], c, s, a) for r in range(F.shape[0])])


# -------------------------------------------------------------------------------------------------------- the capacitance system
def face_green(c, s, nl, a, flaw=None):
    """A[i][j][line] = sum_m phi_m(i) phi_m(j) / ((c + lam_m)^2 + s), C the same with (-1)^m; i, j in {0, 1}: B_r^-1 between the
    planes (0, 1) and, by phi_m(nl - 1 - z) = (-1)^m phi_m(z), between them and (nl - 1, nl - 2)."""
    c = np.asarray(c).astype(LD)
    sym = 1 / ((c[:, None] + lam_neumann(nl, a)) ** 2 + LD(s))                  # [line][m]
    phi = basis_planes01(nl)
    sg = np.where(np.arange(nl) % 2 == 1, LD(-1), LD(1)) if flaw != "sign" else np.ones(nl, dtype=LD)
    A = np.array([[(sym * phi[i] * phi[j]).sum(axis=1) for j in (0, 1)] for i in (0, 1)])
    C = np.array([[(sym * sg * phi[i] * phi[j]).sum(axis=1) for j in (0, 1)] for i in (0, 1)])
    return A, C


def face_maps(c, a):
    """P_top[plane][col][line] (rows: planes nl-2, nl-1; columns u, w) and P_bot (rows: planes 0, 1): the parts of one face's (u, w)
    in the slab below it (top) and above it (bottom)."""
    c = np.asarray(c).astype(LD)
    a = LD(a)
    z, o = np.zeros_like(c), np.ones_like(c)
    return np.array([[a * o, z], [c - a, o]]), np.array([[-(c - a), -o], [-a * o, z]])


def reduced_blocks(c, s, nl, a, flaw=None):
    """D0 = G^-1 + K_ii and E = K_{i,i+1} of the capacitance matrix, [2][2][line]."""
    A, C = face_green(c, s, nl, a, flaw)
    Pt, Pb = face_maps(c, a)
    a = LD(a)
    Ginv = np.array([[-2 * np.ones_like(A[0, 0]), -np.ones_like(A[0, 0]) / a], [-np.ones_like(A[0, 0]) / a, np.zeros_like(A[0, 0])]])
    Gtt, Gbb, Gbt = A[::-1, ::-1], A, (C if flaw == "planes" else C[:, ::-1])
    q = lambda X, G, Y: np.einsum("pil,pql,qjl->ijl", X, G, Y)
    D0 = Ginv + q(Pt, Gtt, Pt) + q(Pb, Gbb, Pb)
    E = q(Pb, Gbt, Pt)                          # face i (its bottom part, in slab i + 1) x face i + 1 (its top part, in slab i + 1)
    return D0, (E.transpose(1, 0, 2) if flaw == "E" else E)


def assemble_K(D0, E, R):
    """K[row][col][line], 2 (R - 1) square: D0 on the block diagonal, E above it, E' below."""
    nf = R - 1
    K = np.zeros((2 * nf, 2 * nf, D0.shape[-1]), dtype=D0.dtype)
    for i in range(nf):
        K[2 * i:2 * i + 2, 2 * i:2 * i + 2] = D0
        if i + 1 < nf:
            K[2 * i:2 * i + 2, 2 * i + 2:2 * i + 4] = E
            K[2 * i + 2:2 * i + 4, 2 * i:2 * i + 2] = E.transpose(1, 0, 2)
    return K


def solve_lines(K, g):
    """K[n][n][line] \\ g[n][rhs][line] by Gaussian elimination with partial pivoting per line, in K's precision."""
    n, L = K.shape[0], K.shape[-1]
    A = np.concatenate([np.moveaxis(K, -1, 0), np.moveaxis(g, -1, 0)], axis=2).copy()         # [line][n][n + rhs]
    ar = np.arange(L)
    for j in range(n):
        p = j + np.abs(A[:, j:, j]).argmax(axis=1)
        rj, rp = A[ar, j].copy(), A[ar, p].copy()
        A[ar, j], A[ar, p] = rp, rj
        f = A[:, j + 1:, j] / A[:, j, j][:, None]
        A[:, j + 1:, :] -= f[:, :, None] * A[:, j, :][:, None, :]
    x = np.zeros((L, n, g.shape[1]), dtype=K.dtype)
    for j in range(n - 1, -1, -1):
        x[:, j] = (A[:, j, n:] - np.einsum("lk,lkr->lr", A[:, j, j + 1:n], x[:, j + 1:])) / A[:, j, j][:, None]
    return np.moveaxis(x, 0, -1)


# ------------------------------------------------------------------------------------- face data, the owners' layout, corrections
def face_parts(Y, c, a):
    """[rank][4][..., line]: (u'y, w'y) of the bottom face (the rank is the q side, planes 0, 1) and of the top face (the p side,
    planes nl-2, nl-1) from Y[rank][nl][..., line]; zeros where rank 0 has no bottom face and rank R - 1 no top face."""
    R, nl = Y.shape[:2]
    Pt, Pb = face_maps(c, a)
    out = np.zeros((R, 4) + Y.shape[2:], dtype=LD)
    for r in range(R):
        if r > 0:
            out[r, 0], out[r, 1] = Pb[0, 0] * Y[r, 0] + Pb[1, 0] * Y[r, 1], Pb[0, 1] * Y[r, 0] + Pb[1, 1] * Y[r, 1]
        if r < R - 1:
            out[r, 2] = Pt[0, 0] * Y[r, nl - 2] + Pt[1, 0] * Y[r, nl - 1]
            out[r, 3] = Pt[0, 1] * Y[r, nl - 2] + Pt[1, 1] * Y[r, nl - 1]
    return out


def face_rhs(parts):
    """g[2 (R - 1)][..., line]: face i gets the top part of rank i and the bottom part of rank i + 1."""
    R = parts.shape[0]
    return np.concatenate([parts[i, 2:4] + parts[i + 1, 0:2] for i in range(R - 1)])


def face_slots(nu, R):
    """[rank][4][..., line] from nu[2 (R - 1)][..., line]: (nu of the rank's bottom face, nu of its top face), zeros where there is none."""
    out = np.zeros((R, 4) + nu.shape[1:], dtype=nu.dtype)
    for i in range(R - 1):
        out[i, 2:4] = nu[2 * i:2 * i + 2]
        out[i + 1, 0:2] = nu[2 * i:2 * i + 2]
    return out


def to_owners(x, R, flaw=None):
    """One rank's [4][line] in the all-to-all layout [owner][4][Lr], owner = line // Lr."""
    L = x.shape[-1]
    Lr = L // R
    if flaw == "owner":
        return np.stack([x[:, o::R] for o in range(R)])
    return x.reshape(4, R, Lr).transpose(1, 0, 2).copy()


def from_owners(b):
    """Inverse of to_owners: [owner][4][Lr] -> [4][line]."""
    R, _, Lr = b.shape
    return b.transpose(1, 0, 2).reshape(4, R * Lr).copy()


def correct(F, slots, c, a):
    """f - U nu on the four planes next to every face: F[rank][nl][..., line], slots[rank][4][..., line] (face_slots)."""
    R, nl = F.shape[:2]
    Pt, Pb = face_maps(c, a)
    out = F.astype(LD).copy()
    for r in range(R):
        if r > 0:
            out[r, 0] -= Pb[0, 0] * slots[r, 0] + Pb[0, 1] * slots[r, 1]
            out[r, 1] -= Pb[1, 0] * slots[r, 0] + Pb[1, 1] * slots[r, 1]
        if r < R - 1:
            out[r, nl - 2] -= Pt[0, 0] * slots[r, 2] + Pt[0, 1] * slots[r, 3]
            out[r, nl - 1] -= Pt[1, 0] * slots[r, 2] + Pt[1, 1] * slots[r, 3]
    return out


def slab_zsolve(F, c, s, R, a, flaw=None):
    """M^-1 F for F[nz, line] by the steps of the distributed path; returns (x[nz, line], the intermediates)."""
    nz, L = F.shape
    nl = nz // R
    assert nl * R == nz and nl >= 4
    Fr = F.astype(LD).reshape(R, nl, L)
    Y = local_solve(Fr, c, s, a)
    if R == 1:
        return Y.reshape(nz, L), dict(Y=Y)
    parts = face_parts(Y, c, a)
    g = face_rhs(parts)
    D0, E = reduced_blocks(c, s, nl, a, flaw)
    K = assemble_K(D0, E, R)
    nu = solve_lines(K, g[:, None, :])[:, 0, :]
    Fc = correct(Fr, face_slots(nu, R), c, a)
    return local_solve(Fc, c, s, a).reshape(nz, L), dict(Y=Y, parts=parts, g=g, K=K, nu=nu, Fc=Fc)


# --------------------------------------------------------------------------------------- the float64 block-Thomas (the yardstick)
def block_thomas_f64(c, s, nl, a, g):
    """The float64 NumPy block-Thomas of oracle/slab_zsolve.py (its recurrence, its calls) on g[2 (R - 1)][rhs][line], one line at a
    time through oracle.slab_zsolve.reduced_blocks: the yardstick the device's reduced solve is measured with."""
    from oracle import slab_zsolve as osz
    nf, L = g.shape[0] // 2, g.shape[-1]
    out = np.zeros(g.shape)
    for l in range(L):
        D0, E, _, _ = osz.reduced_blocks(float(c[l]), s, nl, a)
        gl = g[:, :, l].reshape(nf, 2, -1)
        Dk, gk = [None] * nf, [None] * nf
        Dk[0], gk[0] = D0, gl[0]
        for i in range(1, nf):
            W = E.T @ np.linalg.inv(Dk[i - 1])
            Dk[i] = D0 - W @ E
            gk[i] = gl[i] - W @ gk[i - 1]
        nu = [None] * nf
        nu[nf - 1] = np.linalg.solve(Dk[nf - 1], gk[nf - 1])
        for i in range(nf - 2, -1, -1):
            nu[i] = np.linalg.solve(Dk[i], gk[i] - E @ nu[i + 1])
        out[:, :, l] = np.concatenate(nu)
    return out


def reduced_errors(K, g, nu):
    """Per line, of nu[n][rhs][line] against the long-double K (worst right-hand side): the forward error
    max|nu - K^-1 g| / max|K^-1 g|; the componentwise backward error max_i |K nu - g|_i / (|K| |nu| + |g|)_i; and the normwise one,
    max|K nu - g| / (|K|_inf max|nu| + max|g|).  The componentwise measure reaches ONE on lines with c far below zero and on
    single-face right-hand sides: there the true E is 1e-20 and smaller, any float64 alternating sum C is rounding noise of relative
    size one, and a row with g_i = 0 has nothing else to be measured against -- on such a case only the other two measures say
    anything."""
    nu = nu.astype(LD)
    ref = solve_lines(K, g.astype(LD))
    fwd = (np.abs(nu - ref).max(axis=0) / np.abs(ref).max(axis=0)).max(axis=0)
    res = np.abs(np.einsum("ijl,jrl->irl", K, nu) - g)
    den = np.einsum("ijl,jrl->irl", np.abs(K), np.abs(nu)) + np.abs(g)
    bwd = np.where(den > 0, res / np.where(den > 0, den, 1), 0).max(axis=0).max(axis=0)
    nden = np.abs(K).sum(axis=1).max(axis=0) * np.abs(nu).max(axis=0) + np.abs(g).max(axis=0)
    nbwd = (res.max(axis=0) / nden).max(axis=0)
    return fwd.astype(float), bwd.astype(float), nbwd.astype(float)


# --------------------------------------------------------------------------------------------------------------------- line sets
def line_set(nx, ny, h, nz, n_grid=None, mismatch=False):
    """lam0[nx], lam1[ny] and c[line] = (1 + lam0[ix]) + lam1[iy] (line = iy nx + ix, float64 as the kernels form it) such that
    the lines cover: -lam_z(k) and -lam_z(k) + 1e-6 for the global lam_z(k) >= -1 (k = 0 gives c = 0: the zero eigenvalue of the
    whole operator), and a grid over [1 - 8a, 1] with both ends.  The longer axis carries the targets, the other one the offsets
    (0, 1e-6, then 2e-6, ... which only shift the targets again).  Where the wanted k outnumber the target slots an evenly spaced
    subset with both ends is taken (returned as `ks`) and the grid keeps at least 5 points.

    The targets ASCEND along their axis, as the eigenvalues of an axis are monotone, and an even number of them is negative.  The
    fused transform kernels run two x-adjacent lines (2j, 2j + 1) as one complex sequence, so a line's rounding error scales with
    the larger member of its pair: eps times the ratio of the two scales, 1e7 between c = 1 - 8a and c = 0 at h = 1/16.  Ascending,
    the members of a pair differ by one grid step (a factor of at most 4 in scale), and the one jump from the last negative grid
    point to c = 0 falls between two pairs.  mismatch = True interleaves the lower with the upper half instead, so that every pair
    holds a far and a near line: the input of the test that pins that property."""
    a = 1.0 / (h * h)
    lamz = -(4.0 * a) * np.sin(np.pi * np.arange(nz) / (2.0 * nz)) ** 2
    all_ks = np.nonzero(lamz >= -1.0)[0]
    n_t, n_o = max(nx, ny), min(nx, ny)
    assert n_o >= 2 and n_t >= 8, (nx, ny)
    n_grid = max(6, n_t - len(all_ks)) if n_grid is None else n_grid
    ks = all_ks
    if len(ks) > n_t - n_grid:
        ks = ks[np.unique(np.round(np.linspace(0, len(ks) - 1, n_t - n_grid)).astype(int))]
    n_grid = n_t - len(ks)
    # an even number of negative targets: a grid of one point less (at least 5) and a filler inside [0, 1] where needed
    fill = next(d for d in range(n_grid - 4) if (np.linspace(1.0 - 8.0 * a, 1.0, n_grid - d) < 0).sum() % 2 == 0)
    grid = np.concatenate([np.linspace(1.0 - 8.0 * a, 1.0, n_grid - fill), 0.5 / (1 + np.arange(fill))])
    targets = np.sort(np.concatenate([-lamz[ks], grid]))
    if mismatch:
        half = n_t // 2
        mixed = np.empty_like(targets)
        mixed[0:2 * half:2], mixed[1:2 * half:2] = targets[:half], targets[n_t - half:]
        if n_t % 2:
            mixed[-1] = targets[half]
        targets = mixed
    offsets = 1e-6 * np.arange(n_o)
    lam_t, lam_o = targets - 1.0, offsets
    lam0, lam1 = (lam_t, lam_o) if nx >= ny else (lam_o, lam_t)
    c = ((1.0 + lam0)[None, :] + lam1[:, None]).reshape(-1)
    return lam0.copy(), lam1.copy(), c, ks
