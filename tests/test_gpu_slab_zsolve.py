"""The slab z-solve of the distributed Swift-Hohenberg preconditioner on ONE GPU: the three face kernels of csrc/dct_slab.hip
(slab_face_gather, slab_reduced_solve, slab_face_correct), the slab half passes of dct_fused_kernel (csrc/dct_fast.hip, DctSlabHalf)
and the two table fill functions of csrc/dct.hip, each against the long-double reference tests/slab_zsolve_ref.py (pinned on the
CPU by tests/test_slab_zsolve_reference.py).  `rank` and `R` are fields of the kernel argument SlabK and the half passes take
DctSlabHalf by pointer, so this process plays every rank of any R <= 16 on tiny arrays and does the two all-to-alls itself by
copying [owner][4][Lr] blocks between the ranks' buffers (tests/slab_abi.py).  No communicator, no second process.

Every output buffer is filled with NaN first and must come back finite everywhere; no line is left out of an assertion, and every
figure is per line, relative to that line's own size.

Lines.  lam0 and lam1 are kernel inputs, so slab_zsolve_ref.line_set crafts them: c = 1 + lam_x + lam_y on a grid over [1 - 8a, 1]
with both ends, and c = -lam_z(k), c = -lam_z(k) + 1e-6 for the global lam_z(k) >= -1 -- the lines where the operator is nearly
singular and the preconditioner matters.  The reduced-solve tests carry every such k; a whole solve whose shape has fewer lines
than that carries an evenly spaced subset with both ends (k = 0 always).  (h, s) runs over slab_zsolve_ref.HS_CASES.  lam_x ascends
along x as an axis' eigenvalues do, because the fused kernels transform x-adjacent lines in pairs and a line's accuracy is relative
to its pair (test_paired_lines_share_one_scale pins exactly that, on pairs chosen 1e7 apart).

Bounds.
* tables: 4 ulp against long-double formulas (lam_loc relative; phi and the twiddles relative to their amplitude).
* gather, correct: every output within 4 eps sum|terms| of the long-double value; absent faces give zeros; planes the correction
  does not own are bitwise untouched.
* reduced solve: forward error of nu and backward error |K nu - g| / (|K| |nu| + |g|) per line against the long-double K, each
  within 8 x max(the same measure of the float64 NumPy block-Thomas over the case, 64 eps).  The backward error is taken in the
  maximum norm.  Read row by row it cannot be asserted: with c far below zero the true coupling block is 1e-20 and smaller, the
  alternating sums C of ANY float64 solve are rounding noise of relative size one, and rows with g_i = 0 then measure noise
  against noise -- the NumPy yardstick itself reaches 1.0 on every nl = 64 case with R >= 3 (slab_zsolve_ref.reduced_errors).
  That figure is recorded with every probe (componentwise, componentwise_numpy).
* whole solve, gather route and split route: per line against the long-double exact inverse, and the two routes against each other,
  within 8 x max(the float64 restatement's per-line error on the case, 256 eps) of the line's max|x|.
The factor 8 covers another summation order at errors of size eps x condition; the NumPy figure is the yardstick, never the device's.

The coupling block E of the capacitance matrix is symmetric for equal slabs (tests/test_slab_zsolve_reference.py), so the E / E'
orientation of the recurrence cannot be observed; the single-face right-hand sides localise every other slip of the recurrence.

Measured on an MI355X (the file's 138 instances take 12 s), worst per (h, s) in the order of HS_CASES, the NumPy yardstick of the
same case family in brackets:
    whole solve, gather route   1.1e-15 (1.0e-15)   1.3e-13 (5.9e-13)   4.1e-11 (7.8e-11)   2.3e-15 (4.8e-15)   5.6e-9 (2.4e-8)
    whole solve, split route    1.4e-15 (1.0e-15)   5.3e-14 (9.4e-14)   8.0e-12 (9.6e-12)   2.1e-15 (2.5e-15)   1.4e-9 (1.6e-9)
    route against route         7.6e-16             9.6e-15             1.2e-13             1.6e-15             9.3e-13
    reduced solve, forward      8.4e-16 (9.9e-16)   1.7e-13 (5.8e-13)   9.8e-11 (2.5e-10)   5.8e-15 (7.0e-15)   4.6e-9 (2.0e-8)
    reduced solve, backward     4.1e-16 (4.4e-16)   1.0e-13 (2.3e-13)   6.3e-12 (1.5e-11)   4.2e-16 (5.0e-16)   1.7e-11 (3.6e-11)
No case is above 1.7 times its own yardstick.  Tables 2.6 ulp, gather 1.3 eps, correct 1.5 eps of sum|terms|.  Paired lines 1e7 apart
in scale: 2.1e-12 and 1.9e-10 of the pair's max|x| at (1/16, 1) and (1/16, 0.05), which is 1.3e-10 and 2.5e-9 of the small line's own.
Before slab_reduced_solve summed A and C with compensation the reduced solve sat at 3 to 5 times the yardstick and the whole solve at
(64, 3, 128, 3), h = 1/16, s = 0.05 at 9 times (5.1e-9 against 5.7e-10), over the bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import slab_zsolve_ref as zr
from conftest import probe
from slab_abi import DctSlabHalf, K_SLAB_MAX_FACES, Launchers, SlabK

pytestmark = pytest.mark.gpu

EPS = zr.EPS
LD = np.longdouble
HS = zr.HS_CASES
HS_IDS = [f"h{h:.4g}-s{s:g}" for h, s in HS]
FACE_PLANES = lambda nl: (0, 1, nl - 2, nl - 1)


# ------------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def fn(ctx):
    return Launchers(ctx.lib)


def _dev(ctx, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(ctx.torch_device)


def _nan(ctx, n):
    import torch
    t = torch.full((int(n),), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    assert t.data_ptr() % 16 == 0
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _host(ctx, t):
    ctx.sync()
    return t.cpu().numpy()


def _written(x, what):
    assert np.isfinite(x).all(), f"{what}: {int((~np.isfinite(x)).sum())} of {x.size} doubles not written (or not finite)"
    return x


class Rig:
    """The device tables of one (shape, h, s): lam0, lam1 crafted by line_set, lam_loc / phi / twiddles from the fill functions."""

    def __init__(self, ctx, fn, nx, ny, nl, R, h, s, mismatch=False):
        self.ctx, self.fn = ctx, fn
        self.nx, self.ny, self.nl, self.R, self.h, self.s = nx, ny, nl, R, h, s
        self.a = 1.0 / (h * h)
        self.L = nx * ny
        assert self.L % R == 0 and nl >= 4
        self.Lr = self.L // R
        lam0, lam1, self.c, self.ks = zr.line_set(nx, ny, h, nl * R, mismatch=mismatch)
        assert lam0.size == nx and lam1.size == ny and self.c.size == self.L
        lam_loc, phi = fn.slab_tables(nl, self.a)
        self.d = {k: _dev(ctx, v) for k, v in dict(lam0=lam0, lam1=lam1, lam_loc=lam_loc, phi=phi, tw=fn.twiddle_table(nl)).items()}

    def K(self, rank, R=None):
        R = self.R if R is None else R
        return SlabK(nx=self.nx, ny=self.ny, nl=self.nl, R=R, rank=rank, L=self.L, Lr=self.L // R, a=self.a, shift=self.s,
                     lam0=self.d["lam0"].data_ptr(), lam1=self.d["lam1"].data_ptr(), lam_loc=self.d["lam_loc"].data_ptr(),
                     phi=self.d["phi"].data_ptr())

    def check(self, st, what):
        self.ctx.check(st, what)

    # -- one launch each; buffers are [nl][L] slabs and [4 L] face buffers
    def axis_pass(self, inverse, fuse, src, dst, half=None):
        assert src.numel() == dst.numel() == self.nl * self.L and src.data_ptr() != dst.data_ptr()
        self.check(self.fn.dct_axis_fft(self.ctx.h, self.nx, self.ny, self.nl, 2, inverse, _ptr(self.d["tw"]), _ptr(src), _ptr(dst),
                                        _ptr(self.d["lam0"]), _ptr(self.d["lam1"]), _ptr(self.d["lam_loc"]), self.s, fuse, None, None,
                                        None, None if half is None else C.byref(half)), "dct_axis_fft")

    def gather(self, rank, y, sbuf):
        assert y.numel() == self.nl * self.L and sbuf.numel() == 4 * self.L
        self.check(self.fn.slab_faces_gather(self.ctx.h, C.byref(self.K(rank)), _ptr(y), _ptr(sbuf)), "slab_faces_gather")

    def solve(self, owner, rbuf, out):
        assert rbuf.numel() == out.numel() == 4 * self.L and self.R - 1 <= K_SLAB_MAX_FACES
        self.check(self.fn.slab_faces_solve(self.ctx.h, C.byref(self.K(owner)), _ptr(rbuf), _ptr(out)), "slab_faces_solve")

    def correct(self, rank, rbuf, f):
        assert f.numel() == self.nl * self.L and rbuf.numel() == 4 * self.L
        self.check(self.fn.slab_faces_correct(self.ctx.h, C.byref(self.K(rank)), _ptr(rbuf), _ptr(f)), "slab_faces_correct")

    def exchange(self, bufs):
        """The all-to-all of the face buffers: rank r's [dst][4][Lr] blocks go to their owners -- bufs[dst] <- [src][4][Lr]."""
        import torch
        v = [b.view(self.R, 4, self.Lr) for b in bufs]
        return [torch.stack([v[src][dst] for src in range(self.R)]).contiguous().view(-1) for dst in range(self.R)]

    def capacitance(self, sbufs):
        """Exchange, the owners' reduced solves, exchange back: the receive buffers of the correction (checked fully written)."""
        outs = []
        for o, rb in enumerate(self.exchange(sbufs)):
            out = _nan(self.ctx, 4 * self.L)
            self.solve(o, rb, out)
            outs.append(out)
        recv = self.exchange(outs)
        for r, t in enumerate(recv):
            _written(_host(self.ctx, t), f"nu for rank {r}")
        return recv

    def whole_gather(self, F):
        """M^-1 F by round trip, gather, solve, correct, round trip; F[nz][L] -> x[nz][L]."""
        R, nl, L = self.R, self.nl, self.L
        f = [_dev(self.ctx, F[r * nl:(r + 1) * nl]).view(-1) for r in range(R)]
        sb = []
        for r in range(R):
            y, s = _nan(self.ctx, nl * L), _nan(self.ctx, 4 * L)
            self.axis_pass(0, 2, f[r], y)
            self.gather(r, y, s)
            sb.append(s)
        for r, t in enumerate(sb):
            _written(_host(self.ctx, t), f"face data of rank {r}")
        recv = self.capacitance(sb)
        xs = []
        for r in range(R):
            self.correct(r, recv[r], f[r])
            x = _nan(self.ctx, nl * L)
            self.axis_pass(0, 2, f[r], x)
            xs.append(_host(self.ctx, x).reshape(nl, L))
        return _written(np.concatenate(xs), "gather route")

    def whole_split(self, F):
        """M^-1 F by forward half, solve, inverse half."""
        R, nl, L = self.R, self.nl, self.L
        assert self.Lr % 2 == 0
        f = [_dev(self.ctx, F[r * nl:(r + 1) * nl]).view(-1) for r in range(R)]
        sb, yh, idle = [], [], _nan(self.ctx, 4 * L)
        for r in range(R):
            y, s = _nan(self.ctx, nl * L), _nan(self.ctx, 4 * L)
            assert self.fn.dct_slab_half_ok(self.ctx.h, self.nx, self.ny, nl, _ptr(f[r]), _ptr(y)), (self.nx, self.ny, nl)
            hf = DctSlabHalf(face_y=s.data_ptr(), face_d=idle.data_ptr(), phi=self.d["phi"].data_ptr(), Lr=self.Lr, a=self.a,
                             has_bottom=r > 0, has_top=r < R - 1)
            self.axis_pass(0, 0, f[r], y, hf)
            sb.append(s)
            yh.append(y)
        for r, t in enumerate(sb):
            _written(_host(self.ctx, t), f"face data of rank {r} (forward half)")
        assert np.isnan(_host(self.ctx, idle)).all()                 # the forward half leaves face_d alone
        recv = self.capacitance(sb)
        xs = []
        for r in range(R):
            x = _nan(self.ctx, nl * L)
            hf = DctSlabHalf(face_y=idle.data_ptr(), face_d=recv[r].data_ptr(), phi=self.d["phi"].data_ptr(), Lr=self.Lr, a=self.a,
                             has_bottom=r > 0, has_top=r < R - 1)
            self.axis_pass(1, 0, yh[r], x, hf)
            xs.append(_host(self.ctx, x).reshape(nl, L))
        assert np.isnan(_host(self.ctx, idle)).all()                 # and the inverse half face_y
        return _written(np.concatenate(xs), "split route")


def _probe_all(items):
    """probe() every (name, value, bound, info): all are logged before the first failure is raised."""
    bad = []
    for name, value, bound, info in items:
        try:
            probe(name, value, bound, tight=bound / 4, **info)
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("h", [1.0, zr.H_BENCH, 0.0625])
@pytest.mark.parametrize("nl", [8, 64, 512])
def test_table_fill_functions(fn, nl, h):
    """dct_twiddle_fill and slab_tables_fill of the library the GPU tests load, against long-double formulas: 4 ulp."""
    from test_slab_zsolve_reference import table_errors
    e_lam, e_phi, e_tw = table_errors(fn, nl, 1.0 / (h * h))
    _probe_all([("slab_table_ulp", e, 4.0, dict(table=t, nl=nl, h=h)) for t, e in (("lam_loc", e_lam), ("phi", e_phi), ("twiddles", e_tw))])


# --------------------------------------------------------------------------------------------------------------- gather, correct
FACE_SHAPES = [(12, 4, 1), (12, 4, 2), (12, 4, 3), (12, 4, 16), (20, 13, 5)]       # (nx, ny, R): L = 48, and L = 260 (two blocks, ragged)


def _face_rig(ctx, fn, shape, h):
    nx, ny, R = shape
    return Rig(ctx, fn, nx, ny, 8, R, h, 1.0)


@pytest.mark.parametrize("h", [1.0, zr.H_BENCH, 0.0625])
@pytest.mark.parametrize("shape", FACE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_face_gather(ctx, fn, shape, h):
    """slab_face_gather of every rank: (u'y, w'y) of its two faces in the owners' layout [line // Lr][4][line % Lr], zeros where
    the rank has no face.  Formulas written out here, the reference's face_parts / to_owners beside them."""
    rig = _face_rig(ctx, fn, shape, h)
    R, nl, L, a = rig.R, rig.nl, rig.L, LD(rig.a)
    Y = np.random.default_rng(11).standard_normal((R, nl, L))
    c = rig.c.astype(LD)
    ca = c - a
    parts = zr.face_parts(Y.astype(LD), rig.c, rig.a)
    worst = 0.0
    for r in range(R):
        y = Y[r].astype(LD)
        want = np.array([-ca * y[0] - a * y[1], -y[0], a * y[nl - 2] + ca * y[nl - 1], y[nl - 1]])
        terms = np.array([np.abs(ca * y[0]) + np.abs(a * y[1]), np.abs(y[0]), np.abs(a * y[nl - 2]) + np.abs(ca * y[nl - 1]),
                          np.abs(y[nl - 1])])
        if r == 0:
            want[0:2], terms[0:2] = 0, 0
        if r == R - 1:
            want[2:4], terms[2:4] = 0, 0
        assert np.array_equal(want, parts[r])
        sbuf = _nan(ctx, 4 * L)
        rig.gather(r, _dev(ctx, Y[r]).view(-1), sbuf)
        got = _written(_host(ctx, sbuf), f"rank {r}").reshape(R, 4, rig.Lr)
        want_o, terms_o = zr.to_owners(want, R), zr.to_owners(terms, R)
        err = np.abs(got - want_o)
        assert (err <= 4 * EPS * terms_o).all(), (shape, h, r, float((err / np.where(terms_o > 0, terms_o, 1)).max() / EPS))
        assert (got[terms_o == 0] == 0.0).all()
        nz = terms_o > 0
        worst = max(worst, float((err[nz] / terms_o[nz]).max() / EPS)) if nz.any() else worst
    probe("slab_gather_eps", worst, 4.0, tight=1.0, shape=list(shape), h=h)


@pytest.mark.parametrize("h", [1.0, zr.H_BENCH, 0.0625])
@pytest.mark.parametrize("shape", FACE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_face_correct(ctx, fn, shape, h):
    """slab_face_correct of every rank: f - U nu on the planes next to its faces from [line // Lr][4][line % Lr]; the slots of an
    absent face hold NaN and must not be read; every other plane keeps its bits."""
    rig = _face_rig(ctx, fn, shape, h)
    R, nl, L, a = rig.R, rig.nl, rig.L, LD(rig.a)
    rng = np.random.default_rng(12)
    F = rng.standard_normal((R, nl, L))
    slots = rng.standard_normal((R, 4, L))
    slots[0, 0:2] = np.nan
    slots[R - 1, 2:4] = np.nan
    ca = rig.c.astype(LD) - a
    ref = zr.correct(F, np.nan_to_num(slots), rig.c, rig.a)      # the reference's correction is the map written out below
    worst = 0.0
    for r in range(R):
        f = _dev(ctx, F[r]).view(-1)
        rig.correct(r, _dev(ctx, zr.to_owners(slots[r], R)).view(-1), f)
        got = _written(_host(ctx, f), f"rank {r}").reshape(nl, L)
        touched = ([0, 1] if r > 0 else []) + ([nl - 2, nl - 1] if r < R - 1 else [])
        keep = [z for z in range(nl) if z not in touched]
        assert np.array_equal(got[keep].view(np.uint64), F[r][keep].view(np.uint64)), (shape, h, r)
        fl, nu = F[r].astype(LD), slots[r].astype(LD)
        want, terms = {}, {}
        if r > 0:
            want[0], terms[0] = fl[0] + (ca * nu[0] + nu[1]), np.abs(fl[0]) + np.abs(ca * nu[0]) + np.abs(nu[1])
            want[1], terms[1] = fl[1] + a * nu[0], np.abs(fl[1]) + np.abs(a * nu[0])
        if r < R - 1:
            want[nl - 2], terms[nl - 2] = fl[nl - 2] - a * nu[2], np.abs(fl[nl - 2]) + np.abs(a * nu[2])
            want[nl - 1], terms[nl - 1] = fl[nl - 1] - (ca * nu[2] + nu[3]), np.abs(fl[nl - 1]) + np.abs(ca * nu[2]) + np.abs(nu[3])
        for z in touched:
            assert np.array_equal(want[z], ref[r, z])
            e = np.abs(got[z] - want[z]) / terms[z]
            assert (e <= 4 * EPS).all(), (shape, h, r, z, float(e.max() / EPS))
            worst = max(worst, float(e.max() / EPS))
        assert np.array_equal(ref[r][keep], F[r][keep].astype(LD))
    probe("slab_correct_eps", worst, 4.0, tight=1.0, shape=list(shape), h=h)


# ----------------------------------------------------------------------------------------------------------------- reduced solve
def _solve_rig(ctx, fn, R, nl, hs, lr_min=0):
    """Lines for every k with lam_z(k) >= -1 (both offsets) and a grid of at least 5: nx targets, a multiple of R; ny = 2 offsets."""
    h, s = hs
    lamz = -(4.0 / (h * h)) * np.sin(np.pi * np.arange(nl * R) / (2.0 * nl * R)) ** 2
    need = max(int((lamz >= -1.0).sum()) + 7, (lr_min * R + 1) // 2)             # (7: a grid of 5 and line_set's parity rule)
    nx = -(-need // R) * R
    rig = Rig(ctx, fn, nx, 2, nl, R, h, s)
    assert len(rig.ks) == int((lamz >= -1.0).sum())
    return rig


def _face_inputs(R, L, rng):
    """Right-hand sides as the ranks' face data [rhs][rank][4][line]: multiples of 2^-20 (top + bottom adds exactly in float64), NaN in
    the slots of absent faces (never read).  One with every face loaded, then one per face of (first, middle, last)."""
    nf = R - 1
    full = np.round(rng.standard_normal((R, 4, L)) * 2.0 ** 20) / 2.0 ** 20
    sets = [full]
    for i in sorted({0, nf // 2, nf - 1}):
        one = np.zeros((R, 4, L))
        one[i, 2:4], one[i + 1, 0:2] = full[i, 2:4], full[i + 1, 0:2]
        sets.append(one)
    out = np.array(sets)
    out[:, 0, 0:2] = np.nan
    out[:, R - 1, 2:4] = np.nan
    return out


def _run_reduced(rig, parts):
    """The owners' solves on one right-hand side: nu[2 (R - 1)][line] after the layout checks of the output [dst][4][Lr]."""
    R, L, Lr, ctx = rig.R, rig.L, rig.Lr, rig.ctx
    sb = [_dev(ctx, zr.to_owners(parts[r], R)).view(-1) for r in range(R)]
    slots = np.empty((R, 4, L))                                   # [dst rank][4][line], collected from the owners
    for o, rb in enumerate(rig.exchange(sb)):
        out = _nan(ctx, 4 * L)
        rig.solve(o, rb, out)
        slots[:, :, o * Lr:(o + 1) * Lr] = _written(_host(ctx, out), f"owner {o}").reshape(R, 4, Lr)
    assert (slots[0, 0:2] == 0.0).all() and (slots[R - 1, 2:4] == 0.0).all(), "unused face slots are not zero"
    for i in range(R - 1):                                        # face i: top of rank i = bottom of rank i + 1
        assert np.array_equal(slots[i, 2:4].view(np.uint64), slots[i + 1, 0:2].view(np.uint64)), i
    return np.concatenate([slots[i, 2:4] for i in range(R - 1)])


def _reduced_case(ctx, fn, R, nl, hs, lr_min=0):
    rig = _solve_rig(ctx, fn, R, nl, hs, lr_min)
    inputs = _face_inputs(R, rig.L, np.random.default_rng(100 * R + nl))
    g = np.stack([zr.face_rhs(np.nan_to_num(p)) for p in inputs], axis=1)                    # [2 nf][rhs][line], exact
    nu = np.stack([_run_reduced(rig, p) for p in inputs], axis=1)
    K = zr.assemble_K(*zr.reduced_blocks(rig.c, rig.s, nl, rig.a), R)
    dev = zr.reduced_errors(K, g.astype(LD), nu)
    yard = zr.reduced_errors(K, g.astype(LD), zr.block_thomas_f64(rig.c, rig.s, nl, rig.a, g))
    info = dict(R=R, nl=nl, h=hs[0], s=hs[1], lines=rig.L, Lr=rig.Lr)
    info.update(componentwise=float(dev[1].max()), componentwise_numpy=float(yard[1].max()))       # recorded, see the docstring
    _probe_all([(f"slab_reduced_{name}", float(e.max()), 8 * max(float(y.max()), 64 * EPS),
                 dict(info, numpy=float(y.max()), line=int(e.argmax()), c=float(rig.c[e.argmax()])))
                for name, e, y in ((("forward", dev[0], yard[0]), ("backward", dev[2], yard[2])))])


@pytest.mark.parametrize("hs", HS, ids=HS_IDS)
@pytest.mark.parametrize("nl", [8, 64])
@pytest.mark.parametrize("R", [2, 3, 5, 8, 16])
def test_reduced_solve(ctx, fn, R, nl, hs):
    """slab_reduced_solve of every owner, on lines for every nearly singular k: A, C, D0, E from the device tables, the block-Thomas
    recurrence at depth R - 1, the [src][4][Lr] input and [dst][4][Lr] output layouts, zeros in the unused slots, both copies of
    every nu bitwise equal."""
    _reduced_case(ctx, fn, R, nl, hs)


def test_reduced_solve_second_block(ctx, fn):
    """Lr = 264: a second, ragged block of 256 lanes in the owners' launch."""
    _reduced_case(ctx, fn, 2, 8, HS[0], lr_min=264)


def test_reduced_solve_refuses_seventeen_ranks(ctx, fn):
    """R - 1 > kSlabMaxFaces: the launcher returns an error before it launches anything (the kernel's register arrays hold 15 block
    rows).  The buffers are sized for R = 17 all the same."""
    R = K_SLAB_MAX_FACES + 2
    rig = Rig(ctx, fn, 17, 2, 8, 1, 1.0, 1.0)                     # 34 lines, Lr = 2 at R = 17
    rbuf, out = _dev(ctx, np.ones(4 * rig.L)), _nan(ctx, 4 * rig.L)
    st = fn.slab_faces_solve(ctx.h, C.byref(rig.K(0, R=R)), _ptr(rbuf), _ptr(out))
    assert st != 0
    with pytest.raises(Exception, match="at most 16"):
        ctx.check(st, "slab_faces_solve")
    assert np.isnan(_host(ctx, out)).all(), "the refused call wrote something"       # (R = 16 itself runs in test_reduced_solve)


# -------------------------------------------------------------------------------------------------------------------- whole solve
# (nx, ny, nl, R).  Gather route only: nl = 8, 16 (the generic transform kernel).  Both routes: the smallest nx that gives each tile
# height LT = 16, 128, 64, 32 at nl = 64, 64, 128, 256, and LT = 16 at nl = 512; ny makes Lr = nx ny / R even.
GATHER_SHAPES = [(48, 2, 8, 16), (12, 4, 16, 3), (16, 5, 16, 5), (12, 2, 8, 2)]
SPLIT_SHAPES = [(16, 8, 64, 16), (128, 2, 64, 2), (64, 3, 128, 3), (32, 2, 256, 2), (16, 2, 512, 2)]


def _inputs(shape):
    """F[input][nz][line]: a random vector, then a unit source on each of the four face planes (0, 1, nl-2, nl-1), each on a slab of
    its own -- ranks 0 .. R - 1 spread over the four."""
    nx, ny, nl, R = shape
    nz, L = nl * R, nx * ny
    F = np.zeros((5, nz, L))
    F[0] = np.random.default_rng(nl + R).standard_normal((nz, L))
    for j, z in enumerate(FACE_PLANES(nl)):
        F[1 + j, ((j * (R - 1)) // 3) * nl + z] = 1.0
    return F


@functools.lru_cache(maxsize=None)
def _whole_reference(shape, hs, mismatch=False):
    """Exact x[input][nz][line] in long double (the rig rebuilds the same line set), its per-line scale, and the yardstick: the worst
    per-line error of the float64 restatement (both forms) over the case's inputs and lines."""
    from oracle import slab_zsolve as osz
    nx, ny, nl, R = shape
    h, s = hs
    a = 1.0 / (h * h)
    _, _, c, _ = zr.line_set(nx, ny, h, nl * R, mismatch=mismatch)
    F = _inputs(shape)
    X = zr.exact_zsolve(np.moveaxis(F, 0, 1), c, s, a)            # [nz][input][line]
    X = np.moveaxis(X, 1, 0)
    scale = np.abs(X).max(axis=1)                                 # [input][line]
    yard = 0.0
    for i in range(F.shape[0]):
        for l in range(c.size):
            for form in (osz.slab_zsolve, osz.slab_zsolve_split):
                yard = max(yard, float(np.abs(form(F[i, :, l], float(c[l]), s, R, a) - X[i, :, l]).max() / scale[i, l]))
    X.setflags(write=False)
    return X, scale, yard


def _whole_case(ctx, fn, shape, hs, split, pair_scale=False):
    nx, ny, nl, R = shape
    rig = Rig(ctx, fn, nx, ny, nl, R, hs[0], hs[1], mismatch=pair_scale)
    X, own, yard = _whole_reference(shape, hs, pair_scale)
    scale = own
    if pair_scale:                                                # the larger of the x-adjacent lines (2j, 2j + 1), see the docstring
        assert nx % 2 == 0
        scale = np.repeat(own.reshape(own.shape[0], -1, 2).max(axis=2), 2, axis=1)
    F = _inputs(shape)
    bound = 8 * max(yard, 256 * EPS)
    info = dict(shape=list(shape), h=hs[0], s=hs[1], restatement=yard, ks=int(len(rig.ks)))
    items = []
    eg = np.zeros(rig.L)
    es, ed = np.zeros(rig.L), np.zeros(rig.L)
    for i in range(F.shape[0]):
        xg = rig.whole_gather(F[i])
        eg = np.maximum(eg, (np.abs(xg - X[i]).max(axis=0) / scale[i]).astype(float))
        if split:
            xs = rig.whole_split(F[i])
            es = np.maximum(es, (np.abs(xs - X[i]).max(axis=0) / scale[i]).astype(float))
            ed = np.maximum(ed, (np.abs(xs - xg).max(axis=0) / scale[i]).astype(float))
    tag = "_pair_scale" if pair_scale else ""
    if pair_scale:                                                # for the record: the same errors against each line's own scale
        info["own_scale_worst"] = float((np.maximum(eg, es) * (scale / own).max(axis=0)).max())
    for name, e in [("slab_whole_gather", eg)] + ([("slab_whole_split", es), ("slab_whole_routes", ed)] if split else []):
        items.append((name + tag, float(e.max()), bound, dict(info, line=int(e.argmax()), c=float(rig.c[e.argmax()]))))
    _probe_all(items)


@pytest.mark.parametrize("hs", HS, ids=HS_IDS)
@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whole_solve_gather_route(ctx, fn, shape, hs):
    """Round trip (dct_axis_fft, fuse_scale 2), gather, the owners' solves, correct, round trip again -- every rank played here, the
    two exchanges done by copying blocks -- against the exact inverse, per line."""
    _whole_case(ctx, fn, shape, hs, split=False)


@pytest.mark.parametrize("hs", HS, ids=HS_IDS)
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whole_solve_both_routes(ctx, fn, shape, hs):
    """Forward half, the owners' solves, inverse half (DctSlabHalf; dct_slab_half_ok asserted) and the gather route on the same
    inputs: each against the exact inverse and the two against each other, per line."""
    _whole_case(ctx, fn, shape, hs, split=True)


@pytest.mark.parametrize("hs", [HS[2], HS[4]], ids=[HS_IDS[2], HS_IDS[4]])
def test_paired_lines_share_one_scale(ctx, fn, hs):
    """The fused transform kernels run the x-adjacent lines (2j, 2j + 1) as the real and imaginary part of ONE complex sequence, so
    what a line keeps of its accuracy is relative to the larger member of its pair.  Here every pair holds a line from the far end
    of the c range and one with c in [0, 1] (line_set(mismatch=True)): scales 1e7 apart at h = 1/16.  Against the PAIR's max|x| both
    routes hold the whole-solve bound; against the small line's own scale they cannot (own_scale_worst records it).  In an
    application lam_x is the smooth, monotone eigenvalue sequence of the x axis, adjacent lines differ by a few per cent in scale, and
    the two readings agree -- which is what the ascending line sets of the other tests reproduce."""
    _whole_case(ctx, fn, (32, 2, 256, 2), hs, split=True, pair_scale=True)
