"""The stencil kernels of ``csrc/stencil.hip`` -- ``sh_gather_kernel``, the eight instantiations of ``sh_stream_kernel``,
``cgl_kernel``, ``sh1d_kernel``, ``dparam_kernel`` -- called launcher by launcher (``tests/stencil_abi.py``) and compared with the
plain host references of ``tests/stencil_ref.py``, path by path of the dispatch in ``sh_apply``.

Two kinds of reference:
* integer data with coefficients that are powers of four (mesh widths 2, 4, 1: 1/h^2 = 1/4, 1/16, 1) and small dyadic parameters:
  every product and every partial sum is a multiple of the finest granularity below 2^53 units (``Ex.exact()`` asserts it), so a
  correct kernel gives the exact value in ANY summation order, fused or not, and the assertions are ``np.array_equal``.  With v in
  [-4096, 4096] the results need more than 24 mantissa bits: an accumulator that became fp32 is caught as well.
* random real data against the np.longdouble evaluation, with the elementwise bound 64 eps (|A| (|A| |v|) + |g v| + |a0 v|) -- the
  constant of test_gpu_parity.py's _stencil_tol, applied pointwise instead of through a global norm.  It guards what integers cannot:
  a coefficient that is only approximately right.

Every device operand sits between NaN guards of G doubles and every output is pre-filled with NaN: a NaN in a result is an over-read
or an unwritten point, a changed guard bit an over-write.  Slabs (zoff, halo_lo / halo_hi, parts 1 and 2 of the halo overlap) run on
ONE GPU here: a global array is cut at given planes and sh_apply is called per slab with halo buffers the test fills itself; unused
halos and, during part 1, all halos are NaN.  The fused Lanczos kernel on slabs needs the context's partial sums all-reduced over
several ranks; it stays with test_distributed.py and is out of scope here.

COVERAGE (checked by test_stencil_coverage_host.py) maps every kernel launch expression of stencil.hip to the tests that reach it.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import stencil_ref as R
from stencil_abi import DPARAM_GRID_CAP, K_PARTIAL_DOUBLES, NT_POINTS, TX, TY, CglArgs, Launchers, Sh1dArgs, ShArgs

pytestmark = pytest.mark.gpu

G = 64                                   # guard doubles before and after every operand
NAN_BITS = 0x7FF8000000000000            # torch.full(nan)
EPS = np.finfo(np.float64).eps
assert np.finfo(np.longdouble).eps < 1e-18, "the longdouble references need a 64-bit mantissa (x86-64)"

# option defaults of the product path (stencil.hip): every test restores them
DEFAULTS = dict(sh_kernel=1, sh_zchunk=0, sh_vload=1, sh_nt=1, sh_stagger=0, jvp_fd_waves=3)

AINV = (0.25, 0.0625, 1.0)               # 1/h^2 for h = 2, 4, 1: 16 A is integral, c0 = 1 - 2 (ax + ay + az) = -13/8 (2-D: 3/8)
L_, NU = 0.25, 0.75                      # parameters
A0, A1, AG = -0.5, 2.0, 0.75             # out = a0 v + a1 (-L1 v) + ag g(u) v ; ag = a1 unless ag_set

COVERAGE = {
    "sh_gather_kernel": ["test_sh_single_domain_exact", "test_sh_slabs_exact", "test_sh_real_data"],
    "sh_stream_kernel<true, true>": ["test_sh_single_domain_exact", "test_sh_alignment", "test_sh_slabs_exact", "test_sh_nontemporal"],
    "sh_stream_kernel<true, false>": ["test_sh_single_domain_exact", "test_sh_alignment", "test_sh_xcd_map_early_return",
                                      "test_sh_stagger_is_bit_identical", "test_sh_slabs_exact", "test_sh_nontemporal",
                                      "test_sh_real_data"],
    "sh_stream_kernel<false, true>": ["test_sh_single_domain_exact"],
    "sh_stream_kernel<false, false>": ["test_sh_single_domain_exact", "test_sh_real_data"],
    "sh_stream_kernel<true, true, true, 3>": ["test_fused_lanczos_step_exact", "test_fused_real_data"],
    "sh_stream_kernel<true, true, true, 2>": ["test_fused_lanczos_step_exact"],
    "sh_stream_kernel<true, false, true, 3>": ["test_fused_lanczos_step_exact", "test_fused_real_data"],
    "sh_stream_kernel<true, false, true, 2>": ["test_fused_lanczos_step_exact"],
    "cgl_kernel": ["test_cgl_exact", "test_cgl_real_data"],
    "sh1d_kernel": ["test_sh1d_exact", "test_sh1d_real_data"],
    "dparam_kernel": ["test_dparam_exact", "test_dparam_real_data"],
}


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def sc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from bk_amd import hip
    c = hip.Context(0)
    yield c, Launchers(c.lib)
    c.close()


@contextlib.contextmanager
def options(c, **kv):
    for k, v in kv.items():
        c.set_option(k, v)
    try:
        yield
    finally:
        for k in kv:
            c.set_option(k, DEFAULTS[k])


class Buf:
    """n device doubles, `off` doubles past a 16-byte boundary, between NaN guards; NaN unless `data` is given."""

    def __init__(self, data=None, n=None, off=0):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float64).ravel()
        self.n, self.off = (data.size if data is not None else int(n)), off
        self.t = torch.full((2 * G + off + self.n,), float("nan"), dtype=torch.float64, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        if data is not None:
            self.body()[:] = torch.from_numpy(data).to("cuda")

    def body(self):
        return self.t[G + self.off:G + self.off + self.n]

    def addr(self, k=0):
        return C.c_void_p(self.t.data_ptr() + 8 * (G + self.off + k))

    @property
    def p(self):
        return self.addr(0)

    def fill_nan(self):
        self.t.fill_(float("nan"))

    def get(self):
        torch.cuda.synchronize()
        return self.body().cpu().numpy()

    def check(self):
        """Both guards still carry the NaN bits of the fill."""
        torch.cuda.synchronize()
        bits = self.t.view(torch.int64)
        assert bool((bits[:G + self.off] == NAN_BITS).all()) and bool((bits[G + self.off + self.n:] == NAN_BITS).all()), \
            "a guard was written"


def ptr(b, k=0):
    return None if b is None else b.addr(k)


def ints(rng, shape, m):
    """Integers in [-m, m], both ends present."""
    a = rng.integers(-m, m + 1, size=shape, dtype=np.int64)
    a.flat[0], a.flat[-1] = m, -m
    return a


def same(got, want, what):
    """Bitwise equality with the exact reference; no NaN (= unwritten point, or a guard / NaN halo that was read)."""
    want = np.asarray(want, dtype=np.float64).ravel()
    assert not np.isnan(got).any(), (what, "NaN at", np.flatnonzero(np.isnan(got))[:8])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {got.size} points differ, first at", bad[:8], got[bad[:4]], want[bad[:4]])


def sh_args(dims, mode, v, u, out, ag=None, ainv=AINV, a0=A0, a1=A1, l=L_, nu=NU, nz=None, zoff=0, halo_lo=None, halo_hi=None,
            part=0):
    """ShArgs of a grid dims = (nx, ny, nzg); nzg = 1: the 2-D problem (az = 0).  v, u, out: addresses (u is NULL in residual mode:
    it must not be read)."""
    nx, ny, nzg = dims
    a = ShArgs(nx=nx, ny=ny, nz=nzg if nz is None else nz, nzg=nzg, zoff=zoff, ax=ainv[0], ay=ainv[1], az=ainv[2] if nzg > 1 else 0.0,
               l=l, nu=nu, a0=a0, a1=a1, mode=mode, v=v, u=u, out=out, halo_lo=halo_lo, halo_hi=halo_hi, part=part)
    if ag is not None:
        a.ag, a.ag_set = ag, True
    return a


def sh_run(sc, a):
    c, L = sc
    c.check(L.sh_apply(c.h, C.byref(a)), "sh_apply")


def sh_ref(dims, mode, v, u, ag=None, ainv=AINV, a0=A0, a1=A1):
    """v, u: arrays (nzg, ny, nx); 2-D when nzg = 1."""
    if dims[2] == 1:
        return R.sh_apply(v[0], u[0], ainv[:2], L_, NU, a0, a1, ag, mode)
    return R.sh_apply(v, u, ainv, L_, NU, a0, a1, ag, mode)


def sh_data(dims, seed=0):
    rng = np.random.default_rng(1000 * seed + dims[0] + 131 * dims[1] + 17161 * dims[2])
    shape = dims[::-1]
    return ints(rng, shape, 4096), ints(rng, shape, 8)


def stream_variants(dims):
    """(sh_zchunk, sh_vload) of the streaming kernel: chunks 1, 2, 3, nz and the planner's own (0) where the grid has that many
    planes; both stagings where the 16-byte one is eligible (full tiles in x, even plane)."""
    nx, ny, nz = dims
    zchunks = [0] if nz == 1 else sorted({z for z in (1, 2, 3, nz) if z <= nz}) + [0]
    vloads = (1, 0) if nx % TX == 0 and (nx * ny) % 2 == 0 else (1,)
    return [(z, vl) for z in zchunks for vl in vloads]


# ------------------------------------------------------------------------------------------------ (a) sh_apply, one domain
# x: 2, 3 (the clamp after reflection), 64, 128 (one / two full tiles), 65 (okx0 true, okx1 false in the last pair), 66 (a two-column
# overhang tile); y: 2, 16, 17, 33; z: 1 (2-D), 2, 3, 4 (the four ghost-plane conditions on gp overlap), 7, 19.  Every value once with
# the other axes trivial (4, 4, 2-D) and once with all axes from the lists.
SH_SHAPES = ([(x, 4, 1) for x in (2, 3, 64, 128, 65, 66)] + [(4, y, 1) for y in (2, 16, 17, 33)] +
             [(4, 4, z) for z in (2, 3, 4, 7, 19)] +
             [(2, 17, 3), (3, 2, 4), (64, 16, 2), (64, 16, 3), (128, 33, 7), (65, 17, 19), (66, 33, 4), (128, 33, 1), (65, 17, 1),
              (66, 2, 1)])


@pytest.mark.parametrize("mode", [0, 1], ids=["jvp", "residual"])
@pytest.mark.parametrize("dims", SH_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_sh_single_domain_exact(sc, dims, mode):
    c, _ = sc
    v, u = sh_data(dims)
    dv, du, out = Buf(v), (Buf(u) if mode == 0 else None), Buf(n=v.size)
    for ag in (None, AG):
        want = sh_ref(dims, mode, v, u, ag).exact()
        a = sh_args(dims, mode, dv.p, ptr(du), out.p, ag)
        for kernel, zchunk, vload in [(0, 0, 1)] + [(1, z, vl) for z, vl in stream_variants(dims)]:
            with options(c, sh_kernel=kernel, sh_zchunk=zchunk, sh_vload=vload):
                out.fill_nan()
                sh_run(sc, a)
                same(out.get(), want, dict(ag=ag, sh_kernel=kernel, sh_zchunk=zchunk, sh_vload=vload))
                out.check()


@pytest.mark.parametrize("which", ["v", "u", "out"])
@pytest.mark.parametrize("dims", [(64, 16, 4), (128, 17, 5)], ids=lambda d: "x".join(map(str, d)))
def test_sh_alignment(sc, dims, which):
    """One operand one double off a 16-byte boundary: out or u -> vec_ok = 0 (scalar loads / stores), v -> vload = 0."""
    c, _ = sc
    v, u = sh_data(dims)
    for mode in (0, 1):
        if mode == 1 and which == "u":
            continue
        want = sh_ref(dims, mode, v, u).exact()
        dv, du, out = Buf(v, off=which == "v"), (Buf(u, off=which == "u") if mode == 0 else None), Buf(n=v.size, off=which == "out")
        assert getattr(dict(v=dv, u=du, out=out)[which].p, "value") % 16 == 8
        for zchunk in (0, 2):
            with options(c, sh_zchunk=zchunk):
                out.fill_nan()
                sh_run(sc, sh_args(dims, mode, dv.p, ptr(du), out.p))
                same(out.get(), want, dict(mode=mode, sh_zchunk=zchunk))
                out.check()


@pytest.mark.parametrize("mode", [0, 1], ids=["jvp", "residual"])
def test_sh_xcd_map_early_return(sc, mode):
    """3 x 3 tiles x 5 chunks = 45 workgroups in a grid of 48: more than 8 and no multiple of 8, so the XCD-aware block -> tile map
    leaves three workgroups without a tile (the early return) and every tile must still be taken exactly once."""
    c, _ = sc
    dims = (130, 40, 9)
    assert (-(-dims[0] // TX)) * (-(-dims[1] // TY)) * 5 == 45
    v, u = sh_data(dims)
    dv, du, out = Buf(v), (Buf(u) if mode == 0 else None), Buf(n=v.size)
    with options(c, sh_zchunk=2):
        sh_run(sc, sh_args(dims, mode, dv.p, ptr(du), out.p))
    same(out.get(), sh_ref(dims, mode, v, u).exact(), "xcd map")
    out.check()


def test_sh_stagger_is_bit_identical(sc):
    """sh_stagger delays the workgroups of each CU's second and third slot; with more workgroups than CUs some are delayed.  The
    values must not change."""
    c, _ = sc
    dims = (65, 17, 80)                                        # 2 x 2 tiles x 80 one-plane chunks = 320 workgroups
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus % 8 == 0 and 320 > cus, cus                     # (stencil.hip applies the option on such devices only)
    v, u = sh_data(dims)
    dv, du, out = Buf(v), Buf(u), Buf(n=v.size)
    want = sh_ref(dims, 0, v, u).exact()
    got = {}
    for st in (0, 2):
        with options(c, sh_zchunk=1, sh_stagger=st):
            out.fill_nan()
            sh_run(sc, sh_args(dims, 0, dv.p, du.p, out.p))
            got[st] = out.get()
            out.check()
    assert np.array_equal(got[0].view(np.int64), got[2].view(np.int64))
    same(got[2], want, "sh_stagger = 2")


@pytest.mark.parametrize("mode", [0, 1], ids=["jvp", "residual"])
def test_sh_nontemporal(sc, mode):
    """The only large case: from 2^22 points on the u loads and the output stores carry the non-temporal hint (option sh_nt)."""
    c, _ = sc
    dims = (256, 128, 128)
    assert dims[0] * dims[1] * dims[2] >= NT_POINTS
    v, u = sh_data(dims)
    want = sh_ref(dims, mode, v, u).exact()
    dv, du, out = Buf(v), (Buf(u) if mode == 0 else None), Buf(n=v.size)
    for nt, vload in ((1, 1), (0, 1), (1, 0)):
        with options(c, sh_nt=nt, sh_vload=vload):
            out.fill_nan()
            sh_run(sc, sh_args(dims, mode, dv.p, ptr(du), out.p))
            same(out.get(), want, dict(sh_nt=nt, sh_vload=vload))
            out.check()


# ------------------------------------------------------------------------------------------------ (b) slabs on one GPU
def run_slabs(sc, dims, cuts, mode, v, dv, du, out, nanhalo, split, halo_off=0):
    """sh_apply per slab of the global array.  halo_lo / halo_hi: separate buffers with the two planes below / above the slab; the
    first slab's lower and the last slab's upper halo are NaN (never to be read).  split: part 1 with BOTH halos NaN -- a chunk of
    part 1 that reads a halo plane poisons its output -- then part 2 with the halos in place; a point written by neither stays NaN."""
    nx, ny, nzg = dims
    plane = nx * ny
    zoff = 0
    for nz in cuts:
        lo = Buf(v[zoff - 2:zoff], off=halo_off) if zoff > 0 else nanhalo
        hi = Buf(v[zoff + nz:zoff + nz + 2], off=halo_off) if zoff + nz < nzg else nanhalo
        kw = dict(nz=nz, zoff=zoff)
        at = (dv.addr(zoff * plane), ptr(du, zoff * plane), out.addr(zoff * plane))
        if split:
            sh_run(sc, sh_args(dims, mode, *at, halo_lo=nanhalo.p, halo_hi=nanhalo.p, part=1, **kw))
            sh_run(sc, sh_args(dims, mode, *at, halo_lo=lo.p, halo_hi=hi.p, part=2, **kw))
        else:
            sh_run(sc, sh_args(dims, mode, *at, halo_lo=lo.p, halo_hi=hi.p, **kw))
        torch.cuda.synchronize()                               # lo / hi are released at the end of this iteration
        zoff += nz
    assert zoff == nzg


@pytest.mark.parametrize("mode", [0, 1], ids=["jvp", "residual"])
@pytest.mark.parametrize("nzg,cuts", [(7, (2, 3, 2)), (19, (8, 3, 8)), (19, (10, 9))], ids=["2+3+2", "8+3+8", "10+9"])
@pytest.mark.parametrize("nx,ny", [(64, 16), (66, 17)], ids=["64x16", "66x17"])
def test_sh_slabs_exact(sc, nx, ny, nzg, cuts, mode):
    """The concatenated slab outputs equal the global reference: zoff, the halo planes, parts 1 and 2 of the halo overlap with
    tail == 1, tail == 2 (a last chunk of one plane), inner <= 0 and zchunk == 1 (where everything moves to part 2)."""
    c, _ = sc
    dims = (nx, ny, nzg)
    v, u = sh_data(dims, seed=len(cuts))
    want = sh_ref(dims, mode, v, u).exact()
    dv, du, out = Buf(v), (Buf(u) if mode == 0 else None), Buf(n=v.size)
    nanhalo = Buf(n=2 * nx * ny)
    runs = [(0, 0, False, 0)] + [(1, z, split, 0) for z in (1, 2, 3, 0) for split in (False, True)] + [(1, 0, False, 1), (1, 2, True, 1)]
    for kernel, zchunk, split, halo_off in runs:
        with options(c, sh_kernel=kernel, sh_zchunk=zchunk):
            out.fill_nan()
            run_slabs(sc, dims, cuts, mode, v, dv, du, out, nanhalo, split, halo_off)
            same(out.get(), want, dict(sh_kernel=kernel, sh_zchunk=zchunk, split=split, halo_off=halo_off))
            out.check()
    assert bool(torch.isnan(nanhalo.t).all())


# ------------------------------------------------------------------------------------------------ (c) the fused Lanczos step
def fused_problem(c, dims):
    """The problem object whose mesh widths are 2, 4, 1: ls = (nx, 2 ny, nz / 2) gives 1/h^2 = (1/4, 1/16, 1) exactly."""
    from bk_amd import hip
    nx, ny, nz = dims
    return hip.SwiftHohenberg(c, dims, (float(nx), 2.0 * ny, nz / 2.0), l=L_, nu=NU)


def fused_call(sc, prob, dv, du, a0, a1, cc, dr, out):
    c, L = sc
    params = (C.c_double * 2)(L_, NU)
    dot, fused = C.c_double(float("nan")), C.c_int(-1)
    c.check(L.jvp_axpy_dot(prob.h, dv.p, du.p, params, a0, a1, cc, ptr(dr), out.p, C.byref(dot), C.byref(fused)), "jvp_axpy_dot")
    return dot.value, fused.value


@pytest.mark.parametrize("rcase", ["r_c", "r_c0", "r_null"])
@pytest.mark.parametrize("dims,zchunks", [((64, 16, 4), [0]), ((128, 32, 9), [0]), ((66, 17, 7), [1, 2, 3, 7, 0]), ((64, 16, 2), [0])],
                         ids=["64x16x4", "128x32x9", "66x17x7", "64x16x2"])
def test_fused_lanczos_step_exact(sc, dims, zchunks, rcase):
    """out = a0 v + a1 J v + c r and v . out from sh_stream_kernel<true, VL, true, WPE> through bk_problem::jvp_axpy_dot, bit for bit:
    first-plane addends, the ring slot of a chunk's last plane, the flush loop (q = 0 and 1), tile overhang in the dot."""
    from bk_amd import hip
    c, _ = sc
    assert dims[0] * dims[1] * dims[2] < 2 ** 17
    rng = np.random.default_rng(dims[0] + dims[2])
    shape = dims[::-1]
    v, u, r = ints(rng, shape, 64), ints(rng, shape, 8), ints(rng, shape, 64)
    prob = fused_problem(c, dims)
    # precondition: the problem's own 1/h^2 are (1/4, 1/16, 1) -- one plain JVP against the reference
    Jv = prob.jacobian(hip.HipVec.from_numpy(c, u.ravel()), L_)(hip.HipVec.from_numpy(c, v.ravel())).numpy()
    same(Jv, R.sh_apply(v, u, AINV, L_, NU, 0.0, 1.0, None, 0).exact(), "plain JVP of the problem object")
    cc = {"r_c": 0.25, "r_c0": 0.0, "r_null": 0.25}[rcase]
    ref_out, ref_dot = R.sh_fused(v, u, r if rcase == "r_c" else None, AINV, L_, NU, A0, A1, cc)
    want, want_dot = ref_out.exact(), float(ref_dot.exact())
    dv, du, dr, out = Buf(v), Buf(u), (None if rcase == "r_null" else Buf(r)), Buf(n=v.size)
    vloads = (1, 0) if dims[0] % TX == 0 else (1,)
    for zchunk in zchunks:
        for waves in (3, 2):
            for vload in vloads:
                what = dict(sh_zchunk=zchunk, jvp_fd_waves=waves, sh_vload=vload)
                with options(c, **what):
                    out.fill_nan()
                    dot, fused = fused_call(sc, prob, dv, du, A0, A1, cc, dr, out)
                    assert fused == 1, what
                    same(out.get(), want, what)
                    assert dot == want_dot, (what, dot, want_dot)
                    out.check()


def test_fused_misaligned_addend_is_refused(sc):
    """sh_fused_dot_ok: an addend that is not 16-byte aligned is not supported; jvp_axpy_dot then reports fused = 0 and has done
    nothing (its caller runs the separate passes)."""
    c, L = sc
    dims = (64, 16, 4)
    rng = np.random.default_rng(5)
    v, u, r = (ints(rng, dims[::-1], m) for m in (64, 8, 64))
    dv, du, out = Buf(v), Buf(u), Buf(n=v.size)
    prob = fused_problem(c, dims)
    for off, ok in ((1, False), (0, True)):
        dr = Buf(r, off=off)
        a = sh_args(dims, 0, dv.p, du.p, out.p)
        a.addv, a.addc = dr.p, 0.25
        assert L.sh_fused_dot_ok(c.h, C.byref(a)) is ok
        out.fill_nan()
        dot, fused = fused_call(sc, prob, dv, du, A0, A1, 0.25, dr, out)
        assert fused == int(ok)
        if ok:
            ref_out, ref_dot = R.sh_fused(v, u, r, AINV, L_, NU, A0, A1, 0.25)
            same(out.get(), ref_out.exact(), "aligned addend")
            assert dot == float(ref_dot.exact())
        else:
            assert np.isnan(out.get()).all() and np.isnan(dot)             # untouched
        out.check()
    # ... and the other conditions it states: 2-D, the residual mode, parts of the halo overlap, more tiles than partial sums
    assert not L.sh_fused_dot_ok(c.h, C.byref(sh_args((64, 16, 1), 0, dv.p, du.p, out.p)))
    assert not L.sh_fused_dot_ok(c.h, C.byref(sh_args(dims, 1, dv.p, None, out.p)))
    assert not L.sh_fused_dot_ok(c.h, C.byref(sh_args(dims, 0, dv.p, du.p, out.p, part=2)))
    big = (TX * 300, TY * 300, 4)
    with options(c, sh_zchunk=4):
        assert L.sh_fused_dot_ok(c.h, C.byref(sh_args((TX * 256, TY * 288, 4), 0, dv.p, du.p, out.p)))      # = kPartialDoubles tiles
    with options(c, sh_zchunk=4):
        assert 300 * 300 > K_PARTIAL_DOUBLES and not L.sh_fused_dot_ok(c.h, C.byref(sh_args(big, 0, dv.p, du.p, out.p)))


# ------------------------------------------------------------------------------------------------ (d) cGL
CGL_P = dict(r=0.5, mu=0.25, nu=1.0, c3=-1.0, c5=0.75, gamma=0.25)
CGL_AINV = (0.25, 1.0)


def cgl_run(sc, dims, mode, dv, du, out, ainv=CGL_AINV, a0=A0, a1=A1):
    c, L = sc
    a = CglArgs(nx=dims[0], ny=dims[1], ax=ainv[0], ay=ainv[1], a0=a0, a1=a1, mode=mode, v=dv.p, u=ptr(du), out=out.p, **CGL_P)
    c.check(L.cgl_apply(c.h, C.byref(a)), "cgl_apply")


@pytest.mark.parametrize("dims", [(2, 2), (3, 2), (16, 16), (17, 15), (41, 21)], ids=lambda d: "x".join(map(str, d)))
def test_cgl_exact(sc, dims):
    rng = np.random.default_rng(dims[0])
    shape = (2, dims[1], dims[0])
    v, u = ints(rng, shape, 4096), ints(rng, shape, 4)
    p = tuple(CGL_P.values())
    du, out = Buf(u), Buf(n=v.size)
    got = {}
    for mode in (0, 1, 2):
        x = u if mode == 1 else v                              # the residual is evaluated at the state itself
        dv = du if mode == 1 else Buf(v)
        out.fill_nan()
        cgl_run(sc, dims, mode, dv, None if mode == 1 else du, out)
        got[mode] = out.get()
        same(got[mode], R.cgl_apply(x, u, CGL_AINV, *p, A0, A1, mode).exact(), dict(mode=mode))
        out.check()
    assert not np.array_equal(got[0], got[2])                  # the adjoint differs on this data: mode 2 cannot pass as mode 0


# ------------------------------------------------------------------------------------------------ (e) SH 1-D
@pytest.mark.parametrize("mode", [0, 1], ids=["jvp", "residual"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 255, 256, 257, 513])
def test_sh1d_exact(sc, n, mode):
    c, L = sc
    rng = np.random.default_rng(n)
    v, u = (ints(rng, n, 4096), ints(rng, n, 8)) if mode == 0 else (ints(rng, n, 128), None)      # u^5 of the residual: |u| <= 128
    dv, du, out = Buf(v), (Buf(u) if mode == 0 else None), Buf(n=n)
    a = Sh1dArgs(nx=n, ax=0.25, lam=-0.25, nu=0.75, a0=A0, a1=A1, mode=mode, v=dv.p, u=ptr(du), out=out.p)
    c.check(L.sh1d_apply(c.h, C.byref(a)), "sh1d_apply")
    e = R.sh1d_apply(v, u, 0.25, -0.25, 0.75, A0, A1, mode)
    same(out.get(), e.exact(), "sh1d")
    assert e.bits > 24
    out.check()


# ------------------------------------------------------------------------------------------------ (f) dF/dparam
@pytest.mark.parametrize("n", [1, 257, 2 ** 20 + 257])
@pytest.mark.parametrize("pde,ipar", R.DPARAM_CASES)
def test_dparam_exact(sc, pde, ipar, n):
    """n = 2^20 + 257: 4097 blocks' worth of points on the capped grid of 4096 -- the grid-stride loop takes a second turn."""
    c, L = sc
    assert 2 ** 20 + 257 > 256 * DPARAM_GRID_CAP
    rng = np.random.default_rng(pde * 10 + ipar)
    u = ints(rng, (2, n) if pde == R.PDE_CGL2D else n, 64)
    du, out = Buf(u), Buf(n=u.size)
    c.check(L.pde_dparam(c.h, pde, ipar, n, 0.5, du.p, out.p), "pde_dparam")
    same(out.get(), R.dparam(pde, ipar, 0.5, u).exact(), "dparam")
    out.check()


# ------------------------------------------------------------------------------------------------ (g) real data, one per family
def close(got, ref, bound, what):
    """|got - ref| <= bound elementwise, ref in longdouble."""
    assert not np.isnan(got).any(), what
    err = np.abs(got.astype(np.longdouble) - np.asarray(ref).ravel())
    bad = np.flatnonzero(err > np.asarray(bound).ravel())
    assert bad.size == 0, (what, bad[:8], err[bad[:4]], np.asarray(bound).ravel()[bad[:4]])


REAL_AINV = (0.7, 1.3, 2.1)


@pytest.mark.parametrize("dims", [(66, 17, 7), (128, 16, 5), (65, 17, 1)], ids=lambda d: "x".join(map(str, d)))
def test_sh_real_data(sc, dims):
    """Bound 64 eps (|A| (|A| |v|) + |g v| + |a0 v|) elementwise (a1 = 1, ag = a1): every evaluation of the 25-point stencil and the
    pointwise terms sums at most 40 products of the terms this adds up in absolute value."""
    c, _ = sc
    rng = np.random.default_rng(dims[0])
    shape = dims[::-1]
    v, u = rng.standard_normal(shape), rng.standard_normal(shape)
    ld = lambda a: a.astype(np.longdouble)
    ainv = REAL_AINV if dims[2] > 1 else REAL_AINV[:2]
    sq = (lambda a: a[0]) if dims[2] == 1 else (lambda a: a)
    out = Buf(n=v.size)
    for mode in (0, 1):
        ref = R.sh_apply(ld(sq(v)), ld(sq(u)), tuple(np.longdouble(a) for a in ainv), 0.1, 1.2, A0, 1.0, None, mode)
        bound = 64 * EPS * R.sh_abs(sq(v), sq(u), ainv, 0.1, 1.2, A0, 1.0, None, mode)
        dv, du = Buf(v), (Buf(u) if mode == 0 else None)
        a = sh_args(dims, mode, dv.p, ptr(du), out.p, ainv=REAL_AINV, a0=A0, a1=1.0, l=0.1, nu=1.2)
        for kernel, zchunk in ((0, 0), (1, 0), (1, 3)):
            with options(c, sh_kernel=kernel, sh_zchunk=zchunk):
                out.fill_nan()
                sh_run(sc, a)
                close(out.get(), ref, bound, dict(mode=mode, sh_kernel=kernel, sh_zchunk=zchunk))
                out.check()


@pytest.mark.parametrize("dims", [(64, 16, 4), (66, 17, 7)], ids=lambda d: "x".join(map(str, d)))
def test_fused_real_data(sc, dims):
    """out as in test_sh_real_data plus |c r|.  The dot: sum |v| * (the bound of out) for the errors of out, plus the summation
    itself -- one fma per point of a thread's column (4 nz), 6 + 2 levels in the workgroup, the second stage over the tiles: fewer
    than 64 roundings of u = eps / 2 each on partial sums below sum |v out|."""
    from bk_amd import hip
    c, _ = sc
    rng = np.random.default_rng(dims[1])
    shape = dims[::-1]
    v, u, r = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    ls = (np.pi, 2.0, 1.3)
    prob = hip.SwiftHohenberg(c, dims, ls, l=0.1, nu=1.2)
    ainv = tuple(1.0 / (2.0 * l / n) ** 2 for n, l in zip(dims, ls))         # problem.hip: h = 2 l / n, ainv = 1 / (h * h)
    ld = lambda a: a.astype(np.longdouble)
    ref = R.sh_apply(ld(v), ld(u), tuple(np.longdouble(a) for a in ainv), 0.1, 1.2, A0, 1.0, None, 0) + np.longdouble(0.3) * ld(r)
    absout = R.sh_abs(v, u, ainv, 0.1, 1.2, A0, 1.0, None, 0) + 0.3 * np.abs(r)
    ref_dot = (ld(v) * ref).sum()
    dv, du, dr, out = Buf(v), Buf(u), Buf(r), Buf(n=v.size)
    params = (C.c_double * 2)(0.1, 1.2)
    for zchunk in (0, 3):
        with options(c, sh_zchunk=zchunk):
            out.fill_nan()
            dot, fused = C.c_double(), C.c_int()
            c.check(sc[1].jvp_axpy_dot(prob.h, dv.p, du.p, params, A0, 1.0, 0.3, dr.p, out.p, C.byref(dot), C.byref(fused)), "jvp_axpy_dot")
            assert fused.value == 1
            close(out.get(), ref, 64 * EPS * absout, dict(sh_zchunk=zchunk))
            assert abs(dot.value - ref_dot) <= 64 * EPS * (np.abs(v) * absout).sum() + 32 * EPS * np.abs(v * np.asarray(ref, dtype=np.float64)).sum()
            out.check()


def test_cgl_real_data(sc):
    dims = (17, 15)
    rng = np.random.default_rng(3)
    v, u = rng.standard_normal((2, 15, 17)), rng.standard_normal((2, 15, 17))
    p = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.3)
    ainv = (1.7, 0.9)
    c, L = sc
    du, out = Buf(u), Buf(n=v.size)
    for mode in (0, 1, 2):
        x = u if mode == 1 else v
        dv = du if mode == 1 else Buf(v)
        a = CglArgs(nx=17, ny=15, ax=ainv[0], ay=ainv[1], a0=A0, a1=A1, mode=mode, v=dv.p, u=du.p, out=out.p, **p)
        out.fill_nan()
        c.check(L.cgl_apply(c.h, C.byref(a)), "cgl_apply")
        ref = R.cgl_apply(x.astype(np.longdouble), u.astype(np.longdouble), tuple(np.longdouble(t) for t in ainv), *p.values(), A0, A1, mode)
        close(out.get(), ref, 64 * EPS * R.cgl_abs(x, u, ainv, *p.values(), A0, A1, mode), dict(mode=mode))
        out.check()


def test_sh1d_real_data(sc):
    c, L = sc
    n = 257
    rng = np.random.default_rng(4)
    v, u = rng.standard_normal(n), rng.standard_normal(n)
    ax = (n / 12.0) ** 2
    out = Buf(n=n)
    for mode in (0, 1):
        dv, du = Buf(v), Buf(u)
        a = Sh1dArgs(nx=n, ax=ax, lam=-0.1, nu=2.0, a0=A0, a1=A1, mode=mode, v=dv.p, u=du.p, out=out.p)
        out.fill_nan()
        c.check(L.sh1d_apply(c.h, C.byref(a)), "sh1d_apply")
        ref = R.sh1d_apply(v.astype(np.longdouble), u.astype(np.longdouble), np.longdouble(ax), -0.1, 2.0, A0, A1, mode)
        close(out.get(), ref, 64 * EPS * R.sh1d_abs(v, u, ax, -0.1, 2.0, A0, A1, mode), dict(mode=mode))
        out.check()


@pytest.mark.parametrize("pde,ipar", R.DPARAM_CASES)
def test_dparam_real_data(sc, pde, ipar):
    """c * a product of at most five factors of one sum of two squares: fewer than 8 roundings, relative to the value itself."""
    c, L = sc
    n = 257
    rng = np.random.default_rng(pde * 10 + ipar)
    u = rng.standard_normal((2, n) if pde == R.PDE_CGL2D else n)
    du, out = Buf(u), Buf(n=u.size)
    c.check(L.pde_dparam(c.h, pde, ipar, n, 0.3, du.p, out.p), "pde_dparam")
    ref = R.dparam(pde, ipar, np.longdouble(0.3), u.astype(np.longdouble))
    close(out.get(), ref, 8 * EPS * np.abs(np.asarray(ref, dtype=np.float64)), "dparam")
    out.check()
