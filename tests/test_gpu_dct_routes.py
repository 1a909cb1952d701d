"""The Swift-Hohenberg spectral preconditioner Pl^-1 = ((I + Lap)^2 + s)^-1 (bk_precond_sh_create, bk_precond_apply; csrc/dct.hip:
dct_apply, csrc/dct_fast.hip: dct_axis_fused_ok, choose_lt, dct_axis_fft) on every route of its dispatch, at the smallest shape that
reaches each one, against the exact CPU operator oracle.operators.dct_preconditioner (itself pinned to a long-double dense
restatement by tests/test_dct_reference.py).  CASES below is the route table: per case the shape, the pointer layout, the options
and the kernel of every transform pass in launch order,

    F  dct_fused_kernel   -- the only passes option dct_trace prints a line for: their set of (axis, mode) must equal the table's,
                             and their tile count pins the tile height LT (wide tilings 32 / 64 / 128);
    G  dct_fft_kernel     -- the generic LDS FFT kernel (partial tiles, odd n0, misaligned pointers, N < 64, N = 1024, options);
    D  a dense pass       -- dct_axis_direct below N = 32, the guarded fp64-MFMA product from there on;

and ctx.prof_get("dct_pass") counts 2 ndim - 1 passes with the round trip and 2 ndim without it.

Checks: a random vector at shifts 1 and 0 against the oracle, with v and out inside guard bands, out poisoned with NaN, v unchanged,
and the traced application bitwise equal to the untraced one; option and misaligned cases also against the default route of the same
shape; single cosine modes, point sources on the tile and mirror seams, in-place application on one case per route family; the
pointwise entry point bk_precond_op_apply (P.linmap) on its fallbacks.  Every option a test sets is restored in a finally block: the
context is the session's (dct_threads, whose default depends on the shape, is set on a context of the test's own).

Bounds, relative to max|ref| (the project's bounds at shift 1, tests/test_gpu_parity.py): 1e-13 where every pass is an FFT, 1e-12 with a
dense pass.  Shift 0: 7e-12 = 5 x 1.4e-12, the worst error of a correctly rounded float64 dense restatement against long double
over these shapes (test_dct_reference.F64_DENSE_WORST; the scipy oracle itself errs by up to 5.1e-12 there) -- set by (33, 64), where
|Pl^-1| = 7e8; most shapes have |Pl^-1| = 1e5 and a float64 floor of 2.5e-14.  probe() logs every value with a quarter of its bound.
Single modes (shift 1): coefficient by projection and pointwise remainder within 1e-13 (FFT) / 1e-12 (dense) of the coefficient; the
long-double restatement itself leaves 1.1e-14 there, the float64 one 8.9e-15, the scipy oracle 5.8e-14 (test_dct_reference.py).

Measured on an MI355X: the file's 149 instances take 5.9 s.  Worst error per route family (generic / fused / misaligned / options):
random vector at shift 1 1.2e-15 / 1.1e-15 / 1.1e-15 / 1.9e-15 (the last with dct_fft = 0, all passes dense), at shift 0 3.7e-12 at
(33, 64) and 7e-14 .. 6.3e-13 on every other shape -- the oracle's own error there; against the default route of the same shape
at most 2.2e-15; point sources 8.3e-16 at shift 1 and the random vector's figures at shift 0; mode coefficients 1.9e-15; mode
remainders 7.8e-14 with a dense pass (bound 1e-12), 5.1e-14 fused at (128, 64) and 9.0e-14 at (256, 64) with both pointers
misaligned -- the last mode (N0 - 1, N1 - 1), whose coefficient is 4e-5 of the largest, is where the margin to 1e-13 is thin
and where the scipy oracle itself leaves 5.8e-14; the pointwise entry point 1.3e-12 absolute under a bound of 3.0e-10.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import probe
from dct_dense_ref import SHIFTS, box, eigenvalues, mode_tuples, separable_mode
from oracle import operators
from test_dct_reference import F64_DENSE_WORST

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
BAND = 64                           # sentinel doubles on each side of v and out
SENTINEL = -6.02214076e23

# every option of the matrix with its default (csrc/dct.hip, csrc/dct_fast.hip); dct_threads has none that one value restores
DEFAULTS = dict(dct_fused=256, dct_fused_ax0=1, dct_roundtrip=1, dct_lt_wide=1, dct_fastio=1, dct_rt_lanes=256, dct_xcd_map=3,
                dct_fft=1, dct_nt_load=1, dct_nt_store=1, dct_fuse_pw=1, dct_trace=0)
OWN_CONTEXT = ("dct_threads",)

BIG = (64, 256, 256)                # exactly 2^22 points: the non-temporal instantiations; its reference is built once


def _case(dims, routes, layout="al", lt=None, const_len=0, **opts):
    """routes: one letter per pass in launch order -- with the round trip x0 [y0] last2 [y1] x1, without it x0 y0 [z0 z1] y1 x1
    (axis and 0 forward / 1 inverse / 2 round trip); lt: {axis: lines per tile} of fused passes on axis >= 1 where it is not 16."""
    return dict(dims=dims, layout=layout, opts=opts, routes=routes, lt=lt or {}, const_len=const_len)


# ------------------------------------------------------------------------------------------------------------------ the route table
CASES = {
    # --- generic dct_fft_kernel
    "g-4x8x16": _case((4, 8, 16), "GGGGG"),                    # N < 64 on every axis; LT = n0 = 4 on y and z; round trip generic
    "g-16x1024": _case((16, 1024), "GGG"),                     # N = 1024 on y: LT = 8 by the LDS budget
    "g-1024x16": _case((1024, 16), "GGG"),                     # N = 1024 on x: LT = 8, two tiles
    "g-9x64": _case((9, 64), "DGD"),                           # odd n0: pairvec = 0, LT = n0 + 1 = 10 with 9 lines; x direct
    "g-15x64x64": _case((15, 64, 64), "DGGGD"),                # odd n0: a 15-of-16-line tile on y and z; x direct
    "g-33x64": _case((33, 64), "DGD"),                         # three tiles, the last with one line; x guarded MFMA
    "g-24x64": _case((24, 64), "DGD"),                         # even n0, no multiple of 16: pairvec = 1 on a partial tile
    "g-64x8": _case((64, 8), "GGG"),                           # x pass with rows = 8 < 16: LT clipped to 8
    "g-64x3x4": _case((64, 3, 4), "GDGDG"),                    # x pass with rows = 12: LT = 12, no power of two
    "g-64x24": _case((64, 24), "GDDG"),                        # x rows % 16 != 0; dense last axis: no round trip, spectral_scale_kernel
    # --- fused kernel
    "f-64x16": _case((64, 16), "FGF"),                         # one x tile (grid % 8 != 0: no XCD map)
    "f-16x512": _case((16, 512), "GFG"),                       # y round trip, LT = 16
    "f-32x256": _case((32, 256), "GFG", lt={1: 32}),           # LT = 32
    "f-64x128": _case((64, 128), "FFF", lt={1: 64}),           # LT = 64
    "f-128x64": _case((128, 64), "FFF", lt={1: 128}),          # LT = 128
    "f-64x64x64": _case((64, 64, 64), "FFFFF", lt={1: 64, 2: 64}),
    "f-48x128x64": _case((48, 128, 64), "DFFFD"),              # wide tiling declined (48 % 32 != 0): LT = 16; x guarded MFMA
    "f-16x16x512": _case((16, 16, 512), "GGFGG", const_len=512),          # the compile-time-length z round trip
    "f-64x256x256": _case(BIG, "FFFFF", lt={1: 32, 2: 32}),    # non-temporal instantiations
    "f-128x64x64": _case((128, 64, 64), "FFFFF", lt={1: 128, 2: 128}),
    "f-128x512": _case((128, 512), "FFF"),                     # y grid of 8 tiles: the XCD map on a y pass
    "f-256x64": _case((256, 64), "FFF", lt={1: 128}),          # two wide tiles
    # --- v / out 8 bytes off 16-byte alignment: the pass that touches the array is generic, the inner ones stay fused
    "mis-64x64x64-v": _case((64, 64, 64), "GFFFF", "v", lt={1: 64, 2: 64}),
    "mis-64x64x64-o": _case((64, 64, 64), "FFFFG", "o", lt={1: 64, 2: 64}),
    "mis-64x64x64-vo": _case((64, 64, 64), "GFFFG", "vo", lt={1: 64, 2: 64}),
    "mis-256x64-v": _case((256, 64), "GFF", "v", lt={1: 128}),
    "mis-256x64-o": _case((256, 64), "FFG", "o", lt={1: 128}),
    "mis-256x64-vo": _case((256, 64), "GFG", "vo", lt={1: 128}),
    # --- options.  dct_fastio and dct_threads are read for the generic kernel only, so they come with dct_fused = 0; dct_rt_lanes = 512
    # needs (LT / 2) (N / 8) = 512 -- (128, 64, 64), not (64, 64, 64); dct_xcd_map needs grid % 8 == 0 -- (128, 512), not (128, 64)
    "opt-64x64x64-fused0": _case((64, 64, 64), "GGGGG", dct_fused=0),
    "opt-128x64-fused0": _case((128, 64), "GGG", dct_fused=0),
    "opt-64x64x64-ax0": _case((64, 64, 64), "GFFFG", lt={1: 64, 2: 64}, dct_fused_ax0=0),
    "opt-128x64-ax0": _case((128, 64), "GFG", lt={1: 128}, dct_fused_ax0=0),
    "opt-64x64x64-roundtrip0": _case((64, 64, 64), "FFGFFF", lt={1: 64, 2: 64}, dct_roundtrip=0),
    "opt-128x64-roundtrip0": _case((128, 64), "FGFF", lt={1: 128}, dct_roundtrip=0),
    "opt-64x64x64-wide0": _case((64, 64, 64), "FFFFF", dct_lt_wide=0),
    "opt-128x64-wide0": _case((128, 64), "FFF", dct_lt_wide=0),
    "opt-64x64x64-fastio0": _case((64, 64, 64), "GGGGG", dct_fused=0, dct_fastio=0),
    "opt-128x64-fastio0": _case((128, 64), "GGG", dct_fused=0, dct_fastio=0),
    "opt-64x64x64-threads256": _case((64, 64, 64), "GGGGG", dct_fused=0, dct_threads=256),
    "opt-128x64-threads256": _case((128, 64), "GGG", dct_fused=0, dct_threads=256),
    "opt-64x64x64-threads512": _case((64, 64, 64), "GGGGG", dct_fused=0, dct_threads=512),
    "opt-128x64-threads512": _case((128, 64), "GGG", dct_fused=0, dct_threads=512),
    "opt-16x1024-threads256": _case((16, 1024), "GGG", dct_threads=256),            # (default there: 512 lanes)
    "opt-128x64x64-lanes512": _case((128, 64, 64), "FFFFF", lt={1: 128, 2: 128}, dct_rt_lanes=512),
    "opt-128x64-lanes512": _case((128, 64), "FFF", lt={1: 128}, dct_rt_lanes=512),
    "opt-16x512-lanes512": _case((16, 512), "GFG", dct_rt_lanes=512),
    "opt-16x16x512-lanes512": _case((16, 16, 512), "GGFGG", dct_rt_lanes=512),      # (takes the pass off the compile-time length)
    "opt-64x64x64-xcd0": _case((64, 64, 64), "FFFFF", lt={1: 64, 2: 64}, dct_xcd_map=0),
    "opt-128x512-xcd0": _case((128, 512), "FFF", dct_xcd_map=0),
    "opt-64x64x64-fft0": _case((64, 64, 64), "DDDDDD", dct_fft=0),
    "opt-128x64-fft0": _case((128, 64), "DDDD", dct_fft=0),
    "opt-64x256x256-ntload0": _case(BIG, "FFFFF", lt={1: 32, 2: 32}, dct_nt_load=0),
    "opt-64x256x256-ntstore0": _case(BIG, "FFFFF", lt={1: 32, 2: 32}, dct_nt_store=0),
    "opt-64x256x256-nt0": _case(BIG, "FFFFF", lt={1: 32, 2: 32}, dct_nt_load=0, dct_nt_store=0),
}
# options of the pointwise entry point (test_linmap_fallbacks)
LINMAP_OPTIONS = ("dct_fuse_pw",)
# one case per route family for the single-mode, point-source and in-place tests
FAMILIES = ["g-4x8x16", "g-33x64", "g-15x64x64", "g-64x24", "f-128x64", "f-64x64x64", "f-16x16x512", "mis-256x64-vo",
            "opt-64x64x64-fused0", "opt-64x64x64-roundtrip0"]


def option_matrix():
    """Every option key a case or the pointwise test sets (tests/test_dct_coverage_host.py)."""
    return {k for c in CASES.values() for k in c["opts"]} | set(LINMAP_OPTIONS)


def pass_sequence(ndim, n_passes):
    """(axis, mode) of the passes in launch order: mode 0 forward, 1 inverse, 2 round trip (dct_apply)."""
    last = ndim - 1
    if n_passes == 2 * ndim - 1:
        return [(a, 0) for a in range(last)] + [(last, 2)] + [(a, 1) for a in range(last - 1, -1, -1)]
    assert n_passes == 2 * ndim, (ndim, n_passes)
    return [(a, 0) for a in range(ndim)] + [(a, 1) for a in range(last, -1, -1)]


def _expected(case):
    """({(axis, mode): tiles} of the fused passes, number of passes, has a dense pass)"""
    dims, routes = case["dims"], case["routes"]
    n = list(dims) + [1] * (3 - len(dims))
    fused = {}
    for (a, m), r in zip(pass_sequence(len(dims), len(routes)), routes):
        if r == "F":
            lt = 16 if a == 0 else case["lt"].get(a, 16)
            fused[a, m] = (n[1] * n[2]) // lt if a == 0 else (n[0] // lt) * (n[2] if a == 1 else n[1])
    return fused, len(routes), "D" in routes


def _bound(case, shift):
    b1 = 1e-12 if "D" in case["routes"] else 1e-13
    return b1 if shift == 1.0 else max(5 * F64_DENSE_WORST[0.0], b1)


def _hip():
    from bk_amd import hip
    return hip


@contextlib.contextmanager
def _context(ctx, opts):
    """The context the case runs on with its options set: the session's, restored afterwards -- or one of the test's own where an
    option's default cannot be put back."""
    own = any(k in OWN_CONTEXT for k in opts)
    c = _hip().Context(0) if own else ctx
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        yield c
    finally:
        if not own:                 # (a context of the test's own goes with the last plan that refers to it)
            for k, v in DEFAULTS.items():
                c.set_option(k, v)


class _Guarded:
    """n doubles inside an allocation with BAND sentinel doubles on each side, 16-byte aligned or (off) 8 bytes past that."""

    def __init__(self, ctx, n, off, values=None):
        import torch
        self.n, self.lo = n, BAND + int(off)
        self.buf = torch.full((self.lo + n + BAND,), SENTINEL, dtype=torch.float64, device=ctx.torch_device)
        self.t = self.buf[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == 8 * int(off)
        self.t.copy_(torch.from_numpy(values)) if values is not None else self.t.fill_(float("nan"))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def bands_untouched(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == SENTINEL).all())


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _apply(c, P, v, layout, inplace=False):
    """Pl \\ v through bk_precond_apply on guarded buffers (layout: which of v / out is misaligned): the result, after the checks
    that it is finite everywhere, that the bands around v and out are untouched and that v is unchanged."""
    n = v.size
    vin = _Guarded(c, n, "v" in layout, v)
    out = vin if inplace else _Guarded(c, n, "o" in layout)
    c.check(c.lib.bk_precond_apply(P.h, vin.ptr, out.ptr), "bk_precond_apply")
    c.sync()
    got = out.t.cpu().numpy()
    assert np.isfinite(got).all(), "the result is not finite everywhere (poisoned out not overwritten, or a bad read)"
    assert vin.bands_untouched() and out.bands_untouched(), "a store outside the vector"
    assert inplace or _bits_equal(vin.t.cpu().numpy(), v), "the input vector was changed"
    return got


def _plan(c, dims, shift):
    hip = _hip()
    prob = hip.SwiftHohenberg(c, dims, box(dims))
    return prob, hip.DCTPreconditioner(prob, shift)


def _random(dims):
    return np.random.default_rng(1000 * dims[0] + dims[1]).standard_normal(int(np.prod(dims)))


@functools.lru_cache(maxsize=None)
def _oracle(dims, shift):
    return operators.dct_preconditioner(dims, box(dims), shift)


@functools.lru_cache(maxsize=None)
def _random_ref(dims, shift):
    ref = _oracle(dims, shift)(_random(dims))
    ref.setflags(write=False)
    return ref


_default_cache = {}


def _default_route(ctx, dims, shift):
    """The random vector through the default route of the shape (no option set, aligned buffers), once per module."""
    if (dims, shift) not in _default_cache:
        prob, P = _plan(ctx, dims, shift)
        got = _apply(ctx, P, _random(dims), "al")
        got.setflags(write=False)
        _default_cache[dims, shift] = got
    return _default_cache[dims, shift]


def _probe_all(items):
    """probe() every (name, value, bound, info) -- all of them are logged before the first failure is raised."""
    bad = []
    for name, value, bound, info in items:
        try:
            probe(name, value, bound, tight=bound / 4, **info)
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


def parse_trace(err):
    """[(axis, mode, tiles, const_len)] of the dct_trace lines (the line format tests/test_gpu_dct_const_len.py parses)."""
    out = []
    for ln in err.splitlines():
        if ln.startswith("dct_trace axis="):
            f = dict(kv.split("=", 1) for kv in ln.split() if "=" in kv and not kv.startswith("phases"))
            out.append((int(f["axis"]), int(f["mode"]), int(f["tiles"]), int(f["const_len"])))
    return out


# ------------------------------------------------------------------------------------------- a. d. e. f. and the route, per case
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", list(CASES))
def test_route_and_random_vector(ctx, capfd, name, shift):
    """The case's passes are the kernels the table names (trace lines, tile counts, pass count); the random vector agrees with the
    oracle within the bound of the route family and, for an option or a misaligned layout, with the default route of the shape;
    out was poisoned with NaN and comes back finite, the bands around v and out and v itself are untouched; the traced and the
    untraced application give the same bits."""
    case = CASES[name]
    dims, layout = case["dims"], case["layout"]
    fused, n_passes, _ = _expected(case)
    v, ref = _random(dims), _random_ref(dims, shift)
    default = _default_route(ctx, dims, shift) if (case["opts"] or layout != "al") else None
    with _context(ctx, case["opts"]) as c:
        prob, P = _plan(c, dims, shift)
        try:
            capfd.readouterr()
            c.set_option("dct_trace", 1)
            c.prof_enable(True)
            c.prof_reset()
            traced = _apply(c, P, v, layout)
            calls = c.prof_get("dct_pass")["calls"]
        finally:
            c.prof_enable(False)
            c.set_option("dct_trace", 0)
        seen = parse_trace(capfd.readouterr().err)
        got = _apply(c, P, v, layout)
        del P, prob
    assert {(a, m): t for a, m, t, _ in seen} == fused and len(seen) == len(fused), (name, seen, fused)
    assert calls == n_passes, (name, calls, n_passes)
    assert all(cl == (case["const_len"] if (a, m) == (2, 2) else 0) for a, m, _, cl in seen), (name, seen)
    assert _bits_equal(got, traced), (name, np.abs(got - traced).max())
    scale = float(np.abs(ref).max())
    info = dict(case=name, dims=list(dims), shift=shift)
    items = [("dct_route_vs_oracle", np.abs(got - ref).max() / scale, _bound(case, shift), info)]
    if default is not None:
        items.append(("dct_route_vs_default", np.abs(got - default).max() / scale, _bound(case, shift), info))
    _probe_all(items)


# ------------------------------------------------------------------------------------------------------------- b. single modes
@pytest.mark.parametrize("name", FAMILIES)
def test_single_cosine_modes(ctx, name):
    """Input: the separable cosine mode (kx, ky[, kz]); output: that mode divided by (1 + lam_x + lam_y [+ lam_z])^2 + 1.  The first
    and the last mode, the two sides of the even / odd seam N/2 - 1 | N/2 of the Makhoul permutation and low modes that tell the axes
    apart (dct_dense_ref.mode_tuples).  The coefficient recovered by projection and the pointwise remainder are held to 1e-13 (a
    dense pass: 1e-12) of the coefficient; the long-double restatement leaves 1.1e-14 and 4.5e-16 there, a float64 one 8.9e-15
    (tests/test_dct_reference.py).  Shift 1 only: at shift 0 the rounding of the input mode alone leaves 2e-6."""
    case = CASES[name]
    dims, bound = case["dims"], _bound(case, 1.0)
    lam = [eigenvalues(N, l) for N, l in zip(dims, box(dims))]
    items = []
    with _context(ctx, case["opts"]) as c:
        prob, P = _plan(c, dims, 1.0)
        for ks in mode_tuples(dims):
            mode = separable_mode(dims, ks)
            coef = 1.0 / ((1.0 + sum(lm[k] for lm, k in zip(lam, ks))) ** 2 + 1.0)
            g = _apply(c, P, mode, case["layout"])
            info = dict(case=name, dims=list(dims), mode=list(ks))
            items.append(("dct_mode_coefficient", abs(float(g @ mode) - coef) / coef, bound, info))
            items.append(("dct_mode_remainder", float(np.abs(g - coef * mode).max()) / coef, bound, info))
        del P, prob
    _probe_all(items)


# ------------------------------------------------------------------------------------------------------------- c. point sources
def _points(case):
    """Unit impulses: the corners; x on both sides of every line-tile seam LT - 1 | LT of the case and on the last line n0 - 1 (odd
    n0: next to the overhang); N/2 - 1 | N/2 along each axis (the mirror of the Makhoul permutation), the other coordinates mid-way."""
    dims = case["dims"]
    mid = [N // 2 for N in dims]
    pts = [tuple(0 for _ in dims), tuple(N - 1 for N in dims), (dims[0] - 1,) + tuple(0 for _ in dims[1:]),
           (0,) + tuple(N - 1 for N in dims[1:])]
    for lt in sorted({16} | set(case["lt"].values())):
        pts += [(j0,) + tuple(mid[1:]) for j0 in (lt - 1, lt) if j0 < dims[0]]
    pts.append((dims[0] - 1,) + tuple(mid[1:]))
    for a in range(len(dims)):
        pts.append(tuple(mid[b] - 1 if b == a else mid[b] for b in range(len(dims))))
    pts.append(tuple(mid))
    return list(dict.fromkeys(pts))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", FAMILIES)
def test_point_sources_on_the_seams(ctx, name, shift):
    """A unit impulse excites every mode at once and sits on one line of one tile: held to the bound of the random vector."""
    case = CASES[name]
    dims = case["dims"]
    Po = _oracle(dims, shift)
    strides = np.cumprod((1,) + dims[:-1])
    items = []
    with _context(ctx, case["opts"]) as c:
        prob, P = _plan(c, dims, shift)
        for pt in _points(case):
            v = np.zeros(int(np.prod(dims)))
            v[int(np.dot(pt, strides))] = 1.0
            ref = Po(v)
            g = _apply(c, P, v, case["layout"])
            items.append(("dct_point_source", np.abs(g - ref).max() / np.abs(ref).max(), _bound(case, shift),
                          dict(case=name, dims=list(dims), shift=shift, at=list(pt))))
        del P, prob
    _probe_all(items)


# ----------------------------------------------------------------------------------------------------------------- e. in place
@pytest.mark.parametrize("name", ["f-64x64x64", "g-15x64x64", "mis-256x64-vo"])
def test_in_place_application_is_bitwise_the_out_of_place_one(ctx, name):
    """bk_precond_apply(P, w, w): the first pass reads w before anything writes it and the last one writes from the plan's scratch,
    so aliasing is safe on a fused, a generic and a misaligned route -- the same bits as out of place."""
    case = CASES[name]
    v = _random(case["dims"])
    with _context(ctx, case["opts"]) as c:
        prob, P = _plan(c, case["dims"], 1.0)
        layout = "vo" if case["layout"] != "al" else "al"
        out_of_place = _apply(c, P, v, layout)
        in_place = _apply(c, P, v, layout, inplace=True)
        del P, prob
    assert _bits_equal(in_place, out_of_place), (name, np.abs(in_place - out_of_place).max())
    assert np.abs(out_of_place).max() > 0.0


# ------------------------------------------------------------------------------------------------- the pointwise entry point
@pytest.mark.parametrize("variant", ["fuse_pw0", "v_misaligned", "out_misaligned", "u_misaligned"])
@pytest.mark.parametrize("dims", [(64, 64, 64), (256, 64)])
def test_linmap_fallbacks(ctx, dims, variant):
    """a0 v + a1 Pl \\ (J v) through bk_precond_op_apply where apply_pw declines the fused x passes: option dct_fuse_pw = 0, v or out
    8 bytes off alignment (the separate pointwise pass, the plain preconditioner, the axpby), and the state u misaligned (the literal
    stencil chain).  Against (a0 - a1) v + a1 Pl \\ ((g(u) + s) v) built from the oracle as tests/test_gpu_stencil_free.py builds it,
    with that file's bound: the rounding of one stencil evaluation damped by Pl^-1, plus 1e-13 of the result.  The stencil_free
    flag is pw_fused_ok(u, u, u) of ShiftPrecOp::init_fold: it follows the layout of u alone."""
    hip = _hip()
    ls, shift, a0, a1 = box(dims), 1.0, 0.3, 0.9
    n = int(np.prod(dims))
    sh = operators.SwiftHohenberg(dims, ls)
    rng = np.random.default_rng(3)
    u = sh.guess() + 0.3 * rng.standard_normal(n)
    v = rng.standard_normal(n)
    ref = a0 * v + a1 * _oracle(dims, shift)(sh.dF(u, 0.1, 1.2, v))
    floor = 8 * EPS * abs(sh.L1).sum(axis=1).max() * np.abs(v).max() / operators.dct_symbol(dims, ls, shift).min()
    scale = float(np.abs(ref).max())
    with _context(ctx, dict(dct_fuse_pw=0) if variant == "fuse_pw0" else {}) as c:
        prob, P = _plan(c, dims, shift)
        U = _Guarded(c, n, variant == "u_misaligned", u)
        J = prob.jacobian(hip.HipVec(c, U.t), 0.1)
        vin = _Guarded(c, n, variant == "v_misaligned", v)
        out = _Guarded(c, n, variant == "out_misaligned")
        sf = C.c_int(-1)
        c.check(c.lib.bk_precond_op_apply(c.h, P.h, J.h, vin.ptr, a0, a1, out.ptr, C.byref(sf)), "bk_precond_op_apply")
        c.sync()
        got = out.t.cpu().numpy()
        intact = vin.bands_untouched() and out.bands_untouched() and U.bands_untouched()
        same_v = _bits_equal(vin.t.cpu().numpy(), v) and _bits_equal(U.t.cpu().numpy(), u)
        del J, P, prob
    assert np.isfinite(got).all() and intact and same_v, (dims, variant, intact, same_v)
    assert sf.value == (0 if variant == "u_misaligned" else 1), (dims, variant, sf.value)
    probe("dct_linmap", float(np.abs(got - ref).max()), floor + 1e-13 * scale, tight=(floor + 1e-13 * scale) / 4, dims=list(dims),
          variant=variant, floor=float(floor), scale=scale)
