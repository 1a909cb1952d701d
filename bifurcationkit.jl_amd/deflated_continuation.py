"""Deflated continuation, ``continuation(prob, DefCont(...), contParams)`` of src/DeflatedContinuation.jl (Farrell, Beentjes,
Birkisson, "The computation of disconnected bifurcation diagrams", arXiv:1603.00809): the reference's only route to branches that
are NOT connected to the one it starts from, as examples/SH2d-fronts.jl:168-181 runs it on Swift-Hohenberg with Pl = lu(L1 + I).

  DefCont                  the algorithm's parameters (:14-33)
  uniform_perturbation     the example's ``perturb_solution = x .+ 0.1 .* rand(length(x))`` on the device (bk_vec_perturb): a
                           counter-based uniform of the global index, restated exactly by tests/defcont_ref.py
  deflated_continuation    deflatedContinuation (:251-356): ``native=True`` runs every Newton as one library call
                           (bk_newton_deflated_exact along the branches, bk_defcont_seek for new ones), ``native=False`` the same
                           kernels call by call (hip.newton_deflated, DeflationOperator.dist)

Every parameter step: empty the operator; continue each active branch by deflated Newton from its previous state at the new
parameter with the solutions found so far in this step deflated (updatebranch!, :100-153; a failure deactivates the branch); then,
every ``seek_every_step`` steps and while fewer than ``max_branches`` branches are active, from each old active branch repeat
perturb -> deflated Newton -> acceptance tests -> accept_solution -> push until a seek fails (:323-351).

Out of scope: eigenvalues, stability and bifurcation detection on the branches (the example runs with detect_bifurcation = 0);
the tangent of getpredictor! (the Newton guess is the previous state, so nothing reads it); plotting; a Julia binding (in Julia
the reference's own DefCont already runs on the plugin surface); more than one rank (the reductions are all-reduced and the
perturbation is indexed globally, but nothing here is exercised on ranks).

Two deliberate differences from the reference, both in the bookkeeping of the first point.  The reference builds every initial
state with ``iterate(contIt)`` from ``roots[1]`` (:162-163), i.e. all initial branches start from the FIRST root; here branch i
starts from root i (with one root, the example's case, the two agree).  And that ``iterate`` records a Newton-corrected point at
the initial parameter; here the roots are taken as given and a branch's first record is its first continued point -- for a branch
found by a seek, the solution the seek returned (its Newton counts are the seek's).
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib as L
from . import continuation as Cn
from . import hip
from .hip import HipVec, _ptr

_MASK = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z: int) -> int:
    """The finaliser of bk_vec_perturb's hash on a Python int."""
    z &= _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def derive_seed(seed: int, branch: int, count: int) -> int:
    """The seed of one perturbation from (seed, branch id, call count): two rounds of the same finaliser."""
    return _mix64(_mix64(seed + (branch + 1) * _GOLDEN) + (count + 1) * _GOLDEN)


def _perturb_solution(x, p, id):
    return x


def _accept_solution(x, p):
    return True


def _update_deflation_op(defop, x, p):
    defop.push(x)


class UniformPerturbation:
    """``x .+ amp .* rand(length(x))`` (examples/SH2d-fronts.jl:181) in place on the device: x[i] += amp U(s, index0 + i) with the
    counter-based uniform of bk_vec_perturb, ``s = derive_seed(seed, branch id, number of calls so far)`` and ``index0`` the
    global index of the rank's first element (z-slab start x plane size) of the problem it is bound to.  The noise therefore does
    not depend on the launch or the rank decomposition, and a NumPy uint64 restatement reproduces it bit for bit."""

    def __init__(self, amp: float, seed: int):
        self.amp, self.seed, self.count, self.index0 = float(amp), int(seed), 0, 0

    def bind(self, prob):
        """Called by the driver: fresh call count, ``index0`` from the problem's slab."""
        plane = int(np.prod(prob.dims[:-1])) * prob.nfields if len(prob.dims) > 1 else prob.nfields
        self.index0, self.count = int(prob.slab[0]) * plane, 0
        return self

    def __call__(self, x: HipVec, p, id):
        s = derive_seed(self.seed, int(id), self.count)
        self.count += 1
        ctx = x.ctx
        ctx.check(ctx.lib.bk_vec_perturb(ctx.h, x.n, _ptr(x.t), self.amp, s, self.index0), "bk_vec_perturb")
        return x


def uniform_perturbation(amp: float, seed: int) -> UniformPerturbation:
    return UniformPerturbation(amp, seed)


@dataclass
class DefCont:
    """DefCont (src/DeflatedContinuation.jl:14-33).  ``alg`` (the predictor) and ``jacobian`` have one value here -- the previous
    state as the guess, and the one-solve step of DeflatedProblemCustomLS with the exact dM (bk_newton_deflated_exact).

    ``stop_plain``: stop the Newton iterations on |F| < tol instead of the reference's |M F| = |M| |F| < tol.  On the device
    |M| |F| stalls where |F| meets its rounding floor (M ~ 1e4 with a few roots 0.2 - 0.4 away; bk_newton_deflated_exact), and
    whether that lies under tol is not a property of the state.  With alpha >= 1 every factor of M is >= 1, so |M F| < tol implies
    |F| < tol: the plain rule accepts everything the reference's rule accepts.  Default (None): the plain rule when
    ``deflation_operator.alpha >= 1``, the reference's otherwise."""
    deflation_operator: object = None
    max_branches: int = 100
    seek_every_step: int = 1
    max_iter_defop: int = 5
    perturb_solution: object = _perturb_solution
    accept_solution: object = _accept_solution
    update_deflation_op: object = _update_deflation_op
    stop_plain: bool | None = None


@dataclass
class DCBranch:
    """One branch: a record per continued point, the saved states (``cp.save_sol_every_step``; the first point always; the last
    state of a branch that was lost, marked ``lost=True``, :150), and whether it is still followed."""
    param: list = field(default_factory=list)
    normu: list = field(default_factory=list)
    itnewton: list = field(default_factory=list)
    itlinear: list = field(default_factory=list)
    step: list = field(default_factory=list)
    sol: list = field(default_factory=list)
    active: bool = True


@dataclass
class DCResult:
    """DCResult (:60-71): the branches, the states of the active ones, the algorithm; ``seeks`` logs every seek (step, branch,
    reason: 0 accepted, 1 not converged, 2 plain residual, 3 known root, 4 refused by accept_solution; Newton and linear
    counts) and ``timing`` the wall time spent in the branch updates and in the seeks."""
    branches: list
    sol: list
    alg: DefCont
    seeks: list = field(default_factory=list)
    timing: dict = field(default_factory=dict)

    def __len__(self):
        return len(self.branches)

    def __getitem__(self, k):
        return self.branches[k]


class _State:                                   # DCState (:87-93)
    def __init__(self, x, active=True):
        self.x, self.active, self.step = x, active, 0


def _seek_native(prob, defop, x, p, ls, tol, max_iterations, norm_inf, stop_plain, cap=L.BK_MAX_NEWTON_ITER + 1):
    """bk_defcont_seek on the already perturbed guess ``x`` (updated in place)."""
    ctx = prob.ctx
    pv = prob._pvec(p)
    arr = (C.c_double * len(pv))(*pv)
    lo = ls._opts()
    m = len(defop)
    rp = (C.c_void_p * max(m, 1))(*[r.t.data_ptr() for r in defop.roots])
    hist = (C.c_double * cap)()
    res = L.DefContSeekResult()
    ctx.check(ctx.lib.bk_defcont_seek(ctx.h, prob.h, _ptr(x.t), arr, len(pv), rp, m, float(defop.power), float(defop.alpha),
                                      1 if defop.accumulator == "mean" else 0, 1 if stop_plain else 0, 1 if norm_inf else 0,
                                      float(tol), int(max_iterations), C.byref(lo), ls._pl(), hist, cap, C.byref(res)),
              "bk_defcont_seek")
    return dict(u=x, converged=bool(res.converged), itnewton=res.itnewton, itlineartot=res.itlinear, accepted=bool(res.accepted),
                reason=res.reason, M=res.M, min_dist=res.min_dist, plain_residual=res.plain_residual,
                min_dist_normC=res.min_dist_normC, itnewton_total=res.itnewton_total,
                residuals=[hist[i] for i in range(min(cap, res.itnewton_total))])


def _seek_mirror(prob, defop, x, p, ls, tol, max_iterations, norm_inf, stop_plain):
    """The same call by call: hip.newton_deflated, the plain residual, one pass of DeflationOperator.dist."""
    s = hip.newton_deflated(prob, defop, x, p, ls, tol=tol, max_iterations=max_iterations, norm_inf=norm_inf, stop_plain=stop_plain)
    u = s["u"]
    fx = prob.residual(u, p)
    plain = fx.norminf() if norm_inf else fx.norm()
    d2, dinf = defop.dist(u)
    dmin = math.inf
    for a, b in zip(d2, dinf):
        di = b if norm_inf else math.sqrt(a)
        dmin = di if (di != di or di < dmin) else dmin
        if di != di:
            break
    reason = 1 if not s["converged"] else 2 if not plain < tol else 3 if not dmin >= tol else 0
    s.update(accepted=reason == 0, reason=reason, plain_residual=plain, min_dist_normC=dmin, itnewton_total=s["itnewton"] + 1)
    return s


def seek(prob, defop, x, p, ls, tol=1e-12, max_iterations=125, norm_inf=False, stop_plain=True, native=True, **kw):
    """_DC_get_new_solution (:269-286) from the already perturbed guess ``x``: dict(u, converged, itnewton, itlineartot, accepted,
    reason, plain_residual, min_dist_normC, M, min_dist, residuals, itnewton_total).  ``native`` updates ``x`` in place."""
    if native:
        return _seek_native(prob, defop, x, p, ls, tol, max_iterations, norm_inf, stop_plain, **kw)
    return _seek_mirror(prob, defop, x, p, ls, tol, max_iterations, norm_inf, stop_plain)


def deflated_continuation(prob, alg: DefCont, cp: Cn.ContinuationPar, normC=Cn.norm2, native=True, verbosity=0) -> DCResult:
    """deflatedContinuation (src/DeflatedContinuation.jl:251-356) from the roots of ``alg.deflation_operator`` at the problem's
    parameter; ``cp.ds`` is the (signed) parameter step, ``cp.newton_options`` the Newton parameters and the linear solver."""
    if normC not in (Cn.norm2, Cn.norminf):
        raise ValueError("deflated_continuation: normC is Cn.norm2 or Cn.norminf (the two norms the device passes form)")
    norm_inf = normC is Cn.norminf
    defop0 = alg.deflation_operator
    if defop0 is None or len(defop0) == 0:
        raise ValueError("You must provide at least one guess")                                       # :226-228
    if not defop0.autodiff:
        raise ValueError("deflated_continuation: DeflationOperator(..., autodiff=True) (the exact derivative) is required")
    nopt = cp.newton_options
    ls, tol = nopt.linsolver, nopt.tol
    stop_plain = (defop0.alpha >= 1) if alg.stop_plain is None else bool(alg.stop_plain)
    max_iter_seek = alg.max_iter_defop * nopt.max_iterations                                         # :223
    defop = replace(defop0, roots=list(defop0.roots))                                                 # copy(defOp), :231
    if hasattr(alg.perturb_solution, "bind"):
        alg.perturb_solution.bind(prob)
    newton = hip.newton_deflated_native if native else hip.newton_deflated
    states = [_State(r.copy()) for r in defop.roots]                                                  # :157-167
    branches = [DCBranch() for _ in states]
    result = DCResult(branches, [], alg, timing=dict(update=0.0, seek=0.0))
    p = float(prob.params[prob.lens])

    def record(br, st, u, s, first=False):
        st.step += 1
        br.param.append(p)
        br.normu.append(normC(u))
        br.itnewton.append(s["itnewton"])
        br.itlinear.append(s["itlineartot"])
        br.step.append(st.step)
        if first or Cn.mod_counter(st.step, cp.save_sol_every_step):
            br.sol.append(dict(x=u.copy(), p=p, step=st.step))

    nstep = 0
    while ((cp.p_min < p < cp.p_max) or nstep == 0) and nstep < cp.max_steps:                         # :289-290
        p = min(max(p + cp.ds, cp.p_min), cp.p_max)                                                   # clamp_predp, :292
        if verbosity > 0:
            print(f"step = {nstep} has {sum(s.active for s in states)}/{len(branches)} active branch(es), p = {p}")
        defop.roots.clear()                                                                           # :299
        t0 = time.perf_counter()
        for idb, st in enumerate(states):                                                             # updatebranch!, :100-153
            if not st.active:
                continue
            s = newton(prob, defop, st.x, p, ls, tol=tol, max_iterations=nopt.max_iterations, norm_inf=norm_inf,
                       stop_plain=stop_plain)
            if s["converged"]:
                st.x = s["u"]
                alg.update_deflation_op(defop, st.x, p)
                record(branches[idb], st, st.x, s, first=not branches[idb].param)
            else:
                st.active = branches[idb].active = False
                branches[idb].sol.append(dict(x=st.x.copy(), p=branches[idb].param[-1] if branches[idb].param else None,
                                              step=st.step, lost=True))
                if verbosity > 0:
                    print(f"  branch {idb} lost after {s['itnewton']} iterations")
        t1 = time.perf_counter()
        result.timing["update"] += t1 - t0
        nbrs = len(states)
        nactive = sum(s.active for s in states)
        if nstep % alg.seek_every_step == 0 and nactive < alg.max_branches:                           # :323
            n_active = 0
            for idb in range(nbrs):
                st = states[idb]
                if not (st.active and n_active < alg.max_branches):
                    continue
                n_active += 1
                success = True
                while success:
                    x = alg.perturb_solution(st.x.copy(), p, idb)                                     # :270-272
                    s = seek(prob, defop, x, p, ls, tol=tol, max_iterations=max_iter_seek, norm_inf=norm_inf,
                             stop_plain=stop_plain, native=native)
                    success, reason = s["accepted"], s["reason"]
                    if success and not any(r is st.x for r in defop.roots):                          # :334, when update_deflation_op kept st.x out
                        d2, dinf = replace(defop, roots=[st.x]).dist(s["u"])
                        if (dinf[0] if norm_inf else math.sqrt(d2[0])) < tol:
                            success, reason = False, 3
                    accepted = success and bool(alg.accept_solution(s["u"], p))                       # :338
                    result.seeks.append(dict(step=nstep, branch=idb, reason=reason if (accepted or not success) else 4,
                                             itnewton=s["itnewton"], itlinear=s["itlineartot"], new_branch=len(states) if accepted else None))
                    if accepted:
                        defop.roots.append(s["u"])                                                    # :340
                        states.append(_State(s["u"], n_active + 1 < alg.max_branches))                # :344
                        branches.append(DCBranch(active=states[-1].active))
                        record(branches[-1], states[-1], s["u"], s, first=True)
                        if verbosity > 0:
                            print(f"  new solution from branch {idb}: branch {len(states) - 1}, {s['itnewton']} iterations")
        result.timing["seek"] += time.perf_counter() - t1
        nstep += 1
    result.sol = [s.x for s in states if s.active]                                                    # :355
    return result
