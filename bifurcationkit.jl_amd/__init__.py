"""bifurcationkit.jl_amd -- MI355X-native Newton-Krylov corrector for BifurcationKit.jl's PALC continuation.

Only what the hot path needs:
  csrc/      hand-written HIP (gfx950) kernels + the C ABI (include/bkhip.h) -> lib/libbkhip.so
  _lib.py    ctypes binding of the C ABI (the Python twin of julia/BifurcationKitHIP.jl)
  hip.py     mirror of the reference's plugin surface (linear / bordered / eigen solvers, problems)
  continuation.py   minimal restatement of the caller (newton, newton_palc, PALC loop) for parity tests
  codim2.py  fold and Hopf points: minimally augmented refinement (newton_fold, newton_hopf) and codim-2 curve continuation
  normal_form1d.py  normal form at simple branch points and folds of Swift-Hohenberg, predictors, automatic branch switching
  deflated_continuation.py  deflated continuation (DefCont): disconnected branches of Swift-Hohenberg by deflated Newton from noise
  periodic_orbit.py  periodic orbits of cGL by the trapezoid rule: functional, preconditioned Newton from the Hopf predictor, PALC
  shooting.py  periodic orbits of cGL by standard shooting on a spectral ETDRK2 flow: flow, functional, Newton, PALC, Floquet multipliers

Import name: ``bk_amd`` (the directory name is not a valid Python identifier; ``bk_amd.py`` at the repo
root registers this package under that name).
"""
from . import _lib  # noqa: F401

__all__ = ["_lib", "hip", "continuation", "codim2", "normal_form1d", "deflated_continuation", "periodic_orbit", "shooting"]
