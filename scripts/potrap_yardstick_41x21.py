#!/usr/bin/env python
"""The yardstick of the 41 x 21, M = 30 Newton case of tests/test_gpu_potrap.py (YARD_41x21), on the CPU: the
restatement's Newton from the one-mode Hopf guess at r = r_hopf - 0.01 with sparse LU of the assembled Jacobian against the same
with preconditioned SciPy GMRES (rtol 1e-9), and the difference of the two converged orbits and T entries.  The sparse LU of the
51 661-unknown Jacobian takes minutes, which is why no test of the suite runs it.  Prints one JSON line.

Usage: python scripts/potrap_yardstick_41x21.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import potrap_ref as R  # noqa: E402
import test_potrap_reference as T  # noqa: E402


def main():
    dims, M, dr = (41, 21), 30, 0.01
    m = R.Model(dims, T.LS)
    r = T._rstar(m) - dr
    pars = dict(T.PARS, r=r)
    pars_of = lambda p: dict(pars, r=p)
    U0, T0 = T._hopf_guess(m, M, dr)
    phi, xpi = R.section_from_guess(m, U0, pars)
    t0 = time.time()
    lu = R.newton(m, U0, T0, r, pars_of, phi, xpi, R.lu_solver(m, pars_of), tol=1e-10, max_iterations=12)
    t1 = time.time()
    gm = R.newton(m, U0, T0, r, pars_of, phi, xpi, R.gmres_solver(m, pars_of, r, T.PARS["nu"], T0, 1e-9), tol=1e-10, max_iterations=12)
    t2 = time.time()
    assert lu["converged"] and gm["converged"]
    print(json.dumps(dict(dims=dims, M=M, dr=dr, orbit=float(np.abs(lu["U"] - gm["U"]).max()), T=abs(lu["T"] - gm["T"]),
                          newton_lu=len(lu["residuals"]) - 1, gmres_counts=gm["itlinear"], amplitude=float(np.abs(lu["U"]).max()),
                          seconds_lu=t1 - t0, seconds_gmres=t2 - t1)))


if __name__ == "__main__":
    main()
