// What the marching kernels of the trapezoid periodic-orbit functional (potrap.hip) and of the monodromy's initial-value system
// (floquet.hip) and of the adjoint (pofold.hip) share: the handle, one slice's stencil load, the chunk rule and the parameter
// check.  The pointwise Jacobian block (cgl_jac) is in cgl_pw.h.
// Internal header.
#pragma once
#include "cgl_pw.h"
#include "common.h"
#include "ops.h"

struct bk_potrap {
    bk_ctx* ctx = nullptr;
    bk_problem* prob = nullptr;
    int M = 0;
    size_t n = 0;                  // grid points per field; a slice holds N = 2 n doubles
    double* phi = nullptr;         // [M N] the normals of the section
    double* xpi = nullptr;         // [M N] its reference point
    double c0 = 0.0;               // <xpi, phi>
    bool has_section = false;
    size_t len() const { return 2 * n * (size_t)M; }
};

namespace bk {

// One slice's values at a grid point: the centre pair and the 5-point Dirichlet Laplacian of both fields (cgl_kernel's lap).
// PK: any kernel-argument struct with nx, ny, ax, ay.
struct PoPoint { double c1, c2, d1, d2; };
template <class PK>
__device__ __forceinline__ PoPoint po_load(const PK& P, const double* s, size_t n, size_t idx, int i, int j) {
    auto lap = [&](const double* f, double c) {
        const double w = i > 0 ? f[idx - 1] : 0.0, e = i + 1 < P.nx ? f[idx + 1] : 0.0;
        const double so = j > 0 ? f[idx - P.nx] : 0.0, nn = j + 1 < P.ny ? f[idx + P.nx] : 0.0;
        return P.ax * ((w + e) - 2.0 * c) + P.ay * ((so + nn) - 2.0 * c);
    };
    PoPoint q;
    q.c1 = s[idx];
    q.c2 = s[idx + n];
    q.d1 = lap(s, q.c1);
    q.d2 = lap(s + n, q.c2);
    return q;
}

constexpr double kPoPivot = 1e-8;      // the project's pivot threshold: a guard, not a tolerance

// potrap.hip
int potrap_chunking(bk_ctx* ctx, size_t n, int M, unsigned* ntiles, int* C, int* nchunks);
int potrap_params(bk_potrap* h, const double* params, int nparams, CglPar* par);

// "who: ..." unless op and pl are an orbit operator and an orbit preconditioner of the same length and the same kind (both
// forward or both adjoint)
int potrap_pair_check(bk_ctx* ctx, const char* who, bk_op* op, bk_precond* pl);

// pofold.hip: the first M N entries and the tail of dG(u, T)^T (w, tau), and the time solve of A0^-T on a spectrum in place
int potrap_adjoint_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* w, double tau, double* out,
                         double* tail);
int potrap_adjoint_timesolve(bk_ctx* ctx, int nx, int ny, int M, double a, double b, double hh, const double* lx, const double* ly,
                             double* spec);

}  // namespace bk
