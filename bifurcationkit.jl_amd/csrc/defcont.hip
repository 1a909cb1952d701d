// Deflated continuation: continuation(prob, DefCont(...), contParams) (src/DeflatedContinuation.jl:196-356), the reference's route
// to branches that are not connected to the one it starts from (examples/SH2d-fronts.jl:168-181).  The loop over steps and
// branches is host logic (deflated_continuation.py); here are the three things it needs on the device:
//
//   DeflDist<K>     reads u and K roots (1 + K streams), writes nothing: d2_i = sum (u - r_i)^2 and dinf_i = max |u - r_i|, the
//                   normC(u - root) of the acceptance tests (:282, :334) for normC = norm and normC = norminf in ONE pass.  The
//                   sums are those of DeflDots<K, D> (deflate.hip) -- same items per lane, same element order, same two stages --
//                   so d2_i is the d_i the Newton iteration itself saw, bit for bit.  The max propagates NaN (vecops.hip: max_nan).
//   perturb         x_i <- x_i + amp U(seed, index0 + i), the perturb_solution of the example (x .+ 0.1 .* rand(length(x)), :181)
//                   with a COUNTER-BASED uniform: U depends on (seed, global index) alone, so the result does not depend on the
//                   grid, the load path or the rank decomposition, and NumPy's uint64 restates it exactly.
//   bk_defcont_seek _DC_get_new_solution (:269-286) and the duplicate test of :334: the deflated Newton of deflate.hip
//                   (defl_newton) with an open iteration count, then the three acceptance tests.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "deflate.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// max that propagates NaN, as norminf does (vecops.hip: max_nan)
__device__ __forceinline__ double max_prop(double a, double b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ double wave_max_prop(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max_prop(v, __shfl_down(v, off, 64));
    return v;
}

template <int KK>
struct DeflDist {
    static constexpr int K = KK, NIN = 1 + K, NV = 2 * K, U = defl_unroll(K), FIELDS = 1;
    static_assert(NV <= kPartialVals, "partial values per workgroup");
    const double* in[NIN];          // u, r_0 .. r_{K-1}
};

// partials[block][2 K]: K sums (the epilogue of block_sum_store: wave sums, then (0 + 1) + (2 + 3)), then K maxima
template <class Pass, int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) defl_dist_kernel(size_t n, Pass pass, double* __restrict__ partials) {
    constexpr int K = Pass::K;
    double s[K], m[K];
#pragma unroll
    for (int i = 0; i < K; ++i) { s[i] = 0.0; m[i] = 0.0; }
    stream_visit<Pass::U, VEC, NTH, 1>(n, pass.in, [&](auto kc, size_t, const auto& x) {
#pragma unroll
        for (int e = 0; e < decltype(kc)::value; ++e)
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const double t = x[e][0] - x[e][1 + i];
                s[i] += t * t;
                m[i] = max_prop(m[i], fabs(t));
            }
    });
    __shared__ double sm[2 * K][4];
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double t = wave_sum(s[i]), q = wave_max_prop(m[i]);
        if (lane == 0) { sm[i][wv_] = t; sm[K + i][wv_] = q; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * K) {
        const int k = threadIdx.x;
        partials[(size_t)blockIdx.x * (2 * K) + k] = k < K ? (sm[k][0] + sm[k][1]) + (sm[k][2] + sm[k][3])
                                                           : max_prop(max_prop(sm[k][0], sm[k][1]), max_prop(sm[k][2], sm[k][3]));
    }
}

// out[2 k] = (d2 | dinf) of the k <= 8 roots.  The load path and the grid are those of stream_reduce for DeflDots<K, 0>; the second
// stage runs once as a sum and once as a max over the same partials (each reads its own half of the result).
int dist_chunk(bk_ctx* ctx, size_t n, const double* u, const double* const* roots, int k, double* out) {
    return count_dispatch<1, kDeflRoots>(k, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        using Pass = DeflDist<K>;
        Pass pass{};
        pass.in[0] = u;
        for (int i = 0; i < K; ++i) pass.in[1 + i] = roots[i];
        const StreamPlan pl = stream_plan<Pass>(ctx, n, all_aligned16(pass.in, n, 1), kRedBlocks);
        {
            ProfScope ps(ctx, "deflation_dist", 8.0 * n * Pass::NIN);
            load_path_dispatch(pl.vec, pl.nth, [&](auto V, auto NT) {
                hipLaunchKernelGGL((defl_dist_kernel<Pass, decltype(V)::value, decltype(NT)::value>), dim3(pl.grid), dim3(kThreads), 0,
                                   ctx->stream, n, pass, ctx->d_partials);
            });
            BK_HIP(ctx, hipGetLastError());
        }
        BK_TRY(reduce_finish(ctx, pl.grid, 2 * K, 0));
        for (int i = 0; i < K; ++i) out[i] = ctx->h_red[i];
        BK_TRY(reduce_finish(ctx, pl.grid, 2 * K, 1));
        for (int i = 0; i < K; ++i) out[K + i] = ctx->h_red[K + i];
        return 0;
    });
}

int v_deflation_dist(bk_ctx* ctx, size_t n, const double* u, const double* const* roots, int nroots, double* d2, double* dinf) {
    for (int c = 0; c < nroots; c += kDeflRoots) {
        const int k = nroots - c < kDeflRoots ? nroots - c : kDeflRoots;
        double out[2 * kDeflRoots];
        BK_TRY(dist_chunk(ctx, n, u, roots + c, k, out));
        for (int i = 0; i < k; ++i) {
            d2[c + i] = out[i];
            dinf[c + i] = out[k + i];
        }
    }
    return 0;
}

// U(seed, g) in [0, 1): splitmix64's finaliser on seed + (g + 1) golden, the top 53 bits (exact in fp64)
__device__ __forceinline__ double hash_u01(unsigned long long seed, unsigned long long g) {
    unsigned long long z = seed + (g + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// x + amp U with the product and the sum rounded one after the other (the file is built without contraction; the pragma says
// so where it matters)
__device__ __forceinline__ double perturbed(double x, double amp, unsigned long long seed, unsigned long long g) {
#pragma clang fp contract(off)
    const double t = amp * hash_u01(seed, g);
    return x + t;
}

__device__ __forceinline__ void st2_nt(double* p, size_t i, double a, double b) {
    nt_d2 r; r.x = a; r.y = b;
    __builtin_nontemporal_store(r, reinterpret_cast<nt_d2*>(p) + i);
}

// in place: every lane loads the items of an iteration, then stores them -- no lane reads what another one writes
template <int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) perturb_kernel(size_t n, double* x, double amp, unsigned long long seed,
                                                           unsigned long long index0) {
    const double* const in[1] = {x};
    stream_visit<4, VEC, NTH, 1>(n, in, [&](auto kc, size_t i, const auto& v) {
        if constexpr (decltype(kc)::value == 2) {
            const double a = perturbed(v[0][0], amp, seed, index0 + 2 * i), b = perturbed(v[1][0], amp, seed, index0 + 2 * i + 1);
            if (NTH) st2_nt(x, i, a, b);
            else st2(x, i, a, b);
        } else {
            x[i] = perturbed(v[0][0], amp, seed, index0 + i);
        }
    });
}

int v_perturb(bk_ctx* ctx, size_t n, double* x, double amp, unsigned long long seed, unsigned long long index0) {
    if (n == 0) return 0;
    ProfScope ps(ctx, "vec_perturb", 16.0 * n);
    const bool vec = aligned16(x);
    const int grid = grid_for(n, vec ? 2 : 1, 4096);          // the launch shape of the in-place axpby (vecops.hip: v_axpbyz)
    load_path_dispatch(vec, vec && nt_hint(ctx, n), [&](auto V, auto NT) {
        hipLaunchKernelGGL((perturb_kernel<decltype(V)::value, decltype(NT)::value>), dim3(grid), dim3(kThreads), 0, ctx->stream, n, x,
                           amp, seed, index0);
    });
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_deflation_dist(bk_ctx* ctx, size_t n, const double* u, const double* const* roots, int nroots, double* d2, double* dinf) {
    if (!ctx || !u || nroots < 0 || (nroots > 0 && (!roots || !d2 || !dinf))) return -1;
    for (int i = 0; i < nroots; ++i)
        if (!roots[i]) return -1;
    return v_deflation_dist(ctx, n, u, roots, nroots, d2, dinf);
}

int bk_vec_perturb(bk_ctx* ctx, size_t n, double* x, double amp, unsigned long long seed, unsigned long long index0) {
    if (!ctx || (n > 0 && !x)) return -1;
    return v_perturb(ctx, n, x, amp, seed, index0);
}

int bk_defcont_seek(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams, const double* const* roots,
                    int nroots, double power, double alpha, int accumulator_mean, int stop_plain, int norm_inf, double tol,
                    int max_iterations, const bk_gmres_opts* lsopts, bk_precond* pl, double* residuals, int residuals_cap,
                    bk_defcont_seek_result* res) {
    if (!ctx || !prob || !x || !params || !lsopts || !res || !residuals || nroots < 0 || (nroots > 0 && !roots)) return -1;
    if (residuals_cap < 1) return set_error(ctx, "bk_defcont_seek: residuals_cap < 1");
    if (max_iterations < 0) return set_error(ctx, "bk_defcont_seek: max_iterations < 0");
    for (int i = 0; i < nroots; ++i) {
        if (!roots[i]) return -1;
        if (roots[i] == x) return set_error(ctx, "bk_defcont_seek: x aliases root %d (the iterate is updated in place)", i);
    }
    DeflNewton o;
    BK_TRY(defl_newton(ctx, prob, x, params, nparams, roots, nroots, power, alpha, accumulator_mean, stop_plain, norm_inf, tol,
                       max_iterations, lsopts, pl, residuals, residuals_cap, &o));
    // the ring in time order: entry k sits at k % cap, the oldest kept one is entry total - cap
    const int total = o.itnewton + 1;
    if (total > residuals_cap) std::rotate(residuals, residuals + total % residuals_cap, residuals + residuals_cap);
    // normC(x - root_i) of :282 (the roots) and :334 (the state sought from, which the driver keeps among the roots)
    std::vector<double> d2(nroots), dinf(nroots);
    BK_TRY(v_deflation_dist(ctx, prob->nloc, x, roots, nroots, d2.data(), dinf.data()));
    double dmin = HUGE_VAL;
    for (int i = 0; i < nroots; ++i) {
        const double di = norm_inf ? dinf[i] : std::sqrt(d2[i]);
        dmin = (di != di || di < dmin) ? di : dmin;                 // a NaN distance is not "far from every root"
        if (di != di) break;
    }
    res->converged = o.converged;
    res->itnewton = o.itnewton;
    res->itlinear = o.itlinear;
    res->M = o.M;
    res->min_dist = o.min_dist;
    res->plain_residual = o.plain_residual;
    res->min_dist_normC = dmin;
    res->itnewton_total = total;
    // the reference's order: Newton converged (:274), the plain residual (:281), no known root within tol (:282)
    res->reason = !o.converged ? 1 : !(o.plain_residual < tol) ? 2 : !(dmin >= tol) ? 3 : 0;
    res->accepted = res->reason == 0;
    return 0;
}

}  // extern "C"
