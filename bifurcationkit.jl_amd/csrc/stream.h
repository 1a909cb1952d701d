// Streaming scaffolding of the HBM-bound kernels: 256-thread workgroups, 16-byte loads per lane, the contiguous-burst grid-stride
// walk and the wave64 sum (vecops.hip), and on top of them the generic passes of fold.hip, hopf.hip, hopf_nf.hip, bautin.hip, nf1d.hip, nfnd.hip
// and bt.hip: reducing, writing, and writing-and-reducing (stream_write_reduce, last in this file).
//
// How to add a streaming pass: write a plain struct with `static constexpr int NIN, U, FIELDS` (read streams; 16-byte items per
// lane in flight; streams per vector: 2 when the stacked cGL fields p, p + n are walked side by side over n points, x[2 k + f] =
// field f of vector k), the vectors `const double* in[NIN / FIELDS]`, its coefficients, and the mathematics of ONE element:
//   reducing  NV,                            operator()(const double (&x)[NIN], double (&s)[NV]) const   adds the element's terms to s
//   writing   NOUT, double* out[NOUT / FIELDS], operator()(const double (&x)[NIN], double (&o)[NOUT]) const, and JOINT
//             (true: the outputs of an element share work, form them all and then store; false: store each as it is formed)
// Fill it on the host and call stream_reduce(ctx, name, n, pass, out) or stream_write(ctx, name, n, pass), n = elements per
// stream.  Load path, grid, profiling scope and the two-stage sum are theirs; a count that selects the struct (Pass<M>) goes
// through count_dispatch.  The element order per lane is fixed here, so the sums are bitwise reproducible (test_gpu_stream_pass_bits).
// Internal header.
#pragma once
#include <cstdint>
#include <type_traits>
#include <utility>

#include "common.h"

namespace bk {
namespace {

constexpr int kThreads = 256;
constexpr int kVecPairs = -2;      // load path of stream_visit: pairs of elements in the order of the 16-byte path, 8-byte accesses

inline int grid_for(size_t n, int per_thread, int max_blocks) {
    size_t b = (n + (size_t)kThreads * per_thread - 1) / ((size_t)kThreads * per_thread);
    if (b < 1) b = 1;
    if (b > (size_t)max_blocks) b = max_blocks;
    return (int)b;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// non-temporal hint only for vectors that cannot live in the caches anyway (>= 32 MiB): the cache-resident 2-D configs keep
// their operands in L2 / Infinity Cache between kernels
inline bool nt_hint(bk_ctx* ctx, size_t n) { return n >= ((size_t)1 << 22) && ctx->opt("nt_hint", 1.0) != 0.0; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Streams that are read exactly once per kernel (Krylov basis vectors, BLAS-1 operands) are loaded with the non-temporal
// hint: measured at 512^3 (profiles/r2_kernel_variants_512_nt_loads.jsonl) multidot 6.3 -> 6.6-6.9 TB/s, multiaxpy
// 5.1-5.3 -> 5.6 TB/s (with two elements per lane in flight).
typedef double nt_d2 __attribute__((ext_vector_type(2)));
template <bool LDNT>
__device__ __forceinline__ double2 ld2(const double* p, size_t i) {
    if (LDNT) {
        const nt_d2 t = __builtin_nontemporal_load(reinterpret_cast<const nt_d2*>(p) + i);
        return make_double2(t.x, t.y);
    }
    return reinterpret_cast<const double2*>(p)[i];
}

// Grid-stride walk over n2 16-byte items with U items per lane in flight: full iterations carry no bounds guard (the
// body sees a compile-time item count, so all its loads are issued back to back -- a runtime guard per operand or per item
// makes the compiler emit load / s_waitcnt vmcnt(0) pairs, i.e. one exposed memory latency per operand), the ragged end
// runs item by item.  body(integral_constant<int, UU>, first_item, step).
template <int U, class Body>
__device__ __forceinline__ void stream_loop(size_t n2, Body&& body) {
    // a workgroup owns U ADJACENT 4-KiB chunks per iteration (one 16-KiB contiguous burst per stream), not U chunks a whole
    // grid stride apart: measured at 512^3, the strided form costs 25 % (axpby 0.55 vs 0.73 of peak) -- it multiplies the
    // number of DRAM pages the chip has open per stream
    const size_t chunk = (size_t)kThreads * U;
    const size_t gstep = (size_t)gridDim.x * chunk;
    size_t base = (size_t)blockIdx.x * chunk;
    for (; base + chunk <= n2; base += gstep) body(std::integral_constant<int, U>{}, base + threadIdx.x, (size_t)kThreads);
    if (base < n2)
        for (size_t i = base + threadIdx.x; i < n2 && i < base + chunk; i += kThreads) body(std::integral_constant<int, 1>{}, i, (size_t)kThreads);
}

// ------------------------------------------------------------------ generic passes
__device__ __forceinline__ void st2(double* p, size_t i, double a, double b) { reinterpret_cast<double2*>(p)[i] = make_double2(a, b); }

// Epilogue of a reducing kernel: NV sums per lane -> NV partial sums of the workgroup, partials[blockIdx.x * NV + k].  Wave
// sums, then the four waves in the fixed order (0 + 1) + (2 + 3); the second stage (reduce_finish) keeps a fixed order too.
template <int NV>
__device__ __forceinline__ void block_sum_store(const double (&s)[NV], double* partials) {
    __shared__ double sm[NV][4];
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double t = wave_sum(s[k]);
        if (lane == 0) sm[k][wv_] = t;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int k = threadIdx.x;
        partials[(size_t)blockIdx.x * NV + k] = (sm[k][0] + sm[k][1]) + (sm[k][2] + sm[k][3]);
    }
}

// The three load paths of a pass over n elements of NIN = NB x F streams, stream j = field j % F of the vector in[j / F] of F
// stacked fields (in[j / F] + (j % F) n: one pointer per vector is kept, not one per stream -- the nine vectors of
// HopfNfContract as eighteen pointers run out of SGPRs and are re-read from the kernel arguments inside the loop).  visit(integral_constant<int, K>, i, x) with x[K][NIN]:
// K = 2 on the vector path (VEC == 2) -- x[0], x[1] are elements 2 i and 2 i + 1 of every stream; per iteration all NIN x UU
// loads are issued before the first visit, items in the order q = 0..UU-1 -- and K = 1, element i, for the odd last element
// (block 0 / thread 0, after the walk) and on the element-by-element path (VEC == 1).  VEC == kVecPairs walks the pairs of the
// vector path in its order with two 8-byte loads per pair: for misaligned streams of a pass whose sums must not depend on the
// alignment (stream_write_reduce).
template <int U, int VEC, bool NTH, int F, int NB, class Visit>
__device__ __forceinline__ void stream_visit(size_t n, const double* const (&in)[NB], Visit&& visit) {
    constexpr int NIN = NB * F;
    auto stream = [&](int j) { return in[j / F] + (j % F) * n; };
    auto one = [&](size_t i) {
        double x[1][NIN];
#pragma unroll
        for (int j = 0; j < NIN; ++j) x[0][j] = stream(j)[i];
        visit(std::integral_constant<int, 1>{}, i, x);
    };
    if (VEC == 2 || VEC == kVecPairs) {
        stream_loop<U>(n >> 1, [&](auto uc, size_t i0, size_t st) {
            constexpr int UU = decltype(uc)::value;
            double2 v[UU][NIN];
#pragma unroll
            for (int q = 0; q < UU; ++q)
#pragma unroll
                for (int j = 0; j < NIN; ++j) {
                    if constexpr (VEC == 2) {
                        v[q][j] = ld2<NTH>(stream(j), i0 + q * st);
                    } else {
                        const double* p = stream(j) + 2 * (i0 + q * st);
                        v[q][j] = make_double2(p[0], p[1]);
                    }
                }
#pragma unroll
            for (int q = 0; q < UU; ++q) {
                double x[2][NIN];
#pragma unroll
                for (int j = 0; j < NIN; ++j) { x[0][j] = v[q][j].x; x[1][j] = v[q][j].y; }
                visit(std::integral_constant<int, 2>{}, i0 + q * st, x);
            }
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) one(i);
    }
}

// Pass::NV partial sums per workgroup; every lane adds its elements in the order of stream_visit, .x before .y
template <class Pass, int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) stream_reduce_kernel(size_t n, Pass pass, double* __restrict__ partials) {
    double s[Pass::NV];
#pragma unroll
    for (int k = 0; k < Pass::NV; ++k) s[k] = 0.0;
    stream_visit<Pass::U, VEC, NTH, Pass::FIELDS>(n, pass.in, [&](auto kc, size_t, const auto& x) {
#pragma unroll
        for (int e = 0; e < decltype(kc)::value; ++e) pass(x[e], s);
    });
    block_sum_store<Pass::NV>(s, partials);
}

// The read vectors travel as __restrict__ kernel parameters (in = pass.in[...]): pointers inside a struct carry no such
// promise, and without it the loads are scheduled around the stores -- HopfNfRhs then takes 88 VGPRs instead of 62.
// Pass::JOINT = false stores output j before output j + 1 is formed: the body is inlined once per output and the compiler
// drops what that output does not need (HopfOrbit<8>: 45 VGPRs and 1 % faster than with all eight formed first); passes whose
// outputs share work (HopfNfRhs: one Hessian for six outputs) form them in one evaluation, or the shared values stay live
// across the stores (86 VGPRs).
template <class Pass, int VEC, bool NTH, class... In>
__global__ void __launch_bounds__(kThreads) stream_write_kernel(size_t n, Pass pass, In* __restrict__... in) {
    constexpr int F = Pass::FIELDS;
    const double* const ins[Pass::NIN / F] = {in...};
    stream_visit<Pass::U, VEC, NTH, F>(n, ins, [&](auto kc, size_t i, const auto& x) {
        constexpr int K = decltype(kc)::value;
        double o[K][Pass::NOUT];
        if (Pass::JOINT) {
#pragma unroll
            for (int e = 0; e < K; ++e) pass(x[e], o[e]);
        }
#pragma unroll
        for (int j = 0; j < Pass::NOUT; ++j) {
            if (!Pass::JOINT) {
#pragma unroll
                for (int e = 0; e < K; ++e) pass(x[e], o[e]);
            }
            double* out = pass.out[j / F] + (j % F) * n;
            if constexpr (K == 2) st2(out, i, o[0][j], o[1][j]);
            else out[i] = o[0][j];
        }
    });
}

// launch(VEC, NTH) as integral constants: the load path of a kernel template <..., int VEC, bool NTH> -- non-temporal 16-byte
// loads (nth), 16-byte loads (vec) or element by element
template <class Launch>
void load_path_dispatch(bool vec, bool nth, Launch&& launch) {
    if (nth) launch(std::integral_constant<int, 2>{}, std::true_type{});
    else if (vec) launch(std::integral_constant<int, 2>{}, std::false_type{});
    else launch(std::integral_constant<int, 1>{}, std::false_type{});
}

// f(integral_constant<int, M>) for M = m clamped to LO..HI: a run-time count into the template argument of a pass
template <int LO, int HI, class F>
int count_dispatch(int m, F&& f) {
    if constexpr (LO < HI) {
        if (m > LO) return count_dispatch<LO + 1, HI>(m, f);
    }
    return f(std::integral_constant<int, LO>{});
}

// every one of the `fields` stacked fields of n elements of every vector 16-byte aligned
template <class T, int N>
bool all_aligned16(T* const (&p)[N], size_t n, int fields) {
    for (int j = 0; j < N; ++j)
        for (int f = 0; f < fields; ++f)
            if (!aligned16(p[j] + f * n)) return false;
    return true;
}

// The load path and grid of a pass: 16-byte loads only if every stream is 16-byte aligned (`vec`), the non-temporal hint by
// vector length, 2 U elements per thread on the vector path and 1 otherwise
struct StreamPlan { bool vec, nth; int grid; };
template <class Pass>
StreamPlan stream_plan(bk_ctx* ctx, size_t n, bool vec, int cap) {
    return {vec, vec && nt_hint(ctx, n * Pass::FIELDS), grid_for(n, vec ? 2 * Pass::U : 1, cap)};
}

// out[0..NV) = the sums of a reducing pass over n elements per stream, all-reduced (reduce_finish)
template <class Pass>
int stream_reduce(bk_ctx* ctx, const char* name, size_t n, const Pass& pass, double* out) {
    const StreamPlan pl = stream_plan<Pass>(ctx, n, all_aligned16(pass.in, n, Pass::FIELDS), kRedBlocks);
    {
        ProfScope ps(ctx, name, 8.0 * n * Pass::NIN);
        load_path_dispatch(pl.vec, pl.nth, [&](auto V, auto NT) {
            hipLaunchKernelGGL((stream_reduce_kernel<Pass, decltype(V)::value, decltype(NT)::value>), dim3(pl.grid), dim3(kThreads), 0,
                               ctx->stream, n, pass, ctx->d_partials);
        });
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, pl.grid, Pass::NV, 0));
    for (int k = 0; k < Pass::NV; ++k) out[k] = ctx->h_red[k];
    return 0;
}

template <int VEC, bool NTH, class Pass, size_t... J>
void stream_write_launch(bk_ctx* ctx, int grid, size_t n, const Pass& pass, std::index_sequence<J...>) {
    stream_write_kernel<Pass, VEC, NTH><<<dim3(grid), dim3(kThreads), 0, ctx->stream>>>(n, pass, pass.in[J]...);
}

// a writing pass over n elements per stream; the outputs must not alias the inputs or each other
template <class Pass>
int stream_write(bk_ctx* ctx, const char* name, size_t n, const Pass& pass) {
    if (n == 0) return 0;
    const StreamPlan pl = stream_plan<Pass>(ctx, n, all_aligned16(pass.in, n, Pass::FIELDS) && all_aligned16(pass.out, n, Pass::FIELDS), 4096);
    ProfScope ps(ctx, name, 8.0 * n * (Pass::NIN + Pass::NOUT));
    load_path_dispatch(pl.vec, pl.nth, [&](auto V, auto NT) {
        stream_write_launch<decltype(V)::value, decltype(NT)::value>(ctx, pl.grid, n, pass, std::make_index_sequence<Pass::NIN / Pass::FIELDS>{});
    });
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ a pass that writes AND reduces
// Pass: NIN, NOUT, NV, U, FIELDS, in[], out[], operator()(x, o, s) -- the element's outputs into o, its NV terms added to s.  The
// outputs are stored as stream_write_kernel stores them, the terms summed as stream_reduce_kernel sums them.  Both load paths walk
// pairs of elements in one order on one grid (VEC == 2: 16-byte accesses; kVecPairs when a stream is misaligned), so the sums are
// bitwise the same run to run AND between aligned and misaligned operands; the element-by-element path of the two passes above
// walks in another order, and their sums differ in the last bits between the paths.
template <class Pass, int VEC, bool NTH, class... In>
__global__ void __launch_bounds__(kThreads) stream_write_reduce_kernel(size_t n, Pass pass, double* __restrict__ partials,
                                                                       In* __restrict__... in) {
    constexpr int F = Pass::FIELDS;
    const double* const ins[Pass::NIN / F] = {in...};
    double s[Pass::NV];
#pragma unroll
    for (int k = 0; k < Pass::NV; ++k) s[k] = 0.0;
    stream_visit<Pass::U, VEC, NTH, F>(n, ins, [&](auto kc, size_t i, const auto& x) {
        constexpr int K = decltype(kc)::value;
        double o[K][Pass::NOUT];
#pragma unroll
        for (int e = 0; e < K; ++e) pass(x[e], o[e], s);
#pragma unroll
        for (int j = 0; j < Pass::NOUT; ++j) {
            double* out = pass.out[j / F] + (j % F) * n;
            if constexpr (K == 2 && VEC == 2) {
                st2(out, i, o[0][j], o[1][j]);
            } else if constexpr (K == 2) {
                out[2 * i] = o[0][j];
                out[2 * i + 1] = o[1][j];
            } else {
                out[i] = o[0][j];
            }
        }
    });
    block_sum_store<Pass::NV>(s, partials);
}

template <int VEC, bool NTH, class Pass, size_t... J>
void stream_write_reduce_launch(bk_ctx* ctx, int grid, size_t n, const Pass& pass, std::index_sequence<J...>) {
    stream_write_reduce_kernel<Pass, VEC, NTH><<<dim3(grid), dim3(kThreads), 0, ctx->stream>>>(n, pass, ctx->d_partials, pass.in[J]...);
}

// sums[0..NV) all-reduced; the outputs must not alias the inputs or each other
template <class Pass>
int stream_write_reduce(bk_ctx* ctx, const char* name, size_t n, const Pass& pass, double* sums) {
    static_assert(Pass::NV <= kPartialVals, "partial sums per workgroup");
    const bool vec = all_aligned16(pass.in, n, Pass::FIELDS) && all_aligned16(pass.out, n, Pass::FIELDS);
    const bool nth = vec && nt_hint(ctx, n * Pass::FIELDS);
    const int grid = grid_for(n, 2 * Pass::U, kRedBlocks);          // the same on both load paths
    {
        ProfScope ps(ctx, name, 8.0 * n * (Pass::NIN + Pass::NOUT));
        constexpr auto seq = std::make_index_sequence<Pass::NIN / Pass::FIELDS>{};
        if (nth) stream_write_reduce_launch<2, true>(ctx, grid, n, pass, seq);
        else if (vec) stream_write_reduce_launch<2, false>(ctx, grid, n, pass, seq);
        else stream_write_reduce_launch<kVecPairs, false>(ctx, grid, n, pass, seq);
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, grid, Pass::NV, 0));
    for (int k = 0; k < Pass::NV; ++k) sums[k] = ctx->h_red[k];
    return 0;
}

}  // namespace
}  // namespace bk
