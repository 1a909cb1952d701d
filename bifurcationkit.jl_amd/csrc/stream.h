// Streaming scaffolding of the HBM-bound kernels (vecops.hip, fold.hip, hopf.hip, and minaug.h for the epilogue the last two
// share): 256-thread workgroups, 16-byte loads per lane, the contiguous-burst grid-stride walk and the wave64 sum.
// Internal header.
#pragma once
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace bk {
namespace {

constexpr int kThreads = 256;

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

}  // namespace
}  // namespace bk
