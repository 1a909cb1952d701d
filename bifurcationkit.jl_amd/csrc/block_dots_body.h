// Body of the block Arnoldi projection pass (vecops.hip: block_dots_kernel; block_dots_wide.hip: block_dots_wide_kernel): one
// function template so that every kernel head that runs it gives each accumulator the same fma sequence -- the instantiations
// differ only in how many basis vectors (KB), right-hand slots (NRT) and triangle values (TRI) they keep in registers.
// Per workgroup: KB x NRT values [i * NRT + r], then (TRI) the NRT (NRT + 1) / 2 triangle values in row order.
// Internal header.
#pragma once
#include "stream.h"

namespace bk {
namespace {

template <int KB, bool TRI, int U, bool LDNT, int NRT>
__device__ __forceinline__ void block_dots_body(size_t n, const double* __restrict__ V, size_t ldv, int kb,
                                                const double* __restrict__ Rv, int nr, double* __restrict__ partials) {
    constexpr int NR = NRT, NT3 = TRI ? NRT * (NRT + 1) / 2 : 1;
    double acc[KB > 0 ? KB : 1][NR], tri[NT3];
#pragma unroll
    for (int i = 0; i < (KB > 0 ? KB : 1); ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[i][r] = 0.0;
#pragma unroll
    for (int t = 0; t < NT3; ++t) tri[t] = 0.0;
    stream_loop<U>(n >> 1, [&](auto uc, size_t i0, size_t st) {
        constexpr int UU = decltype(uc)::value;
        double2 rv[NR][UU];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r < nr) {
#pragma unroll
                for (int u = 0; u < UU; ++u) rv[r][u] = ld2<LDNT>(Rv + (size_t)r * ldv, i0 + u * st);
            } else {
#pragma unroll
                for (int u = 0; u < UU; ++u) rv[r][u] = make_double2(0.0, 0.0);
            }
        }
        if (TRI) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int c = r; c < NR; ++c) {
                    double a = tri[TRI ? r * NR - r * (r - 1) / 2 + (c - r) : 0];
#pragma unroll
                    for (int u = 0; u < UU; ++u) { a = fma(rv[r][u].x, rv[c][u].x, a); a = fma(rv[r][u].y, rv[c][u].y, a); }
                    tri[TRI ? r * NR - r * (r - 1) / 2 + (c - r) : 0] = a;
                }
        }
#pragma unroll
        for (int i = 0; i < KB; ++i) {
            if (i < kb) {
                double2 vv[UU];
#pragma unroll
                for (int u = 0; u < UU; ++u) vv[u] = ld2<LDNT>(V + (size_t)i * ldv, i0 + u * st);
#pragma unroll
                for (int r = 0; r < NR; ++r)
#pragma unroll
                    for (int u = 0; u < UU; ++u) { acc[i][r] = fma(vv[u].x, rv[r][u].x, acc[i][r]); acc[i][r] = fma(vv[u].y, rv[r][u].y, acc[i][r]); }
            }
        }
    });
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double rl[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) rl[r] = r < nr ? Rv[(size_t)r * ldv + n - 1] : 0.0;
        if (TRI) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int c = r; c < NR; ++c) tri[TRI ? r * NR - r * (r - 1) / 2 + (c - r) : 0] = fma(rl[r], rl[c], tri[TRI ? r * NR - r * (r - 1) / 2 + (c - r) : 0]);
        }
#pragma unroll
        for (int i = 0; i < KB; ++i)
            if (i < kb) {
                const double vl = V[(size_t)i * ldv + n - 1];
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[i][r] = fma(vl, rl[r], acc[i][r]);
            }
    }
    constexpr int NV = KB * NR + (TRI ? NR * (NR + 1) / 2 : 0);
    __shared__ double sm[4][NV];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < KB; ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double s_ = wave_sum(acc[i][r]);
            if (lane == 0) sm[wid][i * NR + r] = s_;
        }
    if (TRI) {
#pragma unroll
        for (int t = 0; t < NT3; ++t) {
            const double s_ = wave_sum(tri[t]);
            if (lane == 0) sm[wid][KB * NR + t] = s_;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < NV; j += kThreads)
        partials[(size_t)blockIdx.x * NV + j] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
}

}  // namespace
}  // namespace bk
