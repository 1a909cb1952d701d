// The first projection launch of a block with SIX right-hand vectors (sstep.h; vecops.hip: v_block_dots): 8 measured basis vectors,
// the 6 right-hand vectors and their triangle in one visit -- 8 x 6 + 21 = 69 accumulators, one more than the 4 x 8 + 36 launch --
// where the 8-slot routing runs (4 + 6) + (4 + 6) streams in two launches with two reductions.  A solve whose last block is two
// steps after a four-step block (u = 4, s = 2) ends on this shape.  Same body (block_dots_body.h), same grid, same items per lane
// and same load path as the launches it replaces: every accumulator sees the fma sequence it saw there, so D and T keep their bits.
#include <algorithm>

#include "block_dots_body.h"
#include "common.h"
#include "sstep.h"
#include "stream.h"

namespace bk {

namespace {

template <int KB, int U, bool LDNT, int NRT>
__global__ void __launch_bounds__(kThreads) block_dots_wide_kernel(size_t n, const double* __restrict__ V, size_t ldv, int kb,
                                                                   const double* __restrict__ Rv, int nr, double* __restrict__ partials) {
    block_dots_body<KB, true, U, LDNT, NRT>(n, V, ldv, kb, Rv, nr, partials);
}

}  // namespace

// D[i * 8 + r] for the first min(kold, 8) basis vectors and all of T; *done = basis vectors covered.  grid and nt as v_block_dots
// chose them for its other launches; 5 < nr <= kBlockDotsWideNr.
int block_dots_wide(bk_ctx* ctx, int grid, bool nt, size_t n, const double* V, size_t ldv, int kold, const double* Rv, int nr,
                    double* D, double* T, int* done) {
    constexpr int NRW = kBlockDotsWideNr, NV = 8 * NRW + NRW * (NRW + 1) / 2;
    static_assert(NV <= kPartialVals && NV <= kRedSlots && NRW <= sstep::kR, "d_partials / h_red too small");
    if (nr < 1 || nr > NRW || kold < 1) return set_error(ctx, "block_dots_wide: bad sizes");
    const int kb = std::min(kold, 8);
    {
        ProfScope ps(ctx, "multidot", 8.0 * n * (kb + nr));
        if (nt) hipLaunchKernelGGL((block_dots_wide_kernel<8, 2, true, NRW>), dim3(grid), dim3(kThreads), 0, ctx->stream, n, V, ldv, kb, Rv, nr, ctx->d_partials);
        else hipLaunchKernelGGL((block_dots_wide_kernel<8, 2, false, NRW>), dim3(grid), dim3(kThreads), 0, ctx->stream, n, V, ldv, kb, Rv, nr, ctx->d_partials);
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, grid, NV, 0));
    for (int i = 0; i < kb; ++i)
        for (int r = 0; r < sstep::kR; ++r) D[i * sstep::kR + r] = r < NRW ? ctx->h_red[i * NRW + r] : 0.0;
    for (int t = 0; t < sstep::kTri; ++t) T[t] = 0.0;
    for (int r = 0, t = 0; r < NRW; ++r)
        for (int c = r; c < NRW; ++c, ++t) T[sstep::tri(r, c)] = ctx->h_red[8 * NRW + t];
    *done = kb;
    return 0;
}

}  // namespace bk
