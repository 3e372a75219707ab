// marf_gn.hip -- the plain Gauss-Newton launches (marf_gn_normal): marf_gn_dev.h's tile
// kernel without the robust weight, and the reduction of a patch's tile partials.  The robust launches
// are marf_gn_robust.hip's.
#include "marf_gn_dev.h"

namespace marf {

// out[b][e] = the sum of patch b's tile partials [tpp][56] of value e, in fp64, in tile order
__global__ __launch_bounds__(64) void k_gn_reduce(const double* __restrict__ part, int tpp, int nvals,
                                                  double* __restrict__ out) {
    const int e = threadIdx.x;
    if (e >= nvals) return;
    const double* p = part + (size_t)blockIdx.x * tpp * GN_VALS + e;
    double s = 0.0;
    // unrolled so 8 partial loads are in flight per thread (latency-bound); the summation order is unchanged
#pragma unroll 8
    for (int t = 0; t < tpp; ++t) s += p[(size_t)t * GN_VALS];
    out[(size_t)blockIdx.x * GN_VALS + e] = s;
}

}  // namespace marf

using namespace marf;

// split: the bf16x3 tile recipe (TP 128 or 64); else fp32 (TP 64)
hipError_t marf_launch_gn(const GnArgs& a, bool split, int TP, bool loss_only, size_t lds, int n_tiles, hipStream_t s,
                          bool robust) {
    return robust ? marf_launch_gn_robust(a, split, TP, loss_only, lds, n_tiles, s)
                  : pick_gn<false>(a, split, TP, loss_only, lds, n_tiles, s);
}

hipError_t marf_launch_gn_reduce(const double* partial, int tiles_per_patch, int B, bool loss_only, double* out,
                                 hipStream_t s) {
    hipLaunchKernelGGL(k_gn_reduce, dim3(B), dim3(64), 0, s, partial, tiles_per_patch, loss_only ? 2 : GN_VALS, out);
    return hipGetLastError();
}
