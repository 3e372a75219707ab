// marf_gn_robust.hip -- the ROBUST instantiations of marf_gn_dev.h's tile kernel (marf_gn_normal_robust:
// Huber / Cauchy IRLS), in a unit of their own so that the plain kernels of marf_gn.hip
// compile as they did without them.
#include "marf_gn_dev.h"

using namespace marf;

hipError_t marf_launch_gn_robust(const GnArgs& a, bool split, int TP, bool loss_only, size_t lds, int n_tiles,
                                 hipStream_t s) {
    return pick_gn<true>(a, split, TP, loss_only, lds, n_tiles, s);
}
