// libqbp.so, translation unit of the layered BP kernels (qbp_layered.hpp): sum-product and min-sum, the batch build and
// the Monte-Carlo build of bp_layered_kernel, each with the messages in LDS and (LARGE) in a global workspace.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_layered.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <int VARIANT, bool MC, bool LARGE>
hipError_t layered_launch_k(const LayeredParams& P, int grid, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<bp_layered_kernel<VARIANT, MC, LARGE>>(dim3(grid), dim3(LAYERED_THREADS), lds, s, P);
}

template <int VARIANT>
hipError_t layered_launch_v(bool mc, bool large, const LayeredParams& P, int grid, size_t lds, hipStream_t s)
{
    if (large)
        return mc ? layered_launch_k<VARIANT, true, true>(P, grid, lds, s)
                  : layered_launch_k<VARIANT, false, true>(P, grid, lds, s);
    return mc ? layered_launch_k<VARIANT, true, false>(P, grid, lds, s)
              : layered_launch_k<VARIANT, false, false>(P, grid, lds, s);
}

}  // namespace

hipError_t launch_layered(bool mc, bool large, int variant, const LayeredParams& P, int grid, size_t lds,
                          hipStream_t s)
{
    if (variant == QBP_MIN_SUM) return layered_launch_v<2>(mc, large, P, grid, lds, s);
    if (variant == QBP_SUM_PRODUCT) return layered_launch_v<0>(mc, large, P, grid, lds, s);
    return hipErrorInvalidValue;
}

}  // namespace qbp
