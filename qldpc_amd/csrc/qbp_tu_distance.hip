// libqbp.so, translation unit of the distance search kernel (qbp_distance.hpp): the search build and the capture build.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_distance.hpp"
#include "qbp_launch.hpp"

static_assert(QBP_DISTANCE_PHILOX_STREAM == qbp::DIST_PHILOX_WORD3, "Philox counter word 3 of the distance search");

namespace qbp {

hipError_t launch_dist_search(bool capture, const DistParams& P, unsigned grid, size_t lds, hipStream_t s)
{
    return capture ? launch_dynamic_lds<dist_search_kernel<true>>(dim3(grid), dim3(64), lds, s, P)
                   : launch_dynamic_lds<dist_search_kernel<false>>(dim3(grid), dim3(64), lds, s, P);
}

}  // namespace qbp
