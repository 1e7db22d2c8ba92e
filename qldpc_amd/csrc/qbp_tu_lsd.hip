// libqbp.so, translation unit of the localized statistics decoding kernel (qbp_lsd.hpp): the batch build and the
// records build.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_lsd.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <bool RECORDS>
hipError_t lsd_launch_k(const LsdParams& P, unsigned grid, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<lsd_kernel<RECORDS>>(dim3(grid), dim3(64), lds, s, P);
}

}  // namespace

hipError_t launch_lsd(bool records, const LsdParams& P, unsigned grid, size_t lds, hipStream_t s)
{
    return records ? lsd_launch_k<true>(P, grid, lds, s) : lsd_launch_k<false>(P, grid, lds, s);
}

}  // namespace qbp
