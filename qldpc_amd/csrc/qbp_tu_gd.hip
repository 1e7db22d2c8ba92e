// libqbp.so, translation unit of the BP guided decimation kernel (qbp_gd.hpp): sum-product and min-sum, the batch
// build and the records build, each with the messages in LDS and (LARGE) in a global workspace.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_gd.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <int VARIANT, bool RECORDS, bool LARGE>
hipError_t gd_launch_k(const GdParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<bp_gd_kernel<VARIANT, RECORDS, LARGE>>(dim3(grid), dim3(threads), lds, s, P);
}

}  // namespace

namespace {

template <bool LARGE>
hipError_t gd_launch_layout(bool records, int variant, const GdParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    if (variant == QBP_MIN_SUM)
        return records ? gd_launch_k<2, true, LARGE>(P, grid, threads, lds, s)
                       : gd_launch_k<2, false, LARGE>(P, grid, threads, lds, s);
    return records ? gd_launch_k<0, true, LARGE>(P, grid, threads, lds, s)
                   : gd_launch_k<0, false, LARGE>(P, grid, threads, lds, s);
}

}  // namespace

hipError_t launch_gd(bool records, bool large, int variant, const GdParams& P, int grid, int threads, size_t lds,
                     hipStream_t s)
{
    return large ? gd_launch_layout<true>(records, variant, P, grid, threads, lds, s)
                 : gd_launch_layout<false>(records, variant, P, grid, threads, lds, s);
}

}  // namespace qbp
