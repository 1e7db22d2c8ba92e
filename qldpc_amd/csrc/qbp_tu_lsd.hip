// libqbp.so, translation unit of the localized statistics decoding kernels (qbp_lsd.hpp; qbp_lsd_large.hpp, the rows
// in a global workspace): the batch build and the records build of each.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_lsd.hpp"
#include "qbp_lsd_large.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <bool RECORDS>
hipError_t lsd_launch_k(const LsdParams& P, unsigned grid, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<lsd_kernel<RECORDS>>(dim3(grid), dim3(64), lds, s, P);
}

template <bool RECORDS>
hipError_t lsd_large_launch_k(const LsdParams& P, const LsdLargeWorkspace& Wk, unsigned grid, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<lsd_large_kernel<RECORDS>>(dim3(grid), dim3(LSD_LARGE_THREADS), lds, s, P, Wk);
}

}  // namespace

hipError_t launch_lsd(bool records, const LsdParams& P, unsigned grid, size_t lds, hipStream_t s)
{
    return records ? lsd_launch_k<true>(P, grid, lds, s) : lsd_launch_k<false>(P, grid, lds, s);
}

hipError_t launch_lsd_large(bool records, const LsdParams& P, const LsdLargeWorkspace& Wk, unsigned grid, size_t lds,
                            hipStream_t s)
{
    return records ? lsd_large_launch_k<true>(P, Wk, grid, lds, s) : lsd_large_launch_k<false>(P, Wk, grid, lds, s);
}

}  // namespace qbp
