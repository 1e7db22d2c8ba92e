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
    auto kern = lsd_kernel<RECORDS>;
    static thread_local size_t lds_set[64] = {0};
    const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(kern), lds, lds_set);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, s, P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lsd(bool records, const LsdParams& P, unsigned grid, size_t lds, hipStream_t s)
{
    return records ? lsd_launch_k<true>(P, grid, lds, s) : lsd_launch_k<false>(P, grid, lds, s);
}

}  // namespace qbp
