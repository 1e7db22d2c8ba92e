// libqbp.so, translation unit of the Relay-BP kernel (qbp_relay.hpp): the batch build and the records build.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_relay.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <bool RECORDS>
hipError_t relay_launch_k(const RelayParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    auto kern = bp_relay_kernel<RECORDS>;
    static thread_local size_t lds_set[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || lds_set[dev] < lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) lds_set[dev] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_relay(bool records, const RelayParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    return records ? relay_launch_k<true>(P, grid, threads, lds, s) : relay_launch_k<false>(P, grid, threads, lds, s);
}

}  // namespace qbp
