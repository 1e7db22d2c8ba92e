// libqbp.so, translation unit of the fixed-point min-sum kernel (qbp_quant.hpp): int8 and int16 messages, the batch
// build and the Monte-Carlo build.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_quant.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <typename MsgT, bool MC>
hipError_t quant_launch_k(const QuantParams& P, int grid, size_t lds, hipStream_t s)
{
    auto kern = bp_quant_kernel<MsgT, MC>;
    static thread_local size_t lds_set[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || lds_set[dev] < lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) lds_set[dev] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(QUANT_THREADS), lds, s, P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_quant(bool mc, bool wide, const QuantParams& P, int grid, size_t lds, hipStream_t s)
{
    if (wide) return mc ? quant_launch_k<int16_t, true>(P, grid, lds, s) : quant_launch_k<int16_t, false>(P, grid, lds, s);
    return mc ? quant_launch_k<int8_t, true>(P, grid, lds, s) : quant_launch_k<int8_t, false>(P, grid, lds, s);
}

}  // namespace qbp
