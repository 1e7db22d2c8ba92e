// libqbp.so, translation unit of the Pauli-frame simulator (qbp_frame.hpp): the sampling and the enumeration build of
// frame_sim_kernel, and frame_assemble_kernel.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#define QBP_FRAME_TU
#include "qbp_frame.hpp"
#include "qbp_launch.hpp"

static_assert(QBP_FRAME_PHILOX_STREAM == qbp::FRAME_PHILOX_WORD3, "Philox counter word 3 of the frame sampler");
static_assert(QBP_FRAME_MAX_CLASSES == qbp::FRAME_MAX_CLASSES, "rate classes of the frame sampler");
static_assert(QBP_FRAME_RZ == qbp::FRAME_RZ && QBP_FRAME_RX == qbp::FRAME_RX && QBP_FRAME_CX == qbp::FRAME_CX &&
              QBP_FRAME_MZ == qbp::FRAME_MZ && QBP_FRAME_MX == qbp::FRAME_MX && QBP_FRAME_XERR == qbp::FRAME_XERR &&
              QBP_FRAME_ZERR == qbp::FRAME_ZERR && QBP_FRAME_DEP1 == qbp::FRAME_DEP1 && QBP_FRAME_DEP2 == qbp::FRAME_DEP2,
              "op kinds of the frame simulator");

namespace qbp {

hipError_t launch_frame_sim(bool sample, const FrameParams& P, hipStream_t s)
{
    const dim3 grid((unsigned)((P.W + FRAME_SIM_THREADS - 1) / FRAME_SIM_THREADS)), block(FRAME_SIM_THREADS);
    if (sample) hipLaunchKernelGGL(frame_sim_kernel<true>, grid, block, 0, s, P);
    else hipLaunchKernelGGL(frame_sim_kernel<false>, grid, block, 0, s, P);
    return hipGetLastError();
}

hipError_t launch_frame_assemble(const FrameParams& P, unsigned grid, hipStream_t s)
{
    hipLaunchKernelGGL(frame_assemble_kernel, dim3(grid), dim3(FRAME_THREADS), 0, s, P);
    return hipGetLastError();
}

}  // namespace qbp
