// libqbp.so, translation unit of the Relay-BP kernels (qbp_relay.hpp): the batch build and the records build of
// bp_relay_kernel, each with the messages in LDS and (LARGE) in a global workspace.
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_relay.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <bool RECORDS, bool LARGE>
hipError_t relay_launch_k(const RelayParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<bp_relay_kernel<RECORDS, LARGE>>(dim3(grid), dim3(threads), lds, s, P);
}

}  // namespace

hipError_t launch_relay(bool records, bool large, const RelayParams& P, int grid, int threads, size_t lds,
                        hipStream_t s)
{
    if (large)
        return records ? relay_launch_k<true, true>(P, grid, threads, lds, s)
                       : relay_launch_k<false, true>(P, grid, threads, lds, s);
    return records ? relay_launch_k<true, false>(P, grid, threads, lds, s)
                   : relay_launch_k<false, false>(P, grid, threads, lds, s);
}

}  // namespace qbp
