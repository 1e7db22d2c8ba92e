// libqbp.so, translation unit of the sliding-window glue kernels (qbp_window.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/qbp.h"
#define QBP_WINDOW_TU
#include "qbp_window.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

// blocks for `items` lanes' worth of work: at most WINDOW_MAX_GRID, the kernels stride over the rest
unsigned window_grid(long long items)
{
    const long long blocks = (items + WINDOW_THREADS - 1) / WINDOW_THREADS;
    return (unsigned)std::max<long long>(1, std::min<long long>(blocks, WINDOW_MAX_GRID));
}

}  // namespace

hipError_t launch_window_gather(const uint8_t* r, long long B, int m, const int32_t* checks, int mk, uint8_t* syn,
                                hipStream_t s)
{
    hipLaunchKernelGGL(window_gather_kernel, dim3(window_grid(B * mk)), dim3(WINDOW_THREADS), 0, s, r, B, m, checks, mk, syn);
    return hipGetLastError();
}

hipError_t launch_window_gather_prior(const double* prior, const int32_t* vars, int total, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(window_gather_prior_kernel, dim3(window_grid(total)), dim3(WINDOW_THREADS), 0, s, prior, vars, total,
                       out);
    return hipGetLastError();
}

hipError_t launch_window_fail_list(const uint8_t* conv, long long B, long long* list, unsigned long long* count,
                                   hipStream_t s)
{
    hipLaunchKernelGGL(window_fail_list_kernel, dim3(window_grid(B)), dim3(WINDOW_THREADS), 0, s, conv, B, list, count);
    return hipGetLastError();
}

hipError_t launch_window_commit(const WindowCommit& P, bool final_pass, hipStream_t s)
{
    if (final_pass)
        hipLaunchKernelGGL(window_commit_kernel<true>, dim3(window_grid(P.B * 64)), dim3(WINDOW_THREADS), 0, s, P);
    else
        hipLaunchKernelGGL(window_commit_kernel<false>,
                           dim3(window_grid(P.B * ((long long)P.n_upd + P.n_commit + 1))), dim3(WINDOW_THREADS), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_window_syndrome(const uint8_t* errors, long long T, int m, int n, const int32_t* row_ptr,
                                  const int32_t* col_idx, uint8_t* syn, hipStream_t s)
{
    hipLaunchKernelGGL(window_syndrome_kernel, dim3(window_grid(T * m)), dim3(WINDOW_THREADS), 0, s, errors, T, m, n,
                       row_ptr, col_idx, syn);
    return hipGetLastError();
}

hipError_t launch_window_classify(const uint8_t* errors, const uint8_t* x, const uint8_t* valid, const int32_t* iters,
                                  const int32_t* fails, long long T, int n, const unsigned long long* lx_cols,
                                  int half_distance, long long* counters, hipStream_t s)
{
    hipLaunchKernelGGL(window_classify_kernel, dim3(window_grid(T * 64)), dim3(WINDOW_THREADS), 0, s, errors, x, valid,
                       iters, fails, T, n, lx_cols, half_distance, counters);
    return hipGetLastError();
}

}  // namespace qbp
