// libqbp.so, translation unit of BP with a prior per record (qbp_cond.hpp: bp_cond_kernel, sum-product and min-sum) and
// of the glue kernels of the two-stage CSS decoder (Pauli sampler, correction select, classification of both sectors).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/qbp.h"
#define QBP_COND_TU
#include "qbp_cond.hpp"
#include "qbp_launch.hpp"

static_assert(QBP_CSS_PHILOX_STREAM == qbp::CSS_PHILOX_WORD3, "Philox counter word 3 of the Pauli sampler");

namespace qbp {
namespace {

template <int VARIANT>
hipError_t cond_launch_k(const CondParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<bp_cond_kernel<VARIANT>>(dim3(grid), dim3(threads), lds, s, P);
}

// blocks for `items` lanes' worth of work: at most CSS_MAX_GRID, the kernels stride over the rest
unsigned css_grid(long long items)
{
    const long long blocks = (items + CSS_THREADS - 1) / CSS_THREADS;
    return (unsigned)std::max<long long>(1, std::min<long long>(blocks, CSS_MAX_GRID));
}

}  // namespace

hipError_t launch_cond(int variant, const CondParams& P, int grid, int threads, size_t lds, hipStream_t s)
{
    return variant == QBP_MIN_SUM ? cond_launch_k<2>(P, grid, threads, lds, s) : cond_launch_k<0>(P, grid, threads, lds, s);
}

hipError_t launch_css_sample_pauli(uint8_t* e_a, uint8_t* e_b, int n, long long T, long long trial_begin,
                                   unsigned long long seed, unsigned t1, unsigned t2, unsigned t3, hipStream_t s)
{
    hipLaunchKernelGGL(css_sample_pauli_kernel, dim3(css_grid(T * ((n + 3) / 4))), dim3(CSS_THREADS), 0, s, e_a, e_b, n, T,
                       trial_begin, seed, t1, t2, t3);
    return hipGetLastError();
}

hipError_t launch_css_select(const uint8_t* hard, const uint8_t* sol, const uint8_t* conv, long long T, int n, uint8_t* x,
                             hipStream_t s)
{
    hipLaunchKernelGGL(css_select_kernel, dim3(css_grid(T * n)), dim3(CSS_THREADS), 0, s, hard, sol, conv, T, n, x);
    return hipGetLastError();
}

hipError_t launch_css_classify(const CssClassify& P, hipStream_t s)
{
    hipLaunchKernelGGL(css_classify_kernel, dim3(css_grid(P.T * 64)), dim3(CSS_THREADS), 0, s, P);
    return hipGetLastError();
}

}  // namespace qbp
