// libqbp.so, translation units of the general-H kernel (qbp_generic.hpp).  Compiled three times, once
// per memory mode (-DQBP_GENERIC_MEM=0 / 1 / 2: six instantiations each), so that the three builds run
// in parallel; the mode-0 unit also holds the dispatcher and the prior permutation kernel.
#ifndef QBP_GENERIC_MEM
#error "compile with -DQBP_GENERIC_MEM=0, 1 or 2"
#endif
// With -DQBP_COLS_TU: the three Monte-Carlo instantiations with a sampler threshold per qubit (qbp_mc_run_probs),
// under other names.
// With -DQBP_BUDGETS_TU: those three once more, checkpointing a running trial at a ladder of iteration budgets
// (qbp_mc_run_budgets).
// With -DQBP_SPECTRUM_TU: those three again, adding residual weights and iteration indices to tables
// (qbp_mc_run_spectrum).
// With -DQBP_SHOTS_TU: three that decode recorded shots (qbp_decode_shots).
// With -DQBP_LLRHIST_TU: the budgets builds once more, binning the posterior LLRs of every emission
// (qbp_mc_run_llr_hist).
#if defined(QBP_LLRHIST_TU)
#define QBP_MC_COLS 1
#define QBP_MC_BUDGETS 1
#define QBP_MC_LLRHIST 1
#define bp_generic_kernel bp_generic_llrhist_kernel
#elif defined(QBP_SHOTS_TU)
#define QBP_MC_SHOTS 1
#define bp_generic_kernel bp_generic_shots_kernel
#elif defined(QBP_SPECTRUM_TU)
#define QBP_MC_COLS 1
#define QBP_MC_SPECTRUM 1
#define bp_generic_kernel bp_generic_spectrum_kernel
#elif defined(QBP_BUDGETS_TU)
#define QBP_MC_COLS 1
#define QBP_MC_BUDGETS 1
#define bp_generic_kernel bp_generic_budgets_kernel
#elif defined(QBP_COLS_TU)
#define QBP_MC_COLS 1
#define bp_generic_kernel bp_generic_cols_kernel
#elif QBP_GENERIC_MEM == 0
#define QBP_DEFINE_KERNELS 1
#endif
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_generic.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <int VARIANT, bool MC, int MEM>
hipError_t generic_launch_k(const GenericParams& G, int grid, int threads, size_t lds, hipStream_t s)
{
    return launch_dynamic_lds<bp_generic_kernel<VARIANT, MC, MEM>>(dim3(grid), dim3(threads), lds, s, G);
}

template <bool MC, int MEM>
hipError_t generic_launch_v(int variant, const GenericParams& G, int grid, int threads, size_t lds, hipStream_t s)
{
    switch (variant) {
        case QBP_SUM_PRODUCT: return generic_launch_k<0, MC, MEM>(G, grid, threads, lds, s);
        case QBP_DAMPED_SP:   return generic_launch_k<1, MC, MEM>(G, grid, threads, lds, s);
        default:              return generic_launch_k<2, MC, MEM>(G, grid, threads, lds, s);
    }
}

}  // namespace

#define QBP_CAT2(a, b) a##b
#define QBP_CAT(a, b) QBP_CAT2(a, b)

#if defined(QBP_LLRHIST_TU)
// launch_generic_llrhist_mem0 / _mem1 / _mem2 (Monte-Carlo only)
hipError_t QBP_CAT(launch_generic_llrhist_mem, QBP_GENERIC_MEM)(int variant, const GenericParams& G, int grid, int threads,
                                                                size_t lds, hipStream_t s)
{
    return generic_launch_v<true, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s);
}
#elif defined(QBP_SHOTS_TU)
// launch_generic_shots_mem0 / _mem1 / _mem2 (Monte-Carlo only)
hipError_t QBP_CAT(launch_generic_shots_mem, QBP_GENERIC_MEM)(int variant, const GenericParams& G, int grid, int threads,
                                                              size_t lds, hipStream_t s)
{
    return generic_launch_v<true, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s);
}
#elif defined(QBP_SPECTRUM_TU)
// launch_generic_spectrum_mem0 / _mem1 / _mem2 (Monte-Carlo only)
hipError_t QBP_CAT(launch_generic_spectrum_mem, QBP_GENERIC_MEM)(int variant, const GenericParams& G, int grid, int threads,
                                                                 size_t lds, hipStream_t s)
{
    return generic_launch_v<true, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s);
}
#elif defined(QBP_BUDGETS_TU)
// launch_generic_budgets_mem0 / _mem1 / _mem2 (Monte-Carlo only)
hipError_t QBP_CAT(launch_generic_budgets_mem, QBP_GENERIC_MEM)(int variant, const GenericParams& G, int grid, int threads,
                                                                size_t lds, hipStream_t s)
{
    return generic_launch_v<true, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s);
}
#elif defined(QBP_COLS_TU)
// launch_generic_cols_mem0 / _mem1 / _mem2 (Monte-Carlo only)
hipError_t QBP_CAT(launch_generic_cols_mem, QBP_GENERIC_MEM)(int variant, const GenericParams& G, int grid, int threads,
                                                             size_t lds, hipStream_t s)
{
    return generic_launch_v<true, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s);
}
#else
// launch_generic_mem0 / _mem1 / _mem2: this unit's memory mode
hipError_t QBP_CAT(launch_generic_mem, QBP_GENERIC_MEM)(bool mc, int variant, const GenericParams& G, int grid,
                                                        int threads, size_t lds, hipStream_t s)
{
    return mc ? generic_launch_v<true, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s)
              : generic_launch_v<false, QBP_GENERIC_MEM>(variant, G, grid, threads, lds, s);
}
#endif

#if QBP_GENERIC_MEM == 0 && !defined(QBP_COLS_TU) && !defined(QBP_BUDGETS_TU) && !defined(QBP_SPECTRUM_TU) && \
    !defined(QBP_SHOTS_TU) && !defined(QBP_LLRHIST_TU)
hipError_t launch_generic_llrhist_mem0(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_llrhist_mem1(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_llrhist_mem2(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_shots_mem0(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_shots_mem1(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_shots_mem2(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_spectrum_mem0(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_spectrum_mem1(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_spectrum_mem2(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_mem1(bool, int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_mem2(bool, int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_cols_mem0(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_cols_mem1(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_cols_mem2(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_budgets_mem0(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_budgets_mem1(int, const GenericParams&, int, int, size_t, hipStream_t);
hipError_t launch_generic_budgets_mem2(int, const GenericParams&, int, int, size_t, hipStream_t);

hipError_t launch_generic(bool mc, int mem, int variant, const GenericParams& G, int grid, int threads,
                          size_t lds, hipStream_t s)
{
    static_assert(GENERIC_MEM_GLOBAL == 0 && GENERIC_MEM_LDS == 1 && GENERIC_MEM_SPLIT == 2, "mode numbering");
    if (mc && G.det_bits) {           // recorded shots (qbp_decode_shots)
        switch (mem) {
            case GENERIC_MEM_LDS:   return launch_generic_shots_mem1(variant, G, grid, threads, lds, s);
            case GENERIC_MEM_SPLIT: return launch_generic_shots_mem2(variant, G, grid, threads, lds, s);
            default:                return launch_generic_shots_mem0(variant, G, grid, threads, lds, s);
        }
    }
    if (mc && G.llr_hist) {           // posterior-LLR histograms per iteration budget (qbp_mc_run_llr_hist)
        switch (mem) {
            case GENERIC_MEM_LDS:   return launch_generic_llrhist_mem1(variant, G, grid, threads, lds, s);
            case GENERIC_MEM_SPLIT: return launch_generic_llrhist_mem2(variant, G, grid, threads, lds, s);
            default:                return launch_generic_llrhist_mem0(variant, G, grid, threads, lds, s);
        }
    }
    if (mc && G.spectrum) {           // residual-weight and iteration tables (qbp_mc_run_spectrum)
        switch (mem) {
            case GENERIC_MEM_LDS:   return launch_generic_spectrum_mem1(variant, G, grid, threads, lds, s);
            case GENERIC_MEM_SPLIT: return launch_generic_spectrum_mem2(variant, G, grid, threads, lds, s);
            default:                return launch_generic_spectrum_mem0(variant, G, grid, threads, lds, s);
        }
    }
    if (mc && G.n_budgets) {          // a ladder of iteration budgets (qbp_mc_run_budgets)
        switch (mem) {
            case GENERIC_MEM_LDS:   return launch_generic_budgets_mem1(variant, G, grid, threads, lds, s);
            case GENERIC_MEM_SPLIT: return launch_generic_budgets_mem2(variant, G, grid, threads, lds, s);
            default:                return launch_generic_budgets_mem0(variant, G, grid, threads, lds, s);
        }
    }
    if (mc && G.thr_cols) {           // a sampler threshold per qubit (qbp_mc_run_probs)
        switch (mem) {
            case GENERIC_MEM_LDS:   return launch_generic_cols_mem1(variant, G, grid, threads, lds, s);
            case GENERIC_MEM_SPLIT: return launch_generic_cols_mem2(variant, G, grid, threads, lds, s);
            default:                return launch_generic_cols_mem0(variant, G, grid, threads, lds, s);
        }
    }
    switch (mem) {
        case GENERIC_MEM_LDS:   return launch_generic_mem1(mc, variant, G, grid, threads, lds, s);
        case GENERIC_MEM_SPLIT: return launch_generic_mem2(mc, variant, G, grid, threads, lds, s);
        default:                return launch_generic_mem0(mc, variant, G, grid, threads, lds, s);
    }
}

hipError_t launch_permute_prior(const double* prior, const int32_t* svar, double* out, int n, hipStream_t s)
{
    hipLaunchKernelGGL(generic_permute_prior, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, prior, svar, out, n);
    return hipGetLastError();
}
#endif

}  // namespace qbp
