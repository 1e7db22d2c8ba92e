// libqbp.so, translation unit of the on-chip kernel (qbp_kernels.hpp): its 27 instantiations.
// Compiled twice: as is (numpy's tanh / arctanh: the default), and with -DQBP_FAST_TU -DQBP_MATH_FAST=1 under
// other names (QBP_FLAG_FAST_MATH: round 2's approximations); each build is a code object of its own.
// Both again with -DQBP_COLS_TU: the 12 Monte-Carlo instantiations with a sampler threshold per qubit
// (qbp_mc_run_probs), under other names again; and those 12 once more with -DQBP_BUDGETS_TU: the builds that checkpoint a
// running trial at a ladder of iteration budgets (qbp_mc_run_budgets; per-qubit thresholds always); and once more with
// -DQBP_SPECTRUM_TU: the builds that add residual weights and iteration indices to tables (qbp_mc_run_spectrum; per-qubit
// thresholds or stored errors); and once more with -DQBP_SHOTS_TU: the builds that decode recorded shots
// (qbp_decode_shots: detection events read from memory, observable predictions written); and once more with
// -DQBP_LLRHIST_TU: budgets builds that also bin the posterior LLRs of every emission (qbp_mc_run_llr_hist; per-qubit
// thresholds or stored errors).
#if defined(QBP_LLRHIST_TU)
#define QBP_MC_COLS 1
#define QBP_MC_BUDGETS 1
#define QBP_MC_LLRHIST 1
#ifdef QBP_FAST_TU
#define bp_fused_kernel bp_fused_llrhist_kernel_fast_math
#define launch_fused launch_fused_llrhist_fast_math
#else
#define bp_fused_kernel bp_fused_llrhist_kernel
#define launch_fused launch_fused_llrhist
#endif
#elif defined(QBP_SHOTS_TU)
#define QBP_MC_SHOTS 1
#ifdef QBP_FAST_TU
#define bp_fused_kernel bp_fused_shots_kernel_fast_math
#define launch_fused launch_fused_shots_fast_math
#else
#define bp_fused_kernel bp_fused_shots_kernel
#define launch_fused launch_fused_shots
#endif
#elif defined(QBP_SPECTRUM_TU)
#define QBP_MC_COLS 1
#define QBP_MC_SPECTRUM 1
#ifdef QBP_FAST_TU
#define bp_fused_kernel bp_fused_spectrum_kernel_fast_math
#define launch_fused launch_fused_spectrum_fast_math
#else
#define bp_fused_kernel bp_fused_spectrum_kernel
#define launch_fused launch_fused_spectrum
#endif
#elif defined(QBP_BUDGETS_TU)
#define QBP_MC_COLS 1
#define QBP_MC_BUDGETS 1
#ifdef QBP_FAST_TU
#define bp_fused_kernel bp_fused_budgets_kernel_fast_math
#define launch_fused launch_fused_budgets_fast_math
#else
#define bp_fused_kernel bp_fused_budgets_kernel
#define launch_fused launch_fused_budgets
#endif
#elif defined(QBP_COLS_TU)
#define QBP_MC_COLS 1
#ifdef QBP_FAST_TU
#define bp_fused_kernel bp_fused_cols_kernel_fast_math
#define launch_fused launch_fused_cols_fast_math
#else
#define bp_fused_kernel bp_fused_cols_kernel
#define launch_fused launch_fused_cols
#endif
#elif defined(QBP_FAST_TU)
#define bp_fused_kernel bp_fused_kernel_fast_math
#define launch_fused launch_fused_fast_math
#else
#define QBP_DEFINE_KERNELS 1
#endif
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#include "qbp_kernels.hpp"
#include "qbp_launch.hpp"

namespace qbp {
namespace {

template <int DC, int DV, int VARIANT, bool MC, bool FORCE, int MAXT, int MINW, bool ONEBAR = false>
hipError_t launch_k(const FusedParams& P, const LaunchCfg& cfg, hipStream_t stream)
{
    // the dynamic-LDS limit of an instantiation is raised once per device and size (the attribute
    // call costs a few microseconds, which matters for one-syndrome-per-call users)
    return launch_dynamic_lds<bp_fused_kernel<DC, DV, VARIANT, MC, FORCE, MAXT, MINW, ONEBAR>>(
        dim3(cfg.grid), dim3(cfg.threads), (size_t)cfg.lds_bytes, stream, P);
}

template <int VARIANT, bool MC, int MAXT, int MINW = 1>
hipError_t launch_one(const FusedParams& P, const LaunchCfg& cfg, hipStream_t stream)
{
    const bool force = (P.flags & QBP_FLAG_FORCE_FULL) != 0;
    if constexpr (!MC) {      // (the wide shape is 1.5 % slower with one barrier -- more spills -- and keeps two)
        if (force && cfg.one_barrier && cfg.dc == DC_SMALL)
            return launch_k<DC_SMALL, DV_SMALL, VARIANT, false, true, MAXT, MINW, true>(P, cfg, stream);
    }
    if (cfg.dc == DC_SMALL)
        return force ? launch_k<DC_SMALL, DV_SMALL, VARIANT, MC, true, MAXT, MINW>(P, cfg, stream)
                     : launch_k<DC_SMALL, DV_SMALL, VARIANT, MC, false, MAXT, MINW>(P, cfg, stream);
    return force ? launch_k<DC_WIDE, DV_WIDE, VARIANT, MC, true, MAXT, MINW>(P, cfg, stream)
                 : launch_k<DC_WIDE, DV_WIDE, VARIANT, MC, false, MAXT, MINW>(P, cfg, stream);
}

template <bool MC>
hipError_t launch_variant(int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s)
{
    // __launch_bounds__(1024): 128-VGPR budget = 4 wavefronts per SIMD, the fastest geometry
    // measured (profiles/r01_tune.txt; builds with 3 or 5 waves per SIMD were slower).
    switch (variant) {
        case QBP_SUM_PRODUCT: return launch_one<0, MC, FUSED_MAX_THREADS>(P, cfg, s);
        case QBP_DAMPED_SP:   return launch_one<1, MC, FUSED_MAX_THREADS>(P, cfg, s);
        default:              return launch_one<2, MC, FUSED_MAX_THREADS>(P, cfg, s);
    }
}

}  // namespace

hipError_t launch_fused(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s)
{
#if defined(QBP_COLS_TU) || defined(QBP_BUDGETS_TU) || defined(QBP_SPECTRUM_TU) || defined(QBP_SHOTS_TU) || \
    defined(QBP_LLRHIST_TU)
    if (!mc) return hipErrorInvalidValue;       // (Monte-Carlo builds only)
    return launch_variant<true>(variant, P, cfg, s);
#else
    return mc ? launch_variant<true>(variant, P, cfg, s) : launch_variant<false>(variant, P, cfg, s);
#endif
}

#ifdef QBP_DEFINE_KERNELS
hipError_t launch_debug_math(int kind, const double* x, double* y, long long count, hipStream_t s)
{
    const int threads = 256;
    const long long blocks = (count + threads - 1) / threads;
    hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)blocks), dim3(threads), 0, s, kind, x, y, count);
    return hipGetLastError();
}

hipError_t launch_mc_sample(uint8_t* errors, int n, long long T, long long trial_begin, int draws,
                            unsigned long long seed, unsigned threshold, hipStream_t s)
{
    const long long items = T * ((n + 3) / 4);
    const int threads = 256;
    hipLaunchKernelGGL(mc_sample_kernel, dim3((unsigned)((items + threads - 1) / threads)), dim3(threads), 0, s,
                       errors, n, T, trial_begin, draws, seed, threshold);
    return hipGetLastError();
}

hipError_t launch_mc_sample_cols(uint8_t* errors, int n, long long T, long long trial_begin, int draws,
                                 unsigned long long seed, const uint32_t* thr, hipStream_t s)
{
    const long long items = T * ((n + 3) / 4);
    const int threads = 256;
    hipLaunchKernelGGL(mc_sample_cols_kernel, dim3((unsigned)((items + threads - 1) / threads)), dim3(threads), 0, s,
                       errors, n, T, trial_begin, draws, seed, thr);
    return hipGetLastError();
}

hipError_t launch_mc_sample_weight(uint8_t* errors, int n, int weight, long long T, long long trial_begin,
                                   unsigned long long seed, hipStream_t s)
{
    // the rows are the kernel's membership map and the buffer is reused across chunks and calls: whatever an
    // earlier launch left in it would come out as extra ones
    hipError_t e = hipMemsetAsync(errors, 0, (size_t)T * (size_t)n, s);
    if (e != hipSuccess || weight == 0) return e;
    const int threads = 256;
    hipLaunchKernelGGL(mc_sample_weight_kernel, dim3((unsigned)((T + threads - 1) / threads)), dim3(threads), 0, s,
                       errors, n, weight, T, trial_begin, seed);
    return hipGetLastError();
}

static_assert(QBP_FAULT_PHILOX_STREAM == FAULT_PHILOX_WORD3, "Philox counter word 3 of the fixed-weight fault sampler");

hipError_t launch_mc_sample_fault_weight(uint8_t* errors, int n, int weight, long long T, long long trial_begin,
                                         unsigned long long seed, const long long* first_fault, const uint8_t* site_k,
                                         const int32_t* fault_column, unsigned n_sites, uint32_t* picks,
                                         long long stride, hipStream_t s)
{
    // (the buffer is the weight sampler's, and a row is toggled, not set: cleared for the same reason)
    hipError_t e = hipMemsetAsync(errors, 0, (size_t)T * (size_t)n, s);
    if (e != hipSuccess || weight == 0) return e;
    const int threads = 256;
    // picks holds the sites of `stride` trials: the launches of one call follow each other on s and share it
    for (long long a = 0; a < T; a += stride) {
        const long long t = T - a < stride ? T - a : stride;
        hipLaunchKernelGGL(mc_sample_fault_weight_kernel, dim3((unsigned)((t + threads - 1) / threads)), dim3(threads), 0,
                           s, errors + (size_t)a * (size_t)n, n, weight, t, trial_begin + a, seed, first_fault, site_k,
                           fault_column, n_sites, picks, stride);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_mc_enum_weight(uint8_t* errors, int n, int weight, long long T, long long rank_begin,
                                 const unsigned long long* binom, hipStream_t s)
{
    // (the buffer is the weight sampler's: cleared for the same reason)
    hipError_t e = hipMemsetAsync(errors, 0, (size_t)T * (size_t)n, s);
    if (e != hipSuccess || weight == 0) return e;
    const int threads = 256;
    hipLaunchKernelGGL(mc_enum_weight_kernel, dim3((unsigned)((T + threads - 1) / threads)), dim3(threads), 0, s,
                       errors, n, weight, T, rank_begin, binom);
    return hipGetLastError();
}

hipError_t launch_enum_pack(const uint8_t* errors, long long T, int m, int n, const int32_t* row_ptr,
                            const int32_t* col_idx, const unsigned long long* lx_cols, uint8_t* det_bits,
                            unsigned long long* actual, hipStream_t s)
{
    const long long items = T * ((m + 7) / 8 + 1);
    const int threads = 256;
    hipLaunchKernelGGL(enum_pack_kernel, dim3((unsigned)((items + threads - 1) / threads)), dim3(threads), 0, s,
                       errors, T, m, n, row_ptr, col_idx, lx_cols, det_bits, actual);
    return hipGetLastError();
}

hipError_t launch_enum_capture(const unsigned long long* predictions, const unsigned long long* actual,
                               const uint8_t* converged, long long T, long long rank_begin, int what, long long cap,
                               long long* ranks, uint8_t* kinds, unsigned long long* found, hipStream_t s)
{
    const int threads = 256;
    hipLaunchKernelGGL(enum_capture_kernel, dim3((unsigned)((T + threads - 1) / threads)), dim3(threads), 0, s,
                       predictions, actual, converged, T, rank_begin, what, cap, ranks, kinds, found);
    return hipGetLastError();
}
#endif  // QBP_DEFINE_KERNELS

}  // namespace qbp
