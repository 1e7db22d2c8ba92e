// Host-side launch interface between the API translation unit (qbp.hip) and the kernel translation
// units (qbp_tu_*.hip).  Each kernel family is compiled in its own translation unit so that the
// library builds in parallel (make -j) and a change to one kernel recompiles only its family; the
// API unit sees parameter structs and these prototypes, never a kernel instantiation.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace qbp {

struct FusedParams;
struct GenericParams;
struct StreamParams;
struct OsdParams;
struct OsdBigWorkspace;
struct OsdOrderBigArgs;
struct RelayParams;
struct LayeredParams;
struct QuantParams;
struct GdParams;
struct CondParams;
struct CssClassify;
struct LsdParams;
struct LsdLargeWorkspace;
struct WindowCommit;
struct DistParams;
struct FrameParams;

// (row weight, column weight) shapes the on-chip kernel is instantiated for: every code of the
// reference's codes/ is (6, 3); (8, 4) covers their space-time matrices (spaceTime.py: row weight
// 6 + 2, column weight 3).  Anything wider, or with m > 1024, goes to the general-H kernel.
// Threads per workgroup of the on-chip kernel = its register budget: 1024 threads are 4 wavefronts per SIMD
// at <= 128 registers, 768 are 3 at <= 168 (build-time, A/B: tools/build_variants.sh).
#ifndef QBP_FUSED_MAX_THREADS
#define QBP_FUSED_MAX_THREADS 1024
#endif
constexpr int FUSED_MAX_THREADS = QBP_FUSED_MAX_THREADS;
constexpr int DC_SMALL = 6, DV_SMALL = 3;
constexpr int DC_WIDE = 8, DV_WIDE = 4;

struct LaunchCfg {
    int S, threads, lds_bytes, grid, slot_stride, dc;
    int one_barrier;        // forced-iteration decode launch with two copies of R in LDS (qbp_kernels.hpp)
    int r0_table;           // early-exit launch with the first check step's messages tabulated in LDS
};

// Before a launch with `lds` bytes of dynamic LDS: raise the kernel's hipFuncAttributeMaxDynamicSharedMemorySize to it,
// once per device and size.  lds_set: the largest size set so far on every device, one table per kernel.
inline hipError_t raise_dynamic_lds(const void* kernel, size_t lds, size_t (&lds_set)[64])
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds > 0 && (dev < 0 || dev >= 64 || lds_set[dev] < lds)) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) lds_set[dev] = lds;
    }
    return hipSuccess;
}

// One launch of KERNEL with `lds` bytes of dynamic LDS: the attribute as above, the launch, hipGetLastError().  The
// kernel is a template argument so that every instantiation has a table of its own.  (`lds > 0` above sets the
// attribute no earlier or later than a plain `lds_set[dev] < lds` would: no size is below the zeros the table starts
// with, so a launch without dynamic LDS never set it.)
template <auto KERNEL, class... Args>
hipError_t launch_dynamic_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args)
{
    static thread_local size_t lds_set[64] = {0};
    const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(KERNEL), lds, lds_set);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
    return hipGetLastError();
}

// qbp_tu_fused.hip
hipError_t launch_fused(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
hipError_t launch_fused_fast_math(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
// the same with a sampler threshold per qubit (P.thr_cols; Monte-Carlo only): qbp_tu_fused.hip -DQBP_COLS_TU
hipError_t launch_fused_cols(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
hipError_t launch_fused_cols_fast_math(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg,
                                       hipStream_t s);
// the same again, checkpointing at a ladder of iteration budgets (P.budgets; qbp_mc_run_budgets): -DQBP_BUDGETS_TU
hipError_t launch_fused_budgets(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
hipError_t launch_fused_budgets_fast_math(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg,
                                          hipStream_t s);
// the same again, adding residual weights and iteration indices to tables (P.spectrum; qbp_mc_run_spectrum):
// -DQBP_SPECTRUM_TU
hipError_t launch_fused_spectrum(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
hipError_t launch_fused_spectrum_fast_math(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg,
                                           hipStream_t s);
// the same again, decoding recorded shots (P.det_bits; qbp_decode_shots): -DQBP_SHOTS_TU
hipError_t launch_fused_shots(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
hipError_t launch_fused_shots_fast_math(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg,
                                        hipStream_t s);
// budgets builds that also bin the posterior LLRs of every emission (P.llr_hist; qbp_mc_run_llr_hist): -DQBP_LLRHIST_TU
hipError_t launch_fused_llrhist(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg, hipStream_t s);
hipError_t launch_fused_llrhist_fast_math(bool mc, int variant, const FusedParams& P, const LaunchCfg& cfg,
                                          hipStream_t s);
hipError_t launch_debug_math(int kind, const double* x, double* y, long long count, hipStream_t s);
hipError_t launch_mc_sample(uint8_t* errors, int n, long long T, long long trial_begin, int draws,
                            unsigned long long seed, unsigned threshold, hipStream_t s);
// thr: [n rounded up to 4] thresholds, one per qubit (qbp_mc.hpp, mc_error_quad_cols)
hipError_t launch_mc_sample_cols(uint8_t* errors, int n, long long T, long long trial_begin, int draws,
                                 unsigned long long seed, const uint32_t* thr, hipStream_t s);
// rows of exactly `weight` ones (mc_sample_weight_kernel; 0 <= weight <= n); clears errors [T][n] first, on s
hipError_t launch_mc_sample_weight(uint8_t* errors, int n, int weight, long long T, long long trial_begin,
                                   unsigned long long seed, hipStream_t s);
// row b = the columns of `weight` faults at distinct sites (mc_sample_fault_weight_kernel; 0 <= weight <= n_sites); the
// three tables are those of qbp_fault_table_set; picks [weight][stride] is workspace, stride >= 1 trials per launch;
// clears errors [T][n] first, on s
hipError_t launch_mc_sample_fault_weight(uint8_t* errors, int n, int weight, long long T, long long trial_begin,
                                         unsigned long long seed, const long long* first_fault, const uint8_t* site_k,
                                         const int32_t* fault_column, unsigned n_sites, uint32_t* picks,
                                         long long stride, hipStream_t s);
// row b = the weight-`weight` pattern of rank rank_begin + b (mc_enum_weight_kernel; 0 <= weight <= n); binom
// [weight + 1][n + 1]: C(j, t) at t * (n + 1) + j, saturated; clears errors [T][n] first, on s
hipError_t launch_mc_enum_weight(uint8_t* errors, int n, int weight, long long T, long long rank_begin,
                                 const unsigned long long* binom, hipStream_t s);
// qbp_enum_failures: the b8 syndrome row and the Lx word of every error row; the capture behind the shots launches
hipError_t launch_enum_pack(const uint8_t* errors, long long T, int m, int n, const int32_t* row_ptr,
                            const int32_t* col_idx, const unsigned long long* lx_cols, uint8_t* det_bits,
                            unsigned long long* actual, hipStream_t s);
hipError_t launch_enum_capture(const unsigned long long* predictions, const unsigned long long* actual,
                               const uint8_t* converged, long long T, long long rank_begin, int what, long long cap,
                               long long* ranks, uint8_t* kinds, unsigned long long* found, hipStream_t s);
// qbp_tu_generic.hip (Monte-Carlo launches with G.det_bits go to the -DQBP_SHOTS_TU builds, with G.llr_hist to the
// -DQBP_LLRHIST_TU builds, with G.spectrum to the
// -DQBP_SPECTRUM_TU builds, with G.n_budgets to the
// -DQBP_BUDGETS_TU builds, others with G.thr_cols to the -DQBP_COLS_TU builds)
hipError_t launch_generic(bool mc, int mem, int variant, const GenericParams& G, int grid, int threads,
                          size_t lds, hipStream_t s);
hipError_t launch_permute_prior(const double* prior, const int32_t* svar, double* out, int n, hipStream_t s);
// qbp_tu_stream.hip
hipError_t launch_stream(int variant, unsigned grid, const StreamParams& P, const int32_t* col_idx,
                         const int32_t* col_ptr, const int32_t* col_edge, const double* prior,
                         const int32_t* srow, const int32_t* srow_e0, const int32_t* srow_deg,
                         const int32_t* svar, const int32_t* sedge, hipStream_t s);
// qbp_tu_osd.hip
hipError_t launch_osd_small(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, hipStream_t s);
// method: OSD_METHOD_CS / OSD_METHOD_E (qbp_osd_order.hpp), order >= 1
hipError_t launch_osd_order(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, int method, int order,
                            hipStream_t s);
hipError_t launch_osd_big(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk, hipStream_t s);
hipError_t launch_osd_blocked(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                              const OsdBigWorkspace& Wk, hipStream_t s);
// the same four with O.spectrum set (qbp_mc_run_spectrum): qbp_tu_osd.hip -DQBP_SPECTRUM_TU, kernels under names of
// their own that also add the residual weight of every record to rows 1 / 3 of the table
hipError_t launch_osd_small_spectrum(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, hipStream_t s);
hipError_t launch_osd_order_spectrum(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, int method,
                                     int order, hipStream_t s);
hipError_t launch_osd_big_spectrum(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk,
                                   hipStream_t s);
hipError_t launch_osd_blocked_spectrum(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                       const OsdBigWorkspace& Wk, hipStream_t s);
// the same four with O.shots set (qbp_decode_shots): qbp_tu_osd.hip -DQBP_SHOTS_TU, kernels under names of their own
// that store and check the observable prediction of every record
hipError_t launch_osd_small_shots(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, hipStream_t s);
hipError_t launch_osd_order_shots(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, int method,
                                  int order, hipStream_t s);
hipError_t launch_osd_big_shots(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk, hipStream_t s);
hipError_t launch_osd_blocked_shots(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                    const OsdBigWorkspace& Wk, hipStream_t s);
// the same four with O.order set (qbp_osd_batch_ordered): qbp_tu_osd.hip -DQBP_ORDERED_TU, kernels under names of their
// own
hipError_t launch_osd_small_ordered(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, hipStream_t s);
hipError_t launch_osd_order_ordered(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, int method,
                                    int order, hipStream_t s);
hipError_t launch_osd_big_ordered(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk,
                                  hipStream_t s);
hipError_t launch_osd_blocked_ordered(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                      const OsdBigWorkspace& Wk, hipStream_t s);
// order w on the matrices the blocked kernel serves (qbp_osd_order_big.hpp, QBP_FLAG_OSD_LARGE): one per build of
// qbp_tu_osd.hip
hipError_t launch_osd_order_blocked(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                    const OsdBigWorkspace& Wk, const OsdOrderBigArgs& X, hipStream_t s);
hipError_t launch_osd_order_blocked_spectrum(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                             const OsdBigWorkspace& Wk, const OsdOrderBigArgs& X, hipStream_t s);
hipError_t launch_osd_order_blocked_shots(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                          const OsdBigWorkspace& Wk, const OsdOrderBigArgs& X, hipStream_t s);
hipError_t launch_osd_order_blocked_ordered(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                            const OsdBigWorkspace& Wk, const OsdOrderBigArgs& X, hipStream_t s);
// qbp_tu_relay.hip: bp_relay_kernel<records, large>: messages in LDS or (large) in a global workspace, the batch build
// or (records) the build that reads Monte-Carlo failure records
hipError_t launch_relay(bool records, bool large, const RelayParams& P, int grid, int threads, size_t lds,
                        hipStream_t s);
// qbp_tu_layered.hip: bp_layered_kernel<variant, mc, large> (sum-product or min-sum; batch or Monte-Carlo build; the
// messages in LDS or (large) in a global workspace)
hipError_t launch_layered(bool mc, bool large, int variant, const LayeredParams& P, int grid, size_t lds,
                          hipStream_t s);
// qbp_tu_quant.hip: bp_quant_kernel<message type, mc> (int8 messages for q <= 8, else int16; batch or Monte-Carlo build)
hipError_t launch_quant(bool mc, bool wide, const QuantParams& P, int grid, size_t lds, hipStream_t s);
// qbp_tu_gd.hip: bp_gd_kernel<variant, records, large> (sum-product or min-sum; batch build or Monte-Carlo failure
// records; the messages in LDS or (large) in a global workspace)
hipError_t launch_gd(bool records, bool large, int variant, const GdParams& P, int grid, int threads, size_t lds,
                     hipStream_t s);
// qbp_tu_cond.hip: bp_cond_kernel<variant> (sum-product or min-sum; a prior per record), and the glue kernels of the
// two-stage CSS decoder (qbp_cond.hpp): t1 <= t2 <= t3 are the sampler's cumulative thresholds (Z, X, Y)
hipError_t launch_cond(int variant, const CondParams& P, int grid, int threads, size_t lds, hipStream_t s);
hipError_t launch_css_sample_pauli(uint8_t* e_a, uint8_t* e_b, int n, long long T, long long trial_begin,
                                   unsigned long long seed, unsigned t1, unsigned t2, unsigned t3, hipStream_t s);
hipError_t launch_css_select(const uint8_t* hard, const uint8_t* sol, const uint8_t* conv, long long T, int n, uint8_t* x,
                             hipStream_t s);
hipError_t launch_css_classify(const CssClassify& P, hipStream_t s);
// qbp_tu_lsd.hip: lsd_kernel<records> (batch build or Monte-Carlo failure records), one wavefront per record
hipError_t launch_lsd(bool records, const LsdParams& P, unsigned grid, size_t lds, hipStream_t s);
// lsd_large_kernel<records> (qbp_lsd_large.hpp): one workgroup of 256 threads per record, the rows in the workspace
hipError_t launch_lsd_large(bool records, const LsdParams& P, const LsdLargeWorkspace& Wk, unsigned grid, size_t lds,
                            hipStream_t s);
// qbp_tu_distance.hip: dist_search_kernel<capture> (qbp_distance.hpp), one wavefront per trial; capture: the launch
// that repeats the call's best trial and stores its row
hipError_t launch_dist_search(bool capture, const DistParams& P, unsigned grid, size_t lds, hipStream_t s);
// qbp_tu_frame.hip: frame_sim_kernel<sample> (qbp_frame.hpp), one lane per 32 records of the chunk P.W lanes wide, and
// frame_assemble_kernel, which turns the chunk's measurement records into detector rows and observable masks
hipError_t launch_frame_sim(bool sample, const FrameParams& P, hipStream_t s);
hipError_t launch_frame_assemble(const FrameParams& P, unsigned grid, hipStream_t s);
// qbp_tu_window.hip: the glue kernels of sliding-window decoding (qbp_window.hpp)
hipError_t launch_window_gather(const uint8_t* r, long long B, int m, const int32_t* checks, int mk, uint8_t* syn,
                                hipStream_t s);
hipError_t launch_window_gather_prior(const double* prior, const int32_t* vars, int total, double* out, hipStream_t s);
hipError_t launch_window_fail_list(const uint8_t* conv, long long B, long long* list, unsigned long long* count,
                                   hipStream_t s);
// final_pass: converged [B] from the running syndrome, after the last window's commit
hipError_t launch_window_commit(const WindowCommit& P, bool final_pass, hipStream_t s);
hipError_t launch_window_syndrome(const uint8_t* errors, long long T, int m, int n, const int32_t* row_ptr,
                                  const int32_t* col_idx, uint8_t* syn, hipStream_t s);
hipError_t launch_window_classify(const uint8_t* errors, const uint8_t* x, const uint8_t* valid, const int32_t* iters,
                                  const int32_t* fails, long long T, int n, const unsigned long long* lx_cols,
                                  int half_distance, long long* counters, hipStream_t s);
hipError_t launch_hist_minmax(int grid, const double* x, long long count, double* part, hipStream_t s);
hipError_t launch_hist_bin(int grid, size_t lds, const double* msg, const uint8_t* errors, const int32_t* col_idx,
                           long long B, int E, int n, const double* edges, int bins, unsigned long long* hist,
                           hipStream_t s);

}  // namespace qbp
