// libqbp.so, translation unit of the OSD kernels (qbp_osd.hpp: OSD-0, qbp_osd_order.hpp and qbp_osd_order_big.hpp:
// order w) and the
// histogram kernels (qbp_hist.hpp).
// With -DQBP_SPECTRUM_TU: the OSD kernels that classify once more, under other names, adding the residual weight
// of every record to a table (qbp_mc_run_spectrum); no histogram kernels in that unit.
// With -DQBP_SHOTS_TU: all of them once more, whose records are recorded shots: they store the observable prediction of
// every record and compare it with the recorded observables (qbp_decode_shots); no histogram kernels either.
// With -DQBP_ORDERED_TU: all of them once more, which take the column order of every record from the caller instead of
// sorting (qbp_osd_batch_ordered); no histogram kernels either.
#define QBP_DEFINE_KERNELS 1
#if defined(QBP_ORDERED_TU)
#define QBP_OSD_ORDERED 1
#define QBP_OSD_TU_SUFFIX _ordered
#elif defined(QBP_SHOTS_TU)
#define QBP_OSD_SHOTS 1
#define QBP_OSD_TU_SUFFIX _shots
#elif defined(QBP_SPECTRUM_TU)
#define QBP_OSD_SPECTRUM 1
#define QBP_OSD_TU_SUFFIX _spectrum
#endif
#ifdef QBP_OSD_TU_SUFFIX
// the unit's kernels and launch functions under names of their own: <stem><suffix>_kernel, launch_<...><suffix>
#undef QBP_OSD_TIMING
#define QBP_OSD_CAT_(a, b, c) a##b##c
#define QBP_OSD_CAT(a, b, c) QBP_OSD_CAT_(a, b, c)
#define QBP_OSD_KERNEL(stem) QBP_OSD_CAT(stem, QBP_OSD_TU_SUFFIX, _kernel)
#define QBP_OSD_LAUNCH(name) QBP_OSD_CAT(name, QBP_OSD_TU_SUFFIX, )
#define osd0_kernel QBP_OSD_KERNEL(osd0)
#define osd0_big_kernel QBP_OSD_KERNEL(osd0_big)
#define osd0_blocked_kernel QBP_OSD_KERNEL(osd0_blocked)
#define osd_order_kernel QBP_OSD_KERNEL(osd_order)
#define osd_order_blocked_kernel QBP_OSD_KERNEL(osd_order_blocked)
#define launch_osd_small QBP_OSD_LAUNCH(launch_osd_small)
#define launch_osd_order QBP_OSD_LAUNCH(launch_osd_order)
#define launch_osd_big QBP_OSD_LAUNCH(launch_osd_big)
#define launch_osd_blocked QBP_OSD_LAUNCH(launch_osd_blocked)
#define launch_osd_order_blocked QBP_OSD_LAUNCH(launch_osd_order_blocked)
#endif
#include <hip/hip_runtime.h>

#include "../../include/qbp.h"
#ifndef QBP_OSD_TU_SUFFIX
#include "qbp_hist.hpp"
#endif
#include "qbp_launch.hpp"
#include "qbp_osd.hpp"
#include "qbp_osd_order.hpp"
#include "qbp_osd_order_big.hpp"

namespace qbp {

hipError_t launch_osd_small(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, hipStream_t s)
{
    // row width (32-bit words incl. the syndrome word) as a template argument for the codes of the
    // reference: n = 72 / 90 / 108 -> 4 or 5, 144 -> 6, 288 -> 10
    switch (words_per_row) {
#define QBP_OSD_CASE(WW) case WW: hipLaunchKernelGGL(osd0_kernel<WW>, dim3(grid), dim3(64), lds, s, O); break
        QBP_OSD_CASE(2); QBP_OSD_CASE(3); QBP_OSD_CASE(4); QBP_OSD_CASE(5); QBP_OSD_CASE(6);
        QBP_OSD_CASE(7); QBP_OSD_CASE(8); QBP_OSD_CASE(9); QBP_OSD_CASE(10); QBP_OSD_CASE(11);
#undef QBP_OSD_CASE
        default: hipLaunchKernelGGL(osd0_kernel<0>, dim3(grid), dim3(64), lds, s, O);
    }
    return hipGetLastError();
}

hipError_t launch_osd_order(int words_per_row, unsigned grid, size_t lds, const OsdParams& O, int method, int order,
                            hipStream_t s)
{
    switch (words_per_row) {
#define QBP_OSD_CASE(WW) \
    case WW: hipLaunchKernelGGL(osd_order_kernel<WW>, dim3(grid), dim3(64), lds, s, O, method, order); break
        QBP_OSD_CASE(2); QBP_OSD_CASE(3); QBP_OSD_CASE(4); QBP_OSD_CASE(5); QBP_OSD_CASE(6);
        QBP_OSD_CASE(7); QBP_OSD_CASE(8); QBP_OSD_CASE(9); QBP_OSD_CASE(10); QBP_OSD_CASE(11);
#undef QBP_OSD_CASE
        default: hipLaunchKernelGGL(osd_order_kernel<0>, dim3(grid), dim3(64), lds, s, O, method, order);
    }
    return hipGetLastError();
}

hipError_t launch_osd_big(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk, hipStream_t s)
{
    return launch_dynamic_lds<osd0_big_kernel>(dim3(grid), dim3(256), lds, s, O, Wk);
}

template <int RPT>
static hipError_t launch_osd_blocked_rpt(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk,
                                         hipStream_t s)
{
    return launch_dynamic_lds<osd0_blocked_kernel<RPT>>(dim3(grid), dim3(1024), lds, s, O, Wk);
}

// rows per thread: m <= 1024 * rows_per_thread (1, 2, 4 or 8)
hipError_t launch_osd_blocked(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                              const OsdBigWorkspace& Wk, hipStream_t s)
{
    switch (rows_per_thread) {
        case 1: return launch_osd_blocked_rpt<1>(grid, lds, O, Wk, s);
        case 2: return launch_osd_blocked_rpt<2>(grid, lds, O, Wk, s);
        case 4: return launch_osd_blocked_rpt<4>(grid, lds, O, Wk, s);
        case 8: return launch_osd_blocked_rpt<8>(grid, lds, O, Wk, s);
        default: return hipErrorInvalidValue;
    }
}

template <int RPT>
static hipError_t launch_osd_order_blocked_rpt(unsigned grid, size_t lds, const OsdParams& O, const OsdBigWorkspace& Wk,
                                               const OsdOrderBigArgs& X, hipStream_t s)
{
    return launch_dynamic_lds<osd_order_blocked_kernel<RPT>>(dim3(grid), dim3(1024), lds, s, O, Wk, X);
}

// order w on the blocked kernel's matrices; rows per thread as launch_osd_blocked
hipError_t launch_osd_order_blocked(int rows_per_thread, unsigned grid, size_t lds, const OsdParams& O,
                                    const OsdBigWorkspace& Wk, const OsdOrderBigArgs& X, hipStream_t s)
{
    switch (rows_per_thread) {
        case 1: return launch_osd_order_blocked_rpt<1>(grid, lds, O, Wk, X, s);
        case 2: return launch_osd_order_blocked_rpt<2>(grid, lds, O, Wk, X, s);
        case 4: return launch_osd_order_blocked_rpt<4>(grid, lds, O, Wk, X, s);
        case 8: return launch_osd_order_blocked_rpt<8>(grid, lds, O, Wk, X, s);
        default: return hipErrorInvalidValue;
    }
}

#ifdef QBP_OSD_TIMING
extern "C" int qbp_debug_osd_timing(unsigned long long* out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_osd_timing), 8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out + 8, HIP_SYMBOL(g_osd_stat), 8 * sizeof(unsigned long long));
    if (e == hipSuccess && reset) {
        unsigned long long z[8] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_osd_timing), z, sizeof(z));
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_osd_stat), z, sizeof(z));
    }
    return (int)e;
}
#endif

#ifndef QBP_OSD_TU_SUFFIX
hipError_t launch_hist_minmax(int grid, const double* x, long long count, double* part, hipStream_t s)
{
    hipLaunchKernelGGL(hist_minmax_kernel, dim3(grid), dim3(256), 0, s, x, count, part);
    return hipGetLastError();
}

hipError_t launch_hist_bin(int grid, size_t lds, const double* msg, const uint8_t* errors, const int32_t* col_idx,
                           long long B, int E, int n, const double* edges, int bins, unsigned long long* hist,
                           hipStream_t s)
{
    hipLaunchKernelGGL(hist_bin_kernel, dim3(grid), dim3(256), lds, s, msg, errors, col_idx, B, E, n, edges, bins, hist);
    return hipGetLastError();
}
#endif  // !QBP_OSD_TU_SUFFIX

}  // namespace qbp
