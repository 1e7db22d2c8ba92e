// np.histogram's bin rule on the device, stated once: for hist_bin_kernel (qbp_hist.hpp: the alpha-fit message
// histograms) and for the posterior-LLR histograms of the Monte-Carlo kernels (qbp_mc_run_llr_hist: the
// -DQBP_LLRHIST_TU builds of qbp_kernels.hpp and qbp_generic.hpp).
//
// Edges are np.linspace(lo, hi, bins + 1), computed on the host the way numpy does (start + i * step, last edge = hi)
// and held in LDS by the caller.  A value's bin is the one whose edges contain it -- left-closed, the last bin closed on
// both sides -- which is numpy's own rule after its rounding corrections: an estimate from the uniform width, then
// corrected against the edges themselves.
#pragma once

#include <hip/hip_runtime.h>

namespace qbp {

// Bin 0 .. bins - 1 of a value v with le[0] <= v <= le[bins].  norm = bins / (le[bins] - le[0]): it only seeds the
// search, so how it was rounded does not matter.
__device__ __forceinline__ int hist_bin_of(double v, const double* le, int bins, double first, double norm)
{
    int k = (int)((v - first) * norm);
    k = k < 0 ? 0 : (k > bins - 1 ? bins - 1 : k);
    while (k > 0 && v < le[k]) --k;                 // the estimate can be one off next to an edge
    while (k < bins - 1 && v >= le[k + 1]) ++k;
    return k;
}

// Column of v in a row of bins + 3 counts (include/qbp.h, qbp_mc_run_llr_hist): 0 below the range (-inf included),
// 1 .. bins the bins, bins + 1 above the range (+inf included), bins + 2 NaN.  le: [bins + 1] edges, then norm.
__device__ __forceinline__ int llr_hist_col(double v, const double* le, int bins)
{
    const double first = le[0], last = le[bins];
    if (v != v) return bins + 2;
    if (v < first) return 0;
    if (v > last) return bins + 1;
    return 1 + hist_bin_of(v, le, bins, first, le[bins + 1]);
}

}  // namespace qbp
