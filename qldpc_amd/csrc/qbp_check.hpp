// The check update of one row, shared by the on-chip, general-H and streaming kernels
// (beliefPropagation.py:114-126 for sum-product, rework/decoding.py:28-56 for min-sum).
//
//   check_row      a row held in registers (rows of weight <= 8): every kernel family's per-row path
//   minsum_row / minsum_message / sp_message
//                  its pieces, also the row update of the two-pass paths of long rows (sequential row
//                  product / minimum search, then one message per edge)
//   damped_q       the damped variants' new variable->check message (rework/decoding.py:65-67, :179-183)
//
// Like qbp_math.hpp this compiles on the host too (tests/_shim/math_host_shim.cpp): the CPU suite checks
// these functions against the oracle bit for bit.
#pragma once

#include "qbp_math.hpp"

namespace qbp {

#if defined(QBP_DEVICE_BITS)
// Markers around arithmetic that does not run every iteration, for the static instruction count of
// tools/valu_mix.py (no effect on the hardware beyond two one-cycle scalar no-ops inside that path).
#define QBP_COLD_BEGIN() asm volatile("s_nop 9")
#define QBP_COLD_END() asm volatile("s_nop 10")
// true on every lane if it is true on any lane of the wavefront (the caller's branch is wave-uniform)
#define QBP_WAVE_ANY(cond) (__builtin_amdgcn_ballot_w64(cond) != 0ull)
#else
#define QBP_COLD_BEGIN() ((void)0)
#define QBP_COLD_END() ((void)0)
#define QBP_WAVE_ANY(cond) (cond)
#endif

// Scheduling fence between the messages of a wide row: the compiler otherwise overlaps all of a row's table-driven
// evaluations, whose live values then exceed the register budget of the wide builds (general-H kernel on
// 2592 x 7776, messages partly in L2: 1.33e5 -> 1.47e5 syndromes/s, 208 -> 184 spilled bytes; no change elsewhere:
// profiles/r03_ab_math.txt, block 6).  -DQBP_NO_EDGE_FENCES for A/B.
#if defined(QBP_DEVICE_BITS) && !defined(QBP_NO_EDGE_FENCES)
#define QBP_EDGE_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define QBP_EDGE_FENCE() ((void)0)
#endif

// ---- min-sum (rework/decoding.py:28-56) -------------------------------------------------------------
struct MinSumRow {
    double sprod;       // product of the signs (0 -> +1), NaN if any message is NaN
    double min1, min2;  // smallest |q|, and the smallest of the others
};

// load(j) -> message j of the row, j = 0 .. deg - 1 (called twice per message)
template <typename Load>
QBP_HD MinSumRow minsum_row(const Load& load, int deg)
{
    double sprod = 1.0, min1 = __builtin_inf();
    // (keeps its initial value only if every |q| is inf or NaN; min2 is inf then whatever it is)
    int min1_j = 0;
    bool anynan = false;
    for (int j = 0; j < deg; ++j) {
        const double x = load(j);
        const double s = x < 0.0 ? -1.0 : 1.0;
        sprod *= s;
        anynan |= x != x;
        const double a = __builtin_fabs(x);
        if (a < min1) { min1 = a; min1_j = j; }       // argmin: first occurrence
    }
    // np.sign(nan) = nan: one NaN message (inf - inf with infinite priors) makes the row's sign product,
    // hence every R of the row, NaN
    if (anynan) sprod = __builtin_nan("");
    double min2 = __builtin_inf();
    for (int j = 0; j < deg; ++j) {
        const double a = __builtin_fabs(load(j));
        if (j != min1_j && a < min2) min2 = a;
    }
    return MinSumRow{sprod, min1, min2};
}

// R of the edge whose message is x
QBP_HD double minsum_message(double x, const MinSumRow& row, unsigned sbit, double alpha)
{
    const double as = sbit ? -alpha : alpha;          // alpha * syndrome_sign
    const double s = x < 0.0 ? -1.0 : 1.0;
    const double mag = (__builtin_fabs(x) == row.min1) ? row.min2 : row.min1;
    return (as * (row.sprod * s)) * mag;
}

// ---- sum-product (beliefPropagation.py:114-126) ---------------------------------------------------------
// R of the edge whose tanh value is t, in a row whose tanh product is prod: any product, zero, subnormal and
// NaN included (before the alpha scaling of the damped variant)
// IEEE_DIV: the quotient by the compiler's full division sequence.  div_nr's residual a - b q is below the
// subnormal grid when the product is subnormal (a message of magnitude 1e-309 in the row), and its quotient then
// misses numpy's by an ulp; check_row's rare path, which is where such rows go, pays for the scaling steps.
template <int VARIANT, bool IEEE_DIV = false>
QBP_HD double sp_message(double prod, double t, unsigned sbit, NpT np_tab)
{
    const double ts = __builtin_fabs(t) < 1e-15 ? 1e-15 : t;         // t_safe (:122)
    // (a zero or denormal product: quotients of any size, down to the subnormals)
    return check_message<VARIANT>(IEEE_DIV ? prod / ts : div_nr(prod, ts), sbit, np_tab);     // :123-126
}

// Check update of one row held in registers: q[D] -> put(j, R_j), j = 0 .. D - 1.  put takes message j as
// soon as it exists (eight finished messages waiting for their stores are sixteen registers the wide rows do
// not have).  `scale` is false only for the alpha_estimation dump of the damped variant (rework/decoding.py:
// 168-169 returns R before the alpha scaling).  FENCE: QBP_EDGE_FENCE between the messages.  Called by the
// whole wavefront (the sum-product branch is a wave-uniform test).
template <int VARIANT, int D, bool FENCE, typename Put>
QBP_HD void check_row(const double (&q)[D], unsigned sbit, double alpha, bool scale, NpT np_tab, Put&& put)
{
    if constexpr (VARIANT == 2) {
        const MinSumRow row = minsum_row([&](int j) { return q[j]; }, D);
#pragma unroll
        for (int j = 0; j < D; ++j) put(j, minsum_message(q[j], row, sbit, alpha));
    } else {
        double t[D];
        double prod;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            t[j] = tanh_half_msg<VARIANT>(q[j], np_tab);     // np.tanh(Q * 0.5), :114
            if constexpr (FENCE) QBP_EDGE_FENCE();
        }
#pragma unroll
        for (int j = 0; j < D; ++j) prod = (j == 0) ? t[0] : prod * t[j];     // np.prod, ascending column
        // t_safe = where(|t| < 1e-15, 1e-15, t) (:122).  |t| <= 1, so a row whose product is at least 1e-15 in
        // magnitude has no such factor: one wave-uniform test on the product replaces the D compares and 2 D
        // selects in all but degenerate rows (messages of magnitude 1e-15, or six messages near 0.006 at once --
        // those take sp_message)
        if (QBP_WAVE_ANY(!(__builtin_fabs(prod) >= 1e-15))) {
            // (rare path, bracketed for tools/valu_mix.py: the instruction count that prices the kernel must
            // not include it)
            QBP_COLD_BEGIN();
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double r = sp_message<VARIANT, true>(prod, t[j], sbit, np_tab);
                put(j, (VARIANT == 1 && scale) ? r * alpha : r);
            }
            QBP_COLD_END();
        } else {
            // the syndrome sign applied to the product once per row instead of to every quotient
            // (check_message_signed: the same bits)
            const double prod_s = with_syndrome_sign(prod, sbit);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                // prod / t, correctly rounded like numpy's division: 1e-15 <= |prod| <= 1 and 1e-15 <= |t| <= 1,
                // so no operand scaling is needed (div_nr's precondition) and the quotient is at least 1e-15 in
                // magnitude (check_message: NORMAL)
                const double r = check_message_signed<VARIANT>(div_nr(prod_s, t[j]), np_tab);     // :123-126
                put(j, (VARIANT == 1 && scale) ? r * alpha : r);
                if constexpr (FENCE) QBP_EDGE_FENCE();
            }
        }
    }
}

// ---- damped variants: Q = clip(damping * Q_new + (1 - damping) * Q_old) ---------------------------------
// np.clip keeps a NaN a NaN (the damped variants can produce inf - inf when a check has a single edge:
// rework/decoding.py keeps iterating on NaNs there)
QBP_HD double damped_q(double qn, double q_old, double damping, double one_minus_damping, double clip)
{
    const double q = damping * qn + one_minus_damping * q_old;
    const double y = q < -clip ? -clip : q;
    return y > clip ? clip : y;
}

}  // namespace qbp
