// Host build of qldpc_amd/csrc/qbp_math.hpp for tests/test_tanh_fold_cpu.py: the kernels' np_tanh_half next to the
// candidate that folds its multiplication by 0.5 into the first fma (not in the kernels: DESIGN.md section 4), and the
// reciprocal table readers next to the forms they had before their byte offsets came from a byte select.
#include "../../qldpc_amd/csrc/qbp_math.hpp"

alignas(16) static const qbp::NpImage g_image = qbp::np_make_image();
static const double* image() { return reinterpret_cast<const double*>(&g_image); }

// ---- the folded candidate: r = fma(min(|q|, 64), 0.5, -midpoint), row and sign from q -----------------------------
static unsigned folded_tanh_row(unsigned q_hi)
{
    int e = (int)((q_hi >> 19) & 0xfffu);           // q's exponent field is one more than that of x = q / 2
    e = e < 0x7fa ? 0x7fa : (e > 0x7fa + 15 ? 0x7fa + 15 : e);
    return (unsigned)(e - 0x7fa) * 144u;
}
static double folded_np_tanh_half(double q, const double* T)
{
    const unsigned row = folded_tanh_row(qbp::np_hi(q));
    qbp::NpPair c = qbp::np_ld_pair(T, row);
    const double r = __builtin_fma(__builtin_fmin(__builtin_fabs(q), 64.0), 0.5, -c.a);
    double p = c.b;
    for (int s = 1; s <= 8; ++s) {
        c = qbp::np_ld_pair(T, row + 16 * s);
        p = __builtin_fma(p, r, c.a);
        p = __builtin_fma(p, r, c.b);
    }
    return __builtin_copysign(p, q);
}
// ---- the earlier table readers --------------------------------------------------------------------------------------
static unsigned parent_rcp14_hi(unsigned v_hi, const double* T)
{
    const double e = qbp::np_ld_f64(T, qbp::NP_OFF_LUT + ((v_hi >> 12) & 0xf8u));
    const unsigned em16 = (v_hi & 0x7ff00000u) | ((v_hi >> 4) & 0xffffu);
    return (qbp::np_hi(e) - em16) & 0xffff0000u;
}
static unsigned parent_rcp14_12_hi(unsigned p_hi, const double* T)
{
    const double e = qbp::np_ld_f64(T, qbp::NP_OFF_LUT_P + ((p_hi >> 12) & 0xf8u));
    return (qbp::np_hi(e) - (p_hi >> 4)) & 0xffff0000u;
}

// which: 0 the kernels' form (tanh: x = q * 0.5 formed; tables: offsets by byte select), 1 the other one
extern "C" void fold_tanh_half(int which, const double* q, double* y, long n)
{
    for (long i = 0; i < n; ++i) y[i] = which ? folded_np_tanh_half(q[i], image()) : qbp::np_tanh_half(q[i], image());
}
// the NaN-preserving wrap of the damped variant (tanh_half_msg<1>) still sees q
extern "C" void fold_tanh_half_msg1(const double* q, double* y, long n)
{
    for (long i = 0; i < n; ++i) y[i] = qbp::tanh_half_msg<1>(q[i], image());
}
// form: 0 np_rcp14 (any positive normal operand), 1 np_rcp14_12 (operands in [1, 2))
extern "C" void fold_rcp14_hi(int which, int form, const unsigned* v_hi, unsigned* r_hi, long n)
{
    for (long i = 0; i < n; ++i) {
        if (form == 0) r_hi[i] = which ? parent_rcp14_hi(v_hi[i], image()) : qbp::np_hi(qbp::np_rcp14(v_hi[i], image()));
        else r_hi[i] = which ? parent_rcp14_12_hi(v_hi[i], image()) : qbp::np_hi(qbp::np_rcp14_12(v_hi[i], image()));
    }
}
extern "C" double fold_row_midpoint(int row) { return image()[row * 18]; }
