// Host build of qldpc_amd/csrc/qbp_math.hpp and qbp_check.hpp, for the CPU test suite only (ulp-error and
// row-update tests).
#include "../../qldpc_amd/csrc/qbp_check.hpp"
extern "C" void shim_tanh_half(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = qbp::tanh_half(x[i]); }
extern "C" void shim_atanh2(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = qbp::atanh2(x[i]); }
extern "C" void shim_div(const double* a, const double* b, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = qbp::div_nr(a[i], b[i]); }
// numpy-exact forms: the image the kernels keep in LDS, here in host memory
alignas(16) static const qbp::NpImage g_host_image = qbp::np_make_image();
extern "C" void shim_np_tanh_half(const double* x, double* y, long n)
{
    const double* T = reinterpret_cast<const double*>(&g_host_image);
    for (long i = 0; i < n; ++i) y[i] = qbp::np_tanh_half(x[i], T);
}
extern "C" void shim_np_arctanh_x2(const double* x, double* y, long n)
{
    const double* T = reinterpret_cast<const double*>(&g_host_image);
    for (long i = 0; i < n; ++i) y[i] = qbp::np_arctanh_x2(x[i], T);
}
extern "C" void shim_np_rcp14_hi(const unsigned* v_hi, unsigned* r_hi, long n)
{
    for (long i = 0; i < n; ++i) r_hi[i] = qbp::np_rcp14_hi(v_hi[i], reinterpret_cast<const double*>(&g_host_image));
}
// the kernels' tail of the check update: 2 arctanh(clip(x * sign)) with the sign bit set at the end
extern "C" void shim_check_message(const double* x, const unsigned char* sbit, double* y, long n, int variant)
{
    const double* T = reinterpret_cast<const double*>(&g_host_image);
    for (long i = 0; i < n; ++i)
        y[i] = variant == 1 ? qbp::check_message<1>(x[i], sbit[i], T) : qbp::check_message<0>(x[i], sbit[i], T);
}
// the row update of qbp_check.hpp: check_row (a row of D = 1 .. 8 messages in registers, as the kernels run it)
// and the two-pass form of the kernels' long rows (any D).  variant 0 / 1: sum-product, 2: min-sum
template <int VARIANT, int D>
static void check_row_d(const double* q, unsigned sbit, double alpha, bool scale, double* out)
{
    double qd[D];
    for (int j = 0; j < D; ++j) qd[j] = q[j];
    qbp::check_row<VARIANT, D, false>(qd, sbit, alpha, scale, reinterpret_cast<const double*>(&g_host_image),
                                      [&](int j, double r) { out[j] = r; });
}
template <int VARIANT>
static int check_row_v(int D, const double* q, unsigned sbit, double alpha, bool scale, double* out)
{
    switch (D) {
    case 1: check_row_d<VARIANT, 1>(q, sbit, alpha, scale, out); return 0;
    case 2: check_row_d<VARIANT, 2>(q, sbit, alpha, scale, out); return 0;
    case 3: check_row_d<VARIANT, 3>(q, sbit, alpha, scale, out); return 0;
    case 4: check_row_d<VARIANT, 4>(q, sbit, alpha, scale, out); return 0;
    case 5: check_row_d<VARIANT, 5>(q, sbit, alpha, scale, out); return 0;
    case 6: check_row_d<VARIANT, 6>(q, sbit, alpha, scale, out); return 0;
    case 7: check_row_d<VARIANT, 7>(q, sbit, alpha, scale, out); return 0;
    case 8: check_row_d<VARIANT, 8>(q, sbit, alpha, scale, out); return 0;
    default: return -1;
    }
}
extern "C" int shim_check_row(int variant, int D, const double* q, unsigned sbit, double alpha, int scale, double* out)
{
    return variant == 0 ? check_row_v<0>(D, q, sbit, alpha, scale != 0, out)
         : variant == 1 ? check_row_v<1>(D, q, sbit, alpha, scale != 0, out)
         : variant == 2 ? check_row_v<2>(D, q, sbit, alpha, scale != 0, out) : -1;
}
template <int VARIANT>
static void check_long_v(int D, const double* q, unsigned sbit, double alpha, bool scale, double* out)
{
    const double* T = reinterpret_cast<const double*>(&g_host_image);
    if constexpr (VARIANT == 2) {
        const qbp::MinSumRow row = qbp::minsum_row([&](int j) { return q[j]; }, D);
        for (int j = 0; j < D; ++j) out[j] = qbp::minsum_message(q[j], row, sbit, alpha);
    } else {
        double prod = 1.0;
        for (int j = 0; j < D; ++j) {
            out[j] = qbp::tanh_half_msg<VARIANT>(q[j], T);
            prod = (j == 0) ? out[j] : prod * out[j];
        }
        for (int j = 0; j < D; ++j) {
            const double r = qbp::sp_message<VARIANT>(prod, out[j], sbit, T);
            out[j] = (VARIANT == 1 && scale) ? r * alpha : r;
        }
    }
}
extern "C" int shim_check_long(int variant, int D, const double* q, unsigned sbit, double alpha, int scale, double* out)
{
    if (variant == 0) check_long_v<0>(D, q, sbit, alpha, scale != 0, out);
    else if (variant == 1) check_long_v<1>(D, q, sbit, alpha, scale != 0, out);
    else if (variant == 2) check_long_v<2>(D, q, sbit, alpha, scale != 0, out);
    else return -1;
    return 0;
}
