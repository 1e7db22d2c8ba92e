// libqbp.so -- host side of the C ABI declared in include/qbp.h (gfx950 only, no CPU fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/qbp.h"
#include "qbp_kernels.hpp"
#include "qbp_osd.hpp"
#include "qbp_osd_order.hpp"
#include "qbp_osd_order_big.hpp"
#include "qbp_generic.hpp"
#include "qbp_stream.hpp"
#include "qbp_hist.hpp"
#include "qbp_relay.hpp"
#include "qbp_gd.hpp"
#include "qbp_cond.hpp"
#include "qbp_lsd.hpp"
#include "qbp_lsd_large.hpp"
#include "qbp_distance.hpp"
#include "qbp_frame.hpp"
#include "qbp_layered.hpp"
#include "qbp_quant.hpp"
#include "qbp_window.hpp"
#include "qbp_launch.hpp"
#include "qbp_msg_mem.hpp"

static_assert(QBP_NUM_COUNTERS == qbp::NUM_COUNTERS, "counter layout");
static_assert(QBP_MC_MAX_BUDGETS == qbp::MAX_BUDGETS, "budget ladder length");
static_assert(QBP_SPECTRUM_ROWS == qbp::SPECTRUM_ROWS, "spectrum rows");
static_assert(QBP_LLR_HIST_ROWS == qbp::LLR_HIST_ROWS, "LLR histogram rows");
static_assert(QBP_LLR_HIST_WORDS(9, 128) <= QBP_LLR_HIST_MAX_WORDS && QBP_LLR_HIST_WORDS(1, 1024) <= QBP_LLR_HIST_MAX_WORDS,
              "LLR histogram cap");

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// No C++ exception crosses the C ABI: EVERY extern "C" entry point is a function-try-block ending in
// QBP_ABI_CATCH (std::bad_alloc -> QBP_E_NOMEM: tests/test_host_cpu.py forces one).
#define QBP_ABI_CATCH                                                                      \
    catch (const std::bad_alloc&) { return fail(QBP_E_NOMEM, "out of host memory"); }     \
    catch (const std::exception& ex) { return fail(QBP_E_INVALID, "internal error: %s", ex.what()); } \
    catch (...) { return fail(QBP_E_INVALID, "internal error"); }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(QBP_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                               \
    } while (0)

using qbp::DC_SMALL; using qbp::DV_SMALL; using qbp::DC_WIDE; using qbp::DV_WIDE;

// Makes `device` current for the lifetime of the object and restores the caller's device
// afterwards (entry points must not leave a host thread on another GPU than they found it on).
struct DeviceScope {
    int prev = -1;
    hipError_t err;
    explicit DeviceScope(int device)
    {
        err = hipGetDevice(&prev);
        if (err != hipSuccess) { prev = -1; err = hipSuccess; }
        if (prev != device) err = hipSetDevice(device); else prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// Device memory owned by the handle, freed with it (qbp_destroy deletes the handle on its device).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t reserve(size_t count)
    {
        if (count <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) cap = count;
        return e;
    }
    // a host table copied to the device (synchronously: the vector may go out of scope on return)
    hipError_t upload(const std::vector<T>& v)
    {
        hipError_t e = reserve(v.size());
        if (e == hipSuccess && !v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
};

// The host-array side of one call on `s`: every host entry point stages through one of these.
//   in     a host array uploaded into a DevBuf; the device pointer
//   out    null for a null host array; else the DevBuf reserved and its download recorded; the device pointer
//   zeroed a DevBuf of accumulators reserved and set to zero; add: the sum into a host array recorded (null: none)
//   finish rc != 0 (the device entry refused, g_err is its message): synchronise and return rc; else enqueue what
//          out and add recorded, synchronise, add up and return QBP_OK -- or the first HIP error of any step
// Whatever way a call leaves -- finish, an early return, an exception -- the destructor has synchronised the stream
// if finish has not: copies of a refused call may still be in flight, and the next call on the handle, which reserves
// the same DevBufs again, must not find them so.  After a HIP error in / out / zeroed return null and enqueue nothing:
// the caller returns error() instead of making the device call.
class HostStage {
    struct Copy { void* host; const void* dev; size_t bytes; };
    struct Sum { int64_t* host; const long long* dev; size_t count; };
    hipStream_t s;
    hipError_t err = hipSuccess;
    const char* what = "";
    int line = 0;
    bool finished = false;
    std::vector<Copy> downloads;
    std::vector<Sum> sums;
    bool step(hipError_t e, const char* expr, int at)
    {
        if (err == hipSuccess && e != hipSuccess) { err = e; what = expr; line = at; }
        return err == hipSuccess;
    }
// (the message of HIP_TRY: the expression, the HIP error, where)
#define QBP_STAGE_STEP(expr) step((expr), #expr, __LINE__)

public:
    explicit HostStage(hipStream_t stream) : s(stream) {}
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    ~HostStage() { if (!finished) (void)hipStreamSynchronize(s); }
    bool failed() const { return err != hipSuccess; }

    template <typename T>
    T* in(DevBuf<T>& buf, const T* host, size_t count)
    {
        if (failed() || !QBP_STAGE_STEP(buf.reserve(count))) return nullptr;
        QBP_STAGE_STEP(hipMemcpyAsync(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice, s));
        return failed() ? nullptr : buf.p;
    }
    template <typename T>
    T* out(DevBuf<T>& buf, T* host, size_t count)
    {
        if (!host || failed() || !QBP_STAGE_STEP(buf.reserve(count))) return nullptr;
        downloads.push_back({host, buf.p, count * sizeof(T)});
        return buf.p;
    }
    long long* zeroed(DevBuf<long long>& buf, size_t count)
    {
        if (failed() || !QBP_STAGE_STEP(buf.reserve(count))) return nullptr;
        QBP_STAGE_STEP(hipMemsetAsync(buf.p, 0, count * sizeof(long long), s));
        return failed() ? nullptr : buf.p;
    }
    void add(int64_t* host, const long long* dev, size_t count)
    {
        if (host && !failed()) sums.push_back({host, dev, count});
    }
    int error() const
    {
        return fail(QBP_E_HIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(err), __FILE__, line);
    }
    int finish(int rc)
    {
        if (rc || failed()) return rc ? rc : error();      // (the destructor synchronises)
        size_t cells = 0;
        for (const Sum& a : sums) cells += a.count;
        std::vector<long long> tmp(cells);
        for (const Copy& c : downloads)
            if (c.bytes) QBP_STAGE_STEP(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, s));
        long long* t = tmp.data();
        for (const Sum& a : sums) {
            QBP_STAGE_STEP(hipMemcpyAsync(t, a.dev, a.count * sizeof(long long), hipMemcpyDeviceToHost, s));
            t += a.count;
        }
        finished = true;
        if (!QBP_STAGE_STEP(hipStreamSynchronize(s))) return error();
        t = tmp.data();
        for (const Sum& a : sums)
            for (size_t i = 0; i < a.count; ++i) a.host[i] += *t++;
        return QBP_OK;
    }
#undef QBP_STAGE_STEP
};

// "prior has no NaN" (+-inf are legal: a column known to be 0 or 1), or "prior is finite" where the decoder needs it
// (host only, before any GPU work).  Two loops, each the one the entries had inline: the NaN one runs in every
// one-syndrome qbp_decode_batch call.
inline int check_prior(int n, const double* prior, bool must_be_finite)
{
    if (must_be_finite) {
        for (int v = 0; v < n; ++v)
            if (!std::isfinite(prior[v])) return fail(QBP_E_INVALID, "prior[%d] is not finite", v);
        return QBP_OK;
    }
    for (int v = 0; v < n; ++v)
        if (prior[v] != prior[v]) return fail(QBP_E_INVALID, "prior[%d] is NaN (+-inf are legal)", v);
    return QBP_OK;
}

unsigned mc_threshold(double p)
{
    double t = std::floor(p * 4294967296.0);
    if (!(t > 0.0)) t = 0.0;
    if (t > 4294967295.0) t = 4294967295.0;
    return (unsigned)t;
}

// The input tables of a Monte-Carlo call on the device, with host copies of what was uploaded last: a call uploads
// only what changed.  The copy goes on the call's stream, behind any earlier launch there that still reads the table,
// and is waited for because its source is a local.  A failed upload leaves the cache empty.
struct McInputs {
    DevBuf<unsigned long long> d_lx_cols;    // per column, bit l: Lx[l] has it
    std::vector<uint8_t> lx_cache;
    int lx_cache_k = -1;
    DevBuf<uint32_t> d_thr;                  // a sampler threshold per column, [n rounded up to 4] (zero in the padding)
    std::vector<uint32_t> thr_cache;
    DevBuf<double> d_llr_edges;              // qbp_mc_run_llr_hist: np.linspace(lo, hi, bins + 1)
    std::vector<double> edges_cache;

    int prepare_lx(size_t n, const uint8_t* Lx, int32_t k, hipStream_t s)
    {
        if (lx_cache_k == k && lx_cache.size() == (size_t)k * n &&
            (k == 0 || std::memcmp(lx_cache.data(), Lx, (size_t)k * n) == 0))
            return QBP_OK;
        std::vector<unsigned long long> cols(n, 0ull);
        for (int l = 0; l < k; ++l)
            for (size_t v = 0; v < n; ++v)
                if (Lx[(size_t)l * n + v] & 1) cols[v] |= 1ull << l;
        lx_cache_k = -1;
        HIP_TRY(d_lx_cols.reserve(n));
        HIP_TRY(hipMemcpyAsync(d_lx_cols.p, cols.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        lx_cache.assign(Lx, Lx + (size_t)k * n);
        lx_cache_k = k;
        return QBP_OK;
    }
    int prepare_thr(size_t n, const double* probs, hipStream_t s)
    {
        const size_t n4 = (n + 3) / 4 * 4;
        std::vector<uint32_t> thr(n4, 0u);
        for (size_t v = 0; v < n; ++v) thr[v] = mc_threshold(probs[v]);
        if (thr_cache == thr) return QBP_OK;
        thr_cache.clear();
        HIP_TRY(d_thr.reserve(n4));
        HIP_TRY(hipMemcpyAsync(d_thr.p, thr.data(), n4 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        thr_cache.swap(thr);
        return QBP_OK;
    }
    int prepare_edges(int bins, double lo, double hi, hipStream_t s)
    {
        // np.linspace(lo, hi, bins + 1): start + i * step, the last edge exactly hi (as qbp_message_histograms)
        std::vector<double> edges((size_t)bins + 1);
        const double step = (hi - lo) / (double)bins;
        for (int i = 0; i < bins; ++i) edges[i] = (double)i * step + lo;
        edges[bins] = hi;
        if (edges_cache == edges) return QBP_OK;
        edges_cache.clear();
        HIP_TRY(d_llr_edges.reserve(edges.size()));
        HIP_TRY(hipMemcpyAsync(d_llr_edges.p, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        edges_cache.swap(edges);
        return QBP_OK;
    }
};

}  // namespace

struct qbp_handle {
    int device = 0;
    int m = 0, n = 0, E = 0;
    int max_row_deg = 0, max_col_deg = 0;
    int num_cu = 0;
    bool fused_ok = false;
    int dc = DC_SMALL, dv = DV_SMALL;   // instantiation used by this matrix
    int r_stride = 0;                   // on-chip kernel: doubles of one slot's message records (HostTables)
    bool padded = false;
    std::vector<int32_t> row_ptr, col_idx;
    // device tables for the fused kernel
    DevBuf<int32_t> d_tab_var;
    DevBuf<uint16_t> d_tab_gather, d_tab_store;
    DevBuf<uint32_t> d_tab_writer;
    DevBuf<int32_t> d_iso;
    int n_iso = 0;
    DevBuf<unsigned long long> d_work_counter;
    // options
    int opt_slots = 0, opt_blocks_per_cu = 0;
    // last launch configuration (introspection)
    int last_threads = 0, last_lds = 0, last_grid = 0, last_kernel = 0;
    // scratch for the host-pointer entry points
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> d_syn, d_hard, d_conv;
    DevBuf<int32_t> d_iters;
    DevBuf<double> d_llr, d_prior, d_mathx, d_mathy, d_part, d_edges;
    DevBuf<unsigned long long> d_hist;
    McInputs mc_in;                  // the Lx columns, and the sampler thresholds of qbp_mc_run_probs
    DevBuf<long long> d_counters;
    DevBuf<long long> d_spectrum;    // qbp_mc_run_spectrum: [QBP_SPECTRUM_ROWS][n + 1], then iter_hist [max_iter + 1]
    // general-H kernel
    DevBuf<int32_t> d_col_ptr, d_col_edge;
    DevBuf<double> d_wsQ, d_wsR, d_wsV;
    DevBuf<uint8_t> d_wsC;
    int opt_force_generic = 0;
    int opt_forced_two_barriers = 0;   // 1: forced-iteration launches keep the second barrier of the iteration (A/B, tests)
    int last_one_barrier = 0;
    int opt_early_exit_full_wg = 0;    // 1: early-exit launches use 16-wavefront workgroups like forced ones (A/B)
    int opt_no_r0_table = 0;           // 1: early-exit launches compute the first check step like every other (A/B, tests)
    int opt_kernel = 0;             // 0 auto, 1 on-chip, 2 general-H (workgroup per syndrome), 3 streaming
    DevBuf<uint8_t> d_wsS;           // streaming kernel: transposed syndromes; general-H Monte-Carlo: syndromes
    DevBuf<uint8_t> d_wsE;           // general-H Monte-Carlo: sampled errors
    DevBuf<uint8_t> d_weight_err;    // qbp_mc_run_weight, qbp_mc_run_enum, qbp_enum_failures: the errors of one chunk, [chunk][n]
    // weight-w enumeration (qbp_mc_run_enum, qbp_enum_failures): C(j, t) for t <= binom_w, j <= n (enum_prepare); the
    // shots of one chunk of qbp_enum_failures and what the shots launches say of them; scratch of its host entry
    DevBuf<unsigned long long> d_binom;
    int binom_w = -1;
    DevBuf<uint8_t> d_enum_det, d_enum_conv, d_enum_kinds;
    DevBuf<unsigned long long> d_enum_actual, d_enum_pred, d_enum_found;
    DevBuf<long long> d_enum_ranks;
    // fixed-weight fault sampling (qbp_fault_table_set): the active sites' first faults and K, the column of every
    // fault; the sites one launch of the sampler picks, [weight][trials of a launch]
    DevBuf<long long> d_fault_first;
    DevBuf<uint8_t> d_fault_k;
    DevBuf<int32_t> d_fault_col;
    DevBuf<uint32_t> d_fault_picks;
    long long fault_sites = 0;       // N; 0: no table
    long long opt_weight_chunk = 0;  // QBP_OPT_MC_WEIGHT_CHUNK (0 = default)
    long long opt_llr_hist_chunk = 0;   // QBP_OPT_LLR_HIST_CHUNK (0 = default)
    DevBuf<int32_t> d_srow, d_srow_e0, d_srow_deg, d_svar, d_sedge;   // weight-class tables
    DevBuf<int32_t> d_epos, d_cpos, d_long_edge_row;
    DevBuf<int32_t> d_vpos, d_vrow, d_lcol_ptr;      // general-H kernel: column-class tables
    DevBuf<double> d_wsL, d_prior_sorted;
    DevBuf<double> d_wsM;           // Relay-BP and BP guided decimation, large builds: [grid][E] messages (a call has
                                    // one second stage, and neither kernel keeps messages from launch to launch)
    int gcol_base[qbp::GENERIC_MAX_COL_CLASS + 2] = {0};
    int rpad_off[qbp::GENERIC_MAX_ROW_CLASS + 2] = {0}, cpad_off[qbp::GENERIC_MAX_COL_CLASS + 2] = {0};
    int opt_threads = 0;            // general-H kernel: threads per workgroup (0 = auto)
    int opt_no_lds_tables = 0;      // general-H kernel: keep the variable step's tables in L2 (A/B)
    int opt_no_r_split = 0;         // general-H kernel: no part of R in LDS when the messages do not fit (A/B)
    int opt_mem = 0;                // general-H kernel: 0 auto, 1 messages in global memory, 2 half of R in LDS (tests)
    int row_base[qbp::GENERIC_MAX_ROW_CLASS + 2] = {0};
    int row_off[qbp::STREAM_MAX_ROW_CLASS + 3] = {0};
    int col_off[qbp::STREAM_MAX_COL_CLASS + 3] = {0}, col_edge_base[qbp::STREAM_MAX_COL_CLASS + 2] = {0};
    // pinned, device-mapped staging for small host-pointer calls (zero-copy: no hipMemcpy at all)
    void* pin_host = nullptr;
    void* pin_dev = nullptr;
    size_t pin_bytes = 0;
    // two pinned staging buffers for the outputs of large host-pointer calls (device -> pinned by DMA
    // at PCIe rate, pinned -> caller's pageable array by memcpy, one chunk behind)
    void* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    size_t stage_bytes = 0;
    // OSD-0
    bool osd_ok = false;            // fits the one-wavefront kernel (matrix rows in LDS)
    int opt_osd_big = 0;            // QBP_OPT_OSD_BIG
    bool osd_ready = false;         // d_hbits and osd_rank built (osd_prepare)
    int osd_W = 0, osd_NP = 0, osd_lds = 0, osd_rank = 0;
    DevBuf<uint32_t> d_osd_At;
    DevBuf<int32_t> d_osd_piv, d_osd_idx, d_osd_posn;
    DevBuf<int32_t> d_osd_tk;       // osd_order_blocked_kernel: non-pivot columns (and its spilled column table)
    DevBuf<unsigned long long> d_osd_next;   // work counter of osd0_blocked_kernel
    DevBuf<long long> d_osd_redo;   // [0]: count, [1..]: records whose OSD sweep found the syndrome inconsistent
    DevBuf<uint8_t> d_osd_sol;
    DevBuf<int32_t> d_osd_order;    // qbp_osd_batch_ordered: the caller's column orders
    DevBuf<unsigned long long> d_osd_keys;
    DevBuf<uint32_t> d_hbits;
    DevBuf<int32_t> d_row_ptr, d_col_idx;
    DevBuf<uint8_t> d_sol;
    // the order-dependent tables once more, for column sums in the order of a Fortran-ordered dense R
    // (QBP_FLAG_DENSE_F_COLSUM; built at the first such call)
    struct ColumnOrderTables {
        int state = 0;               // 0 not built, 1 ready, -1 not expressible (QBP_E_UNSUPPORTED)
        DevBuf<uint16_t> tab_gather, tab_store;
        DevBuf<uint32_t> tab_writer;
        DevBuf<int32_t> col_edge, sedge, vpos, vrow;
    } f_order;
    // Monte-Carlo + OSD failure records
    DevBuf<long long> d_fail_list;
    DevBuf<unsigned long long> d_fail_count;
    DevBuf<uint8_t> d_fail_syn, d_fail_hard, d_fail_err;
    DevBuf<double> d_fail_llr;
    // qbp_decode_shots, host-pointer entry: recorded observables and predictions of the call
    DevBuf<unsigned long long> d_shot_actual, d_shot_pred;
    // Relay-BP (qbp_relay_configure): the memory strengths in sorted-variable order, the legs' iteration counts, the
    // inverse of svar; scratch of the host-pointer entry
    bool relay_ready = false;
    int relay_L = 0, relay_stop_after = 0;
    double relay_alpha = 1.0, relay_clip = 0.0;
    DevBuf<double> d_relay_gammas;
    DevBuf<int32_t> d_relay_iters, d_relay_vinv, d_relay_legs, d_relay_sol;
    // QBP_OPT_RELAY_MEM, QBP_OPT_LAYERED_MEM, QBP_OPT_GD_MEM, QBP_OPT_LSD_MEM by qbp::MsgMemFamily (qbp_msg_mem.hpp states
    // the rule)
    int opt_msg_mem[qbp::MSG_MEM_FAMILIES] = {0};
    // BP guided decimation (qbp_gd_configure); scratch of the host-pointer entry
    bool gd_ready = false;
    int gd_iters = 0, gd_max_rounds = 0, gd_variant = 0;
    double gd_llr = 0.0, gd_alpha = 1.0, gd_clip = 0.0;
    DevBuf<int32_t> d_gd_rounds;
    // BP with a prior per record (qbp_decode_batch_cond): the second prior in sorted-variable order; scratch of the
    // host-pointer entry
    DevBuf<double> d_prior1_sorted, d_cond_prior1;
    DevBuf<uint8_t> d_cond_sel;
    // localized statistics decoding (qbp_lsd_configure): bits_per_step, the checks of every column (CSC, beside
    // d_col_ptr); scratch of the host-pointer entry.  The large build's rows and sort keys use d_osd_At and d_osd_keys:
    // a call has one second stage, and calls on a handle are serial
    bool lsd_ready = false;
    int lsd_bits = 0;
    DevBuf<int32_t> d_lsd_col_row, d_lsd_stats;
    // distance search (qbp_distance_search): the bit-packed rows of G and L of the call; its histogram, then the
    // call's best word, the capture launch's two words and logical mask; the captured row
    DevBuf<uint32_t> d_dist_gbits, d_dist_lbits;
    DevBuf<long long> d_dist_out;
    DevBuf<uint8_t> d_dist_codeword;
    // layered BP (qbp_layered_configure): the checks level after level, the level boundaries
    bool layered_ready = false;
    int layered_levels = 0, layered_max_width = 0;
    int opt_layered_slots = 0;      // QBP_OPT_LAYERED_SLOTS (0 = auto)
    DevBuf<int32_t> d_layered_order, d_layered_level_ptr;
    DevBuf<double> d_layered_wsR;   // layered BP, large build: [grid][S][E] messages
    // fixed-point min-sum (qbp_quant_configure); scratch of the host-pointer entry
    bool quant_ready = false;
    int quant_bits = 0, quant_num = 1, quant_shift = 0, quant_beta = 0;
    double quant_scale = 1.0;
    int opt_quant_slots = 0;        // QBP_OPT_QUANT_SLOTS (0 = auto)
    DevBuf<int32_t> d_quant_post;
};

namespace {

using qbp::FusedParams;

using qbp::LaunchCfg;

// Dynamic LDS of one workgroup of the fused kernel (the carve is documented in qbp_kernels.hpp)
// slot_counters: counter ints per slot (2 * n_budgets rows in the launches of qbp_mc_run_budgets)
// hist_words: bins of the workgroup's iteration histogram in the launches of qbp_mc_run_spectrum (max_iter + 1; with
// them a residual-weight word per slot), else 0
// llr_bytes: the workgroup's posterior-LLR table in the launches of qbp_mc_run_llr_hist (llr_hist_lds_bytes), else 0
size_t fused_lds_bytes(int dc, int m, int n, int S, int r_stride, bool two_copies = false, bool r0_table = false,
                       int slot_counters = qbp::NUM_COUNTERS, int hist_words = 0, size_t llr_bytes = 0)
{
    const size_t r_doubles = qbp::fused_r_doubles(r_stride, dc == DC_SMALL ? DV_SMALL : DV_WIDE, S);   // one copy of R
    size_t lds = (size_t)qbp::NP_LDS_BYTES +      // tables of tanh / arctanh (qbp_math.hpp), at the start
                 (two_copies ? (size_t)qbp::FUSED_R2_OFF_BYTES : 0) + (r0_table ? (size_t)2 * dc * m * 8 : 0) +
                 (r_doubles + (size_t)dc * m + 3 * (size_t)S) * 8 +
                 (6 * (size_t)S + 1 + (size_t)S * (size_t)slot_counters + (size_t)dc * m) * 4 +
                 2 * (size_t)S * (((size_t)n + 3) / 4) * 4 +    // err_lds[2][S][n4] (Monte-Carlo builds)
                 (hist_words ? ((size_t)S + (size_t)hist_words) * 4 : 0) +
                 (llr_bytes ? llr_bytes + 8 : 0);               // (from the next 8-byte boundary)
    return (lds + 15) & ~(size_t)15;
}

// Everything qbp_create derives from the CSR arrays on the host (no device involved; qbp_plan
// exposes it so that the CPU test-suite can check the tables).
struct HostTables {
    int max_row = 0, max_col = 0, dc = DC_SMALL, dv = DV_SMALL;
    bool fused_ok = false, padded = false;
    std::vector<int32_t> tab_var;      // [dc][m]
    std::vector<uint16_t> tab_nbr;     // [dc][dv][m]  the columns as edge lists: filled for qbp_plan only (no kernel reads it)
    std::vector<uint16_t> tab_gather;  // [dc][m]      the R records of the on-chip kernel (qbp_kernels.hpp)
    std::vector<uint16_t> tab_store;   // [dc][m]
    int r_stride = 0;                  // doubles of one slot's records
    std::vector<uint32_t> tab_writer;  // [m]
    std::vector<int32_t> iso, col_ptr, col_edge;
    // streaming kernel: checks / variables sorted by weight class (qbp_stream.hpp)
    std::vector<int32_t> srow, srow_e0, srow_deg, svar, sedge;
    // general-H kernel: class-blocked transposed message layout (qbp_generic.hpp)
    std::vector<int32_t> epos, cpos, long_edge_row;
    std::vector<int32_t> vpos, vrow, lcol_ptr;         // general-H kernel, variables by column class
    int gcol_base[qbp::GENERIC_MAX_COL_CLASS + 2] = {0};
    int row_base[qbp::GENERIC_MAX_ROW_CLASS + 2] = {0};
    int row_off[qbp::STREAM_MAX_ROW_CLASS + 3] = {0};
    int col_off[qbp::STREAM_MAX_COL_CLASS + 3] = {0}, col_edge_base[qbp::STREAM_MAX_COL_CLASS + 2] = {0};
};

// Order in which np.sum(R, axis=0) adds up the non-zero entries of one column of a FORTRAN-ordered dense
// (m, n) array R -- which is what the reference's dense single-syndrome forms reduce whenever the caller's
// H is Fortran-ordered, as the Hx of its code files is (every (m, n) temporary inherits the layout of
// `mask = H != 0`).  The column is contiguous then and numpy runs pairwise_sum over all m entries, zeros
// included (numpy/_core/src/umath/loops_utils.h.src): fewer than 8 rows left to right; up to 128 rows eight
// running sums by row mod 8, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the m mod 8 trailing rows;
// more rows split in halves (the first a multiple of 8) recursively.  x + 0.0 is exact, so only the
// association of the non-zero entries matters: simulated here symbolically.  Returns false when that
// association is not a left-to-right sum of SOME ordering of the entries (possible from 4 entries on:
// (a + b) + (c + d)); `order` = that ordering as indices into the column's ascending-check list.
struct FSumNode { int leaf, l, r; };
static int fsum_add(std::vector<FSumNode>& pool, int a, int b)
{
    if (a < 0) return b;
    if (b < 0) return a;
    pool.push_back({-1, a, b});
    return (int)pool.size() - 1;
}
static int fsum_range(std::vector<FSumNode>& pool, const std::vector<int>& rows, int lo, int hi)
{
    const int n = hi - lo;
    int a = 0;
    while (a < (int)rows.size() && rows[a] < lo) ++a;
    int b = a;
    while (b < (int)rows.size() && rows[b] < hi) ++b;
    if (a == b) return -1;
    if (n < 8) {
        int res = -1;
        for (int i = a; i < b; ++i) res = fsum_add(pool, res, i);
        return res;
    }
    if (n <= 128) {
        int r[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
        const int body = n - n % 8;
        int i = a;
        for (; i < b && rows[i] - lo < body; ++i) r[(rows[i] - lo) % 8] = fsum_add(pool, r[(rows[i] - lo) % 8], i);
        int res = fsum_add(pool, fsum_add(pool, fsum_add(pool, r[0], r[1]), fsum_add(pool, r[2], r[3])),
                           fsum_add(pool, fsum_add(pool, r[4], r[5]), fsum_add(pool, r[6], r[7])));
        for (; i < b; ++i) res = fsum_add(pool, res, i);
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return fsum_add(pool, fsum_range(pool, rows, lo, lo + n2), fsum_range(pool, rows, lo + n2, hi));
}
static bool fsum_flatten(const std::vector<FSumNode>& pool, int node, std::vector<int>& out)
{
    const FSumNode& x = pool[node];
    if (x.leaf >= 0) { out.push_back(x.leaf); return true; }
    const bool ll = pool[x.l].leaf >= 0, rl = pool[x.r].leaf >= 0;
    if (rl) { if (!fsum_flatten(pool, x.l, out)) return false; out.push_back(pool[x.r].leaf); return true; }
    if (ll) { if (!fsum_flatten(pool, x.r, out)) return false; out.push_back(pool[x.l].leaf); return true; }
    return false;
}
static bool dense_f_column_order(const std::vector<int>& rows, int m, std::vector<int>& order)
{
    std::vector<FSumNode> pool;
    for (int i = 0; i < (int)rows.size(); ++i) pool.push_back({i, -1, -1});
    order.clear();
    if (rows.empty()) return true;
    const int root = fsum_range(pool, rows, 0, m);
    return fsum_flatten(pool, root, order) && order.size() == rows.size();
}

// col_order: 0 = every column's entries in ascending check order (np.sum(R, axis=0) of a C-ordered R adds row
// by row); 1 = the order of a Fortran-ordered R (dense_f_column_order).  All kernels add a column's messages
// left to right in the order of these tables.
int build_tables(const int32_t* row_ptr, const int32_t* col_idx, int m, int n, HostTables& T, int col_order = 0,
                 bool with_nbr = false)
{
    if (!row_ptr || m < 0 || n < 0) return fail(QBP_E_INVALID, "bad matrix arguments");
    if (m == 0 || n == 0) return fail(QBP_E_INVALID, "empty matrix (%d x %d)", m, n);
    if (row_ptr[0] != 0) return fail(QBP_E_INVALID, "row_ptr[0] must be 0");
    const int E = row_ptr[m];
    if (E < 0 || (E > 0 && !col_idx)) return fail(QBP_E_INVALID, "bad CSR arrays");
    // column lists in ascending check order: (check, position in that check's row)
    std::vector<std::vector<std::pair<int, int>>> cols(n);
    for (int c = 0; c < m; ++c) {
        if (row_ptr[c + 1] < row_ptr[c]) return fail(QBP_E_INVALID, "row_ptr not monotone at %d", c);
        T.max_row = std::max(T.max_row, row_ptr[c + 1] - row_ptr[c]);
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n)
                return fail(QBP_E_INVALID, "column index %d out of range in row %d", col_idx[e], c);
            if (e > row_ptr[c] && col_idx[e] <= col_idx[e - 1])
                return fail(QBP_E_INVALID, "columns of row %d not strictly ascending", c);
            cols[col_idx[e]].push_back({c, e - row_ptr[c]});
        }
    }
    for (int v = 0; v < n; ++v) {
        T.max_col = std::max(T.max_col, (int)cols[v].size());
        if (cols[v].empty()) T.iso.push_back(v);
    }
    if (col_order == 1) {
        std::vector<int> rows, order;
        for (int v = 0; v < n; ++v) {
            rows.clear();
            for (const auto& ce : cols[v]) rows.push_back(ce.first);
            if (!dense_f_column_order(rows, m, order))
                return fail(QBP_E_UNSUPPORTED,
                            "column %d (%zu entries): numpy's pairwise sum over a Fortran-ordered dense column "
                            "associates them as a balanced tree, which the kernels' left-to-right sums cannot "
                            "express", v, rows.size());
            std::vector<std::pair<int, int>> perm;
            for (int i : order) perm.push_back(cols[v][i]);
            cols[v] = perm;
        }
    }
    if (T.max_row <= DC_SMALL && T.max_col <= DV_SMALL) { T.dc = DC_SMALL; T.dv = DV_SMALL; }
    else { T.dc = DC_WIDE; T.dv = DV_WIDE; }
    // R records of the on-chip kernel (layout and invariant: qbp_kernels.hpp, fused_r_doubles).  A column of d < DV
    // checks has DV - d zero words to place: as many as the record before left free at its end go in front, where
    // the two records then overlap; the rest go behind.  DV = 3: columns of degree 1 take two words on average, of
    // degree 2 two and a half, of degree 3 three.
    std::vector<int> rec_base((size_t)n, 0), rec_lead((size_t)n, 0);
    if (T.max_col <= T.dv) {
        int words = 0, tail = 0;
        for (int v = 0; v < n; ++v) {
            const int d = (int)cols[v].size();
            if (d == 0) continue;
            const int lead = std::min(tail, T.dv - d);
            rec_base[v] = words - lead;
            rec_lead[v] = lead;
            words = rec_base[v] + T.dv;
            tail = T.dv - d - lead;
        }
        T.r_stride = words;
    }
    T.fused_ok = (m <= qbp::FUSED_MAX_THREADS) && T.max_row <= T.dc && T.max_col <= T.dv &&
                 fused_lds_bytes(T.dc, m, n, 1, T.r_stride) <= 160 * 1024;
    if (T.fused_ok) {
        const int DC = T.dc, DV = T.dv, zoff = DC * m;
        T.tab_var.assign((size_t)DC * m, -1);
        if (with_nbr) T.tab_nbr.assign((size_t)DC * DV * m, (uint16_t)zoff);
        T.tab_writer.assign(m, 0u);
        // padding edges gather the zero record (r_stride) and store to the dump word behind it
        T.tab_gather.assign((size_t)DC * m, (uint16_t)T.r_stride);
        T.tab_store.assign((size_t)DC * m, (uint16_t)(T.r_stride + DV));
        for (int c = 0; c < m; ++c) {
            const int deg = row_ptr[c + 1] - row_ptr[c];
            if (deg < DC) T.padded = true;
            for (int j = 0; j < deg; ++j) {
                const int v = col_idx[row_ptr[c] + j];
                T.tab_var[(size_t)j * m + c] = v;
                const auto& col = cols[v];
                T.tab_gather[(size_t)j * m + c] = (uint16_t)rec_base[v];
                for (size_t k = 0; k < col.size(); ++k) {
                    if (with_nbr) T.tab_nbr[((size_t)j * DV + k) * m + c] = (uint16_t)(col[k].second * m + col[k].first);
                    if (col[k].first == c) T.tab_store[(size_t)j * m + c] = (uint16_t)(rec_base[v] + rec_lead[v] + (int)k);
                }
                if (col[0].first == c) T.tab_writer[c] |= 1u << j;     // (one lane per variable writes its outputs)
            }
        }
    }
    // CSC (edge ids per column, ascending check) for the general-H kernel
    T.col_ptr.assign((size_t)n + 1, 0);
    T.col_edge.assign((size_t)std::max(E, 1), 0);
    for (int v = 0; v < n; ++v) T.col_ptr[v + 1] = T.col_ptr[v] + (int)cols[v].size();
    for (int v = 0; v < n; ++v)
        for (size_t k = 0; k < cols[v].size(); ++k)
            T.col_edge[T.col_ptr[v] + k] = row_ptr[cols[v][k].first] + cols[v][k].second;
    // weight classes of the streaming kernel: rows 0 .. 8 and > 8, columns 0 .. 4 and > 4
    constexpr int RC = qbp::STREAM_MAX_ROW_CLASS, CC = qbp::STREAM_MAX_COL_CLASS;
    for (int k = 0; k <= RC + 1; ++k) {
        T.row_off[k] = (int)T.srow.size();
        for (int c = 0; c < m; ++c) {
            const int deg = row_ptr[c + 1] - row_ptr[c];
            if (std::min(deg, RC + 1) != k) continue;
            T.srow.push_back(c);
            T.srow_e0.push_back(row_ptr[c]);
            T.srow_deg.push_back(deg);
        }
    }
    T.row_off[RC + 2] = m;
    static_assert(qbp::GENERIC_MAX_ROW_CLASS == qbp::STREAM_MAX_ROW_CLASS, "shared row classes");
    T.epos.assign((size_t)std::max(E, 1), 0);
    T.cpos.assign((size_t)std::max(E, 1), 0);
    {
        int base = 0;
        for (int k = 1; k <= RC; ++k) {                 // block of the weight-k checks: [entry j][check i]
            const int cnt = T.row_off[k + 1] - T.row_off[k];
            T.row_base[k] = base;
            for (int i = 0; i < cnt; ++i)
                for (int j = 0; j < k; ++j) T.epos[T.srow_e0[T.row_off[k] + i] + j] = base + j * cnt + i;
            base += k * cnt;
        }
        T.row_base[RC + 1] = base;                      // longer checks: entries contiguous
        for (int i = T.row_off[RC + 1]; i < T.row_off[RC + 2]; ++i)
            for (int j = 0; j < T.srow_deg[i]; ++j) {
                T.epos[T.srow_e0[i] + j] = base++;
                T.long_edge_row.push_back(i - T.row_off[RC + 1]);
            }
    }
    for (int q = 0; q < E; ++q) T.cpos[q] = T.epos[T.col_edge[q]];
    for (int k = 0; k <= CC + 1; ++k) {
        T.col_off[k] = (int)T.svar.size();
        T.col_edge_base[k] = (int)T.sedge.size();
        for (int v = 0; v < n; ++v) {
            if (std::min<int>((int)cols[v].size(), CC + 1) != k) continue;
            T.svar.push_back(v);
            if (k >= 1 && k <= CC)
                for (int q = T.col_ptr[v]; q < T.col_ptr[v + 1]; ++q) T.sedge.push_back(T.col_edge[q]);
        }
    }
    T.col_off[CC + 2] = n;
    if (T.sedge.empty()) T.sedge.push_back(0);
    // general-H kernel: per column entry the message position and the SORTED position of its check,
    // blocked and transposed by column-weight class (qbp_generic.hpp); long columns contiguous
    static_assert(qbp::GENERIC_MAX_COL_CLASS == qbp::STREAM_MAX_COL_CLASS, "shared column classes");
    {
        std::vector<int32_t> wpos((size_t)m, 0);
        for (int w = 0; w < m; ++w) wpos[T.srow[w]] = w;
        T.vpos.assign((size_t)std::max(E, 1), 0);
        T.vrow.assign((size_t)std::max(E, 1), 0);
        int base = 0;
        for (int k = 1; k <= CC; ++k) {
            const int cnt = T.col_off[k + 1] - T.col_off[k];
            T.gcol_base[k] = base;
            for (int i = 0; i < cnt; ++i) {
                const int v = T.svar[T.col_off[k] + i];
                for (int j = 0; j < k; ++j) {
                    T.vpos[(size_t)base + (size_t)j * cnt + i] = T.cpos[T.col_ptr[v] + j];
                    T.vrow[(size_t)base + (size_t)j * cnt + i] = wpos[cols[v][j].first];
                }
            }
            base += k * cnt;
        }
        T.gcol_base[CC + 1] = base;
        for (int i = T.col_off[CC + 1]; i < T.col_off[CC + 2]; ++i) {
            const int v = T.svar[i];
            T.lcol_ptr.push_back(base);
            for (size_t j = 0; j < cols[v].size(); ++j) {
                T.vpos[base] = T.cpos[T.col_ptr[v] + (int)j];
                T.vrow[base] = wpos[cols[v][j].first];
                ++base;
            }
        }
        T.lcol_ptr.push_back(base);
    }
    return QBP_OK;
}

// n_budgets: rows of a qbp_mc_run_budgets launch (its slots keep 2 * n_budgets counter rows in LDS), else 0
// hist_words: max_iter + 1 in a qbp_mc_run_spectrum launch (the workgroup's iteration histogram in LDS), else 0
// llr_bytes: llr_hist_lds_bytes in a qbp_mc_run_llr_hist launch (the workgroup's posterior-LLR table in LDS), else 0
int make_cfg(qbp_handle* h, long long B, LaunchCfg* cfg, bool forced = false, bool mc = false, int n_budgets = 0,
             int hist_words = 0, size_t llr_bytes = 0)
{
    const int m = h->m;
    const int slot_counters = n_budgets > 0 ? 2 * n_budgets * qbp::NUM_COUNTERS : qbp::NUM_COUNTERS;
    auto lds_bytes = [&](int dc, int m_, int n_, int S_, bool two_copies = false, bool r0_table = false) {
        return fused_lds_bytes(dc, m_, n_, S_, h->r_stride, two_copies, r0_table, slot_counters, hist_words, llr_bytes);
    };
    int S = h->opt_slots;
    if (S <= 0) {
        // 16 wavefronts per workgroup (4 per SIMD at the kernel's 128-VGPR budget) was the fastest
        // geometry measured (profiles/r01_tune.txt); small batches spread over the CUs instead.
        S = std::max(1, qbp::FUSED_MAX_THREADS / std::max(m, 1));
        // With early exit the slots of a workgroup are in different iterations, yet every one of them
        // waits at the workgroup's barriers for the slowest (a slot in its first iteration copies six
        // table entries, its neighbour evaluates six tanh / division / atanh chains): two workgroups
        // of 8 wavefronts per CU -- half the slots behind each barrier, and one workgroup computing
        // while the other synchronises or writes results -- are 2 - 18 % faster on every early-exit
        // workload measured, although [[288,12,18]] then runs 6 syndromes per CU instead of 7
        // (profiles/r02_ab_work_chunk.txt, second part).  Not for the (8, 4) shape (m > 512).
        if (!forced && !h->opt_early_exit_full_wg && (qbp::FUSED_MAX_THREADS / 2) / std::max(m, 1) >= 1 && S >= 2)
            S = (qbp::FUSED_MAX_THREADS / 2) / m;
        const long long spread = (B + h->num_cu - 1) / std::max(h->num_cu, 1);
        if (spread < S) S = (int)std::max<long long>(spread, 1);
    }
    S = std::min(S, std::max(1, qbp::FUSED_MAX_THREADS / std::max(m, 1)));
    if ((long long)S > B) S = (int)std::max<long long>(B, 1);
    cfg->dc = h->dc;
    cfg->slot_stride = h->r_stride;
    while (S > 1 && lds_bytes(h->dc, m, h->n, S) > 160 * 1024) --S;   // LDS-limited shapes
    // forced-iteration decode: the one-barrier kernel when two copies of the messages fit (the first one
    // below the constant offset of the second) without giving up a slot
    const bool two = forced && !mc && !h->opt_forced_two_barriers && h->dc == DC_SMALL &&
                     qbp::fused_r_doubles(h->r_stride, h->dv, S) * 8 <= (size_t)qbp::FUSED_R2_OFF_BYTES &&
                     lds_bytes(h->dc, m, h->n, S, true) <= 160 * 1024;
    cfg->one_barrier = two ? 1 : 0;
    h->last_one_barrier = cfg->one_barrier;
    cfg->S = S;
    cfg->threads = std::min(qbp::FUSED_MAX_THREADS, ((S * m + 63) / 64) * 64);
    // early exit: the first check step's messages as an LDS table, when it fits beside S slots
    const bool r0 = !forced && !h->opt_no_r0_table && lds_bytes(h->dc, m, h->n, S, false, true) <= 160 * 1024;
    cfg->r0_table = r0 ? 1 : 0;
    const size_t lds = lds_bytes(h->dc, m, h->n, S, two, r0);
    if (lds > 160 * 1024) return fail(QBP_E_UNSUPPORTED, "LDS need %zu B exceeds 160 KiB", lds);
    cfg->lds_bytes = (int)lds;
    int per_cu = h->opt_blocks_per_cu;
    if (per_cu <= 0) {
        // resident workgroups per CU: 16 wavefronts fit at the 128-VGPR budget; also LDS.  At least
        // two workgroups per CU are queued: with early exit the second round evens out the tail
        // (measured +10 % at p = 0.01, neutral when every syndrome runs max_iter iterations).
        const int waves = cfg->threads / 64;
        const int resident = std::max(1, std::min((qbp::FUSED_MAX_THREADS / 64) / std::max(waves, 1), (int)(160 * 1024 / lds)));
        per_cu = 2 * resident;
    }
    const long long want = (B + S - 1) / S;
    cfg->grid = (int)std::max<long long>(1, std::min<long long>(want, (long long)h->num_cu * per_cu));
    h->last_threads = cfg->threads;
    h->last_lds = cfg->lds_bytes;
    h->last_grid = cfg->grid;
    return QBP_OK;
}

int check_decode_args(qbp_handle* h, long long B, int max_iter, int variant)
{
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", B);
    if (max_iter < 1)
        return fail(QBP_E_INVALID, "max_iter must be >= 1 (got %d); the reference raises "
                                   "UnboundLocalError for maxIter=0", max_iter);
    if (variant < 0 || variant > 2) return fail(QBP_E_INVALID, "unknown variant %d", variant);
    return QBP_OK;
}

// The BP kernel of a call: 1 on-chip, 2 general-H, 3 streaming, or QBP_E_UNSUPPORTED when the on-chip kernel is
// forced on a matrix that does not fit it.  `B`: syndromes (trials) of the call; `col_mode`: resolve_column_order.
int bp_kernel(const qbp_handle* h, long long B, uint32_t flags, int col_mode, bool mc)
{
    const int forced = h->opt_force_generic ? 2 : h->opt_kernel;
    // Monte-Carlo: the streaming kernel has no such mode, and a matrix beyond the on-chip kernel runs the whole
    // loop inside the general-H kernel whatever was asked for
    if (mc) return forced == 2 || !h->fused_ok ? 2 : 1;
    if (forced == 1 && !h->fused_ok) return QBP_E_UNSUPPORTED;
    // automatic: the on-chip kernel when the matrix fits; otherwise one workgroup per syndrome (general-H), except
    // for small graphs in batches that fill the chip with one LANE per syndrome, where the streaming kernel is ahead
    // (tools/bench_generic.py: [[288,12,18]], 262144 syndromes: 3.7e6 against 2.6e6 /s; larger graphs keep their
    // messages in L2 / Infinity Cache under the general-H kernel and win there at every batch size measured)
    int kernel = forced ? forced : h->fused_ok ? 1 : (B >= 131072 && h->E <= 2048) ? 3 : 2;
    // numpy's pairwise column sums only differ from 8 entries per column on; those matrices never
    // fit the on-chip kernel, and only the general-H kernel implements that order
    if ((flags & QBP_FLAG_PAIRWISE_COLSUM) && h->max_col_deg >= 8) kernel = 2;
    if (col_mode == 2) kernel = 2;           // two column orders in one launch: the general-H kernel only
    return kernel;
}

// Column-sum order of a decode call (include/qbp.h, QBP_FLAG_DENSE_F_COLSUM*): clears the two flag bits and
// sets *f_order when the launch has to use the Fortran-order tables (built and uploaded at the first such call).
int resolve_column_order(qbp_handle* h, unsigned& flags, const double* host_prior, int* mode)
{
    *mode = 0;                               // 0 row by row, 1 Fortran order, 2 Fortran order at iteration 0 only
    const unsigned want = flags & (QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0);
    flags &= ~(QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0);
    if (!want) return QBP_OK;
    if (want == (QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0) || (flags & QBP_FLAG_PAIRWISE_COLSUM))
        return fail(QBP_E_INVALID, "at most one column-sum order flag per call");
    if (want == QBP_FLAG_DENSE_F_COLSUM_ITER0 && host_prior) {
        // Iteration 0 does not depend on the order when all of a column's messages have the same magnitude r
        // -- equal priors on every edge and checks of equal weight -- and a column has at most three of them:
        // every partial sum is k r with |k| <= 3, and k r is exact for |k| <= 2 and rounded once, from the
        // exact value, for |k| = 3.  That is the reference's own use (rework/Alvarado.py, rework/main.py:
        // uniform priors on the code files' Hx) and needs no second table set in the launch.
        bool same = h->max_col_deg <= 3;
        const int d0 = h->m > 0 ? h->row_ptr[1] - h->row_ptr[0] : 0;
        for (int c = 0; same && c < h->m; ++c) same = (h->row_ptr[c + 1] - h->row_ptr[c]) == d0;
        if (same && h->E > 0) {
            const double p0 = host_prior[h->col_idx[0]];
            for (int e = 0; same && e < h->E; ++e) same = host_prior[h->col_idx[e]] == p0;
        }
        if (same) return QBP_OK;             // = row-by-row tables
    }
    auto& F = h->f_order;
    if (F.state == 0) {
        HostTables T;
        const int rc = build_tables(h->row_ptr.data(), h->col_idx.data(), h->m, h->n, T, 1);
        if (rc == QBP_E_UNSUPPORTED) { F.state = -1; return rc; }
        if (rc) return rc;
        if (T.fused_ok) {
            HIP_TRY(F.tab_gather.upload(T.tab_gather));
            HIP_TRY(F.tab_store.upload(T.tab_store));
            HIP_TRY(F.tab_writer.upload(T.tab_writer));
        }
        HIP_TRY(F.col_edge.upload(T.col_edge));
        HIP_TRY(F.sedge.upload(T.sedge));
        HIP_TRY(F.vpos.upload(T.vpos));
        HIP_TRY(F.vrow.upload(T.vrow));
        F.state = 1;
    }
    if (F.state < 0)
        return fail(QBP_E_UNSUPPORTED, "the Fortran-order column sums of this matrix are not a left-to-right sum");
    *mode = want == QBP_FLAG_DENSE_F_COLSUM ? 1 : 2;
    return QBP_OK;
}

}  // namespace

// Launch geometry of the general-H kernel (one workgroup per syndrome at a time):
//   messages in LDS when they fit (16 E bytes + bookkeeping <= 160 KiB), else in a global workspace;
//   threads per workgroup: the checks of weight <= 8 in as few, as full passes as possible
//   (864 checks: 896 threads, one pass; 2592: 896 threads, three passes), at most 1024;
//   workgroups per CU: as many as fit 16 wavefronts (the kernel's 128-register budget) and the LDS.
struct GenericGeom { bool lds_msgs, lds_tables; int mem, r_split, threads, per_cu, grid; size_t lds; };

// inplace: sum-product without damping keeps one message array (qbp_generic.hpp): 8 E bytes instead of 16 E
// extra_lds: bytes the launch needs behind everything else (qbp_mc_run_budgets: the counter rows), part of g.lds
static GenericGeom generic_geometry(const qbp_handle* h, long long B, bool inplace, size_t extra_lds = 0)
{
    GenericGeom g{};
    const int E1 = std::max(h->E, 1);
    const size_t LDS_MAX = (size_t)160 * 1024 - extra_lds;
    g.lds_msgs = qbp::generic_lds_bytes(h->m, E1, h->n, true, false, 0, inplace) <= LDS_MAX && h->opt_mem == 0;
    // the variable step's tables (prior, message positions) in LDS too when one workgroup per CU is
    // the geometry anyway and they fit beside (or instead of) the messages
    g.lds_tables = false;
    g.lds = qbp::generic_lds_bytes(h->m, E1, h->n, g.lds_msgs, false, 0, inplace);
    const int short_rows = std::max(1, h->row_off[qbp::GENERIC_MAX_ROW_CLASS + 1] - h->row_off[1]);
    const int work = std::max(h->rpad_off[qbp::GENERIC_MAX_ROW_CLASS + 1], 64);    // padded work items
    const int passes = (work + 1023) / 1024;
    int threads = (((work + passes - 1) / passes) + 63) / 64 * 64;
    int per_cu = std::max(1, 1024 / threads);
    if (g.lds) per_cu = (int)std::min<size_t>((size_t)per_cu, std::max<size_t>(1, ((size_t)160 * 1024) / (g.lds + extra_lds)));
    per_cu = std::min(per_cu, 8);
    // batches that cannot fill the chip: one wide workgroup per syndrome (latency of a single decode)
    if (B < (long long)h->num_cu * per_cu) {
        per_cu = 1;
        const int wide = std::max(std::max(short_rows, h->n / 2), 64);
        threads = std::min(1024, (wide + 63) / 64 * 64);
    }
    // messages in global memory: the variable step is bound by L2 / Infinity-Cache traffic, and more
    // threads per syndrome is what puts more of it in flight (2592 x 7776: 1.89e5 syndromes/s with 1024
    // threads against 1.72e5 with 896, the check step's exact fit)
    if (!g.lds_msgs && B >= (long long)h->num_cu) threads = 1024;
    if (h->opt_threads > 0) threads = std::min(1024, (h->opt_threads + 63) / 64 * 64);
    if (h->opt_blocks_per_cu > 0) per_cu = h->opt_blocks_per_cu;
    g.mem = g.lds_msgs ? qbp::GENERIC_MEM_LDS : qbp::GENERIC_MEM_GLOBAL;
    g.r_split = 0;
    if (h->opt_mem == 2) per_cu = 1;
    if (!g.lds_msgs && per_cu == 1 && !h->opt_no_r_split && h->opt_mem != 1) {
        // the messages do not fit: as much of R as the LDS holds (the rest, and Q, in the workspace)
        const size_t room = LDS_MAX - qbp::generic_lds_bytes(h->m, E1, h->n, false, false);
        int K = (int)std::min<size_t>((size_t)E1, room / 8);
        if (h->opt_mem == 2) K = std::min(K, std::max(1, E1 / 2));     // (tests: both sides of the split in use)
        if (K >= E1 / 4) { g.mem = qbp::GENERIC_MEM_SPLIT; g.r_split = K; }
        g.lds = qbp::generic_lds_bytes(h->m, E1, h->n, false, false, g.r_split);
    }
    if (per_cu == 1 && !h->opt_no_lds_tables && g.mem != qbp::GENERIC_MEM_SPLIT &&
        qbp::generic_lds_bytes(h->m, E1, h->n, g.lds_msgs, true, g.r_split, inplace) <= LDS_MAX) {
        g.lds_tables = true;
        g.lds = qbp::generic_lds_bytes(h->m, E1, h->n, g.lds_msgs, true, g.r_split, inplace);
    }
    g.lds += extra_lds;
    g.threads = threads; g.per_cu = per_cu;
    g.grid = (int)std::max<long long>(1, std::min<long long>(B, (long long)h->num_cu * per_cu));
    return g;
}

// Monte-Carlo arguments of a BP launch (the on-chip and general-H kernels read the same fields).
struct McArgs {
    const unsigned long long* lx_cols;
    long long trial_begin;
    unsigned long long seed;
    unsigned threshold;
    const uint32_t* thr_cols;        // per-column thresholds (qbp_mc_run_probs), else null
    int draws, half_distance;
    long long* counters;
    const uint8_t* errors_in;
    // failure records for the OSD pass (QBP_FLAG_OSD0), else null
    long long* fail_list;
    unsigned long long* fail_count;
    uint8_t *fail_syn, *fail_hard, *fail_err;
    double* fail_llr;
    // qbp_mc_run_budgets: the ladder (host array), else 0 / null
    int n_budgets;
    const int32_t* budgets;
    // qbp_mc_run_spectrum: the two tables (iter_hist may be null), else null
    long long* spectrum;
    long long* iter_hist;
    // qbp_decode_shots: recorded detection events instead of a sampler, predictions out (BpCall::converged too)
    const uint8_t* det_bits;
    int det_row_bytes;
    const unsigned long long* actual;
    unsigned long long* predictions;
    // qbp_mc_run_llr_hist (a ladder too): the table, the edges on the device and their number - 1, else null / 0
    long long* llr_hist;
    const double* llr_edges;
    int llr_bins;
    size_t llr_lds() const { return llr_hist ? qbp::llr_hist_lds_bytes(n_budgets, llr_bins) : 0; }
};

template <typename Params>
static void put_mc(Params& P, const McArgs& a)
{
    P.lx_cols = a.lx_cols; P.trial_begin = a.trial_begin; P.seed = a.seed; P.threshold = a.threshold;
    P.draws = a.draws; P.half_distance = a.half_distance; P.counters = a.counters; P.errors_in = a.errors_in;
    P.thr_cols = a.thr_cols;
    P.fail_list = a.fail_list; P.fail_count = a.fail_count; P.fail_syn = a.fail_syn;
    P.fail_llr = a.fail_llr; P.fail_hard = a.fail_hard; P.fail_err = a.fail_err;
    P.n_budgets = a.n_budgets;
    for (int j = 0; j < a.n_budgets; ++j) P.budgets[j] = a.budgets[j];
    P.spectrum = a.spectrum; P.iter_hist = a.iter_hist;
    P.det_bits = a.det_bits; P.det_row_bytes = a.det_row_bytes; P.actual = a.actual; P.predictions = a.predictions;
    P.llr_hist = a.llr_hist; P.llr_edges = a.llr_edges; P.llr_bins = a.llr_bins;
}

// Per-call arguments of a BP launch, whichever kernel runs it (device pointers; outputs may be null).
struct BpCall {
    const uint8_t* syndromes = nullptr;
    const double* prior = nullptr;
    long long B = 0;
    int max_iter = 0, variant = 0;
    double alpha = 1.0, damping = 1.0, clip_llr = 0.0;
    unsigned flags = 0;
    uint8_t* hard = nullptr;
    uint8_t* converged = nullptr;
    int32_t* iters = nullptr;
    double* llr = nullptr;
    double* dump = nullptr;                  // message dump (general-H kernel only)
    int dump_iter = 0;
    double dump_div = 1.0;
    int col_mode = 0;                        // resolve_column_order
    const McArgs* mc = nullptr;              // Monte-Carlo launch
};

static int generic_launch(qbp_handle* h, const BpCall& c, hipStream_t s)
{
    if ((c.flags & QBP_FLAG_PAIRWISE_COLSUM) && h->max_col_deg > qbp::GENERIC_PAIRWISE_MAX_COL)
        return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_PAIRWISE_COLSUM supports column weights up to %d (got %d)",
                    qbp::GENERIC_PAIRWISE_MAX_COL, h->max_col_deg);
    // one launch hands out its syndromes through a 32-bit counter
    constexpr long long MAX_LAUNCH = (long long)1 << 30;
    if (c.B > MAX_LAUNCH) {
        if (!c.mc)
            return fail(QBP_E_UNSUPPORTED, "the general-H kernel decodes at most 2^30 syndromes per call (got %lld)",
                        c.B);
        for (long long off = 0; off < c.B; off += MAX_LAUNCH) {     // Monte-Carlo: trial ranges of any length
            McArgs mc = *c.mc;
            mc.trial_begin += off;
            BpCall part = c;
            part.B = std::min(MAX_LAUNCH, c.B - off);
            part.mc = &mc;
            const int rc = generic_launch(h, part, s);
            if (rc) return rc;
        }
        return QBP_OK;
    }
    const long long B = c.B;
    const int variant = c.variant, col_mode = c.col_mode;
    const size_t E = (size_t)std::max(h->E, 1), n = (size_t)h->n;
    const bool inplace = QBP_GENERIC_INPLACE != 0 && variant == QBP_SUM_PRODUCT;
    // (qbp_mc_run_budgets: the workgroup's 2 * n_budgets counter rows behind everything else in LDS)
    const size_t budget_lds = c.mc ? (size_t)2 * c.mc->n_budgets * qbp::NUM_COUNTERS * 4 : 0;
    // (qbp_mc_run_spectrum: its residual-weight word and iteration histogram, likewise)
    const size_t spectrum_lds = c.mc && c.mc->spectrum ? (((size_t)c.max_iter + 2) * 4 + 7) & ~(size_t)7 : 0;
    // (qbp_mc_run_llr_hist: its table, likewise -- bytes that a split R then leaves to it)
    // (its doubles need an 8-byte boundary, which the tables in front of it -- 4 E bytes of positions -- may miss)
    const size_t llr_lds = c.mc && c.mc->llr_hist ? c.mc->llr_lds() + 8 : 0;
    const GenericGeom g = generic_geometry(h, B, inplace, budget_lds + spectrum_lds + llr_lds);
    if (g.lds > (size_t)160 * 1024)
        return fail(QBP_E_UNSUPPORTED, "m = %d checks need %zu B of LDS for the parity bits (limit 160 KiB)",
                    h->m, g.lds);
    if (!g.lds_msgs) {
        if (!inplace) HIP_TRY(h->d_wsQ.reserve((size_t)g.grid * E));
        HIP_TRY(h->d_wsR.reserve((size_t)g.grid * E));
    }
    if (inplace) HIP_TRY(h->d_wsV.reserve((size_t)g.grid * n));
    HIP_TRY(h->d_prior_sorted.reserve(n));
    HIP_TRY(qbp::launch_permute_prior(c.prior, h->d_svar.p, h->d_prior_sorted.p, (int)n, s));
    qbp::GenericParams G{};
    G.m = h->m; G.n = h->n; G.E = h->E;
    G.srow = h->d_srow.p; G.srow_e0 = h->d_srow_e0.p; G.srow_deg = h->d_srow_deg.p;
    G.col_idx = h->d_col_idx.p; G.epos = h->d_epos.p;
    G.long_edge_row = h->d_long_edge_row.p;
    {
        const size_t n_long = (size_t)(h->row_off[qbp::GENERIC_MAX_ROW_CLASS + 2] - h->row_off[qbp::GENERIC_MAX_ROW_CLASS + 1]);
        HIP_TRY(h->d_wsL.reserve((size_t)g.grid * 3 * std::max<size_t>(n_long, 1)));
        G.wsL = h->d_wsL.p;
    }
    std::copy(std::begin(h->row_off), std::end(h->row_off), G.row_off);
    std::copy(std::begin(h->row_base), std::end(h->row_base), G.row_base);
    G.svar = h->d_svar.p; G.lcol_ptr = h->d_lcol_ptr.p;
    G.vpos = col_mode == 1 ? h->f_order.vpos.p : h->d_vpos.p;
    G.vrow = col_mode == 1 ? h->f_order.vrow.p : h->d_vrow.p;
    G.vpos0 = col_mode == 2 ? h->f_order.vpos.p : nullptr;      // Fortran order at iteration 0 only
    G.vrow0 = col_mode == 2 ? h->f_order.vrow.p : nullptr;
    std::copy(std::begin(h->col_off), std::end(h->col_off), G.col_off);
    std::copy(std::begin(h->gcol_base), std::end(h->gcol_base), G.col_base);
    std::copy(std::begin(h->rpad_off), std::end(h->rpad_off), G.rpad_off);
    std::copy(std::begin(h->cpad_off), std::end(h->cpad_off), G.cpad_off);
    G.prior_sorted = h->d_prior_sorted.p;
    G.lds_tables = g.lds_tables ? 1 : 0;
    G.r_split = g.r_split;
    G.syndromes = c.syndromes; G.B = B; G.max_iter = c.max_iter; G.flags = c.flags;
    G.alpha = c.alpha; G.damping = c.damping; G.clip_llr = c.clip_llr;
    G.hard = c.hard; G.converged = c.converged; G.iters = c.iters; G.llr = c.llr;
    G.wsQ = h->d_wsQ.p; G.wsR = h->d_wsR.p; G.wsV = h->d_wsV.p;
    G.work_counter = h->d_work_counter.p;
    if (B > (long long)g.grid)     // (else every index it can yield is >= B whatever it holds)
        HIP_TRY(hipMemsetAsync(h->d_work_counter.p, 0, sizeof(unsigned long long), s));
    G.dump_R = c.dump; G.dump_iter = c.dump_iter; G.dump_div = c.dump_div;
    h->last_threads = g.threads; h->last_lds = (int)g.lds; h->last_grid = g.grid;
    if (c.mc) {
        // Monte-Carlo mode: per-workgroup scratch for the sampled error (none with recorded shots)
        if (!c.mc->det_bits) HIP_TRY(h->d_wsE.reserve((size_t)g.grid * ((n + 3) / 4) * 4));
        put_mc(G, *c.mc);
        G.wsE = h->d_wsE.p;
        G.budget_tab_off = (int)(g.lds - budget_lds - spectrum_lds - llr_lds);
        G.spectrum_off = (int)(g.lds - spectrum_lds - llr_lds);
        G.llr_hist_off = (int)((g.lds - llr_lds + 7) & ~(size_t)7);
    }
    HIP_TRY(qbp::launch_generic(c.mc != nullptr, g.mem, variant, G, g.grid, g.threads, g.lds, s));
    return QBP_OK;
}

// OSD fits the one-wavefront kernel: the matrix rows in 64 KiB of LDS, and a lane tracks its rows in a 32-bit mask.
static bool osd_one_wave(const qbp_handle* h)
{
    return qbp::osd_lds_bytes(h->m, h->n, h->osd_W, h->osd_NP) <= 64 * 1024 && h->m <= 64 * 32;
}

// The rows of H bit-packed into osd_W 32-bit words each (d_hbits, read by every OSD kernel) and the rank of H over
// GF(2) (Gaussian elimination on the host, once per code): the elimination loop of the kernels can stop as soon
// as that many pivots are found.  qbp_create builds them for the one-wavefront kernel; matrices beyond it build
// them on first use (about half a second for 2592 x 7776), which most users of such matrices never make.
static int osd_prepare(qbp_handle* h)
{
    if (h->osd_ready) return QBP_OK;
    const int m = h->m, n = h->n, W = h->osd_W;
    std::vector<uint32_t> hbits((size_t)m * W, 0u);
    for (int c = 0; c < m; ++c)
        for (int e = h->row_ptr[c]; e < h->row_ptr[c + 1]; ++e)
            hbits[(size_t)c * W + (h->col_idx[e] >> 5)] |= 1u << (h->col_idx[e] & 31);
    HIP_TRY(h->d_hbits.upload(hbits));
    std::vector<uint32_t> A = hbits;
    int rank = 0;
    for (int col = 0; col < n && rank < m; ++col) {
        const int wi = col >> 5;
        const uint32_t bit = 1u << (col & 31);
        int piv = -1;
        for (int r = rank; r < m; ++r) if (A[(size_t)r * W + wi] & bit) { piv = r; break; }
        if (piv < 0) continue;
        // (rows rank.. are zero left of `col`)
        if (piv != rank) for (int w = wi; w < W; ++w) std::swap(A[(size_t)piv * W + w], A[(size_t)rank * W + w]);
        for (int r = rank + 1; r < m; ++r)
            if (A[(size_t)r * W + wi] & bit)
                for (int w = wi; w < W; ++w) A[(size_t)r * W + w] ^= A[(size_t)rank * W + w];
        ++rank;
    }
    h->osd_rank = rank;
    h->osd_ready = true;
    return QBP_OK;
}

extern "C" {

const char* qbp_last_error(void) { return g_err; }
const char* qbp_version(void) { return "qbp 0.1 (gfx950)"; }

int qbp_create(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n,
               int32_t device, qbp_handle** out)
try {
    if (!out) return fail(QBP_E_INVALID, "out is null");
    *out = nullptr;
    HostTables T;
    int rc0 = build_tables(row_ptr, col_idx, m, n, T);
    if (rc0) return rc0;
    const int E = row_ptr[m];
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev <= 0)
        return fail(QBP_E_NO_DEVICE, "no HIP device available (%s); libqbp has no CPU fallback",
                    de == hipSuccess ? "device count 0" : hipGetErrorString(de));
    if (device < 0 || device >= ndev)
        return fail(QBP_E_NO_DEVICE, "device %d out of range (have %d)", device, ndev);
    DeviceScope on_device(device);
    HIP_TRY(on_device.err);

    struct Guard {                       // destroys a half-built handle on every early exit
        qbp_handle* h;
        ~Guard() { if (h) qbp_destroy(h); }
    } guard{new qbp_handle()};
    qbp_handle* h = guard.h;
    h->device = device; h->m = m; h->n = n; h->E = E;
    h->row_ptr.assign(row_ptr, row_ptr + m + 1);
    h->col_idx.assign(col_idx, col_idx + E);
    h->max_row_deg = T.max_row;
    h->max_col_deg = T.max_col;
    h->dc = T.dc; h->dv = T.dv; h->fused_ok = T.fused_ok; h->padded = T.padded; h->r_stride = T.r_stride;
    h->n_iso = (int)T.iso.size();
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    h->num_cu = prop.multiProcessorCount;

    if (T.fused_ok) {
        HIP_TRY(h->d_tab_var.upload(T.tab_var));
        HIP_TRY(h->d_tab_gather.upload(T.tab_gather));
        HIP_TRY(h->d_tab_store.upload(T.tab_store));
        HIP_TRY(h->d_tab_writer.upload(T.tab_writer));
    }
    HIP_TRY(h->d_iso.upload(T.iso));
    HIP_TRY(h->d_col_ptr.upload(T.col_ptr));
    HIP_TRY(h->d_col_edge.upload(T.col_edge));
    HIP_TRY(h->d_epos.upload(T.epos));
    HIP_TRY(h->d_cpos.upload(T.cpos));
    HIP_TRY(h->d_long_edge_row.upload(T.long_edge_row));
    HIP_TRY(h->d_vpos.upload(T.vpos));
    HIP_TRY(h->d_vrow.upload(T.vrow));
    HIP_TRY(h->d_lcol_ptr.upload(T.lcol_ptr));
    std::copy(std::begin(T.gcol_base), std::end(T.gcol_base), h->gcol_base);
    {   // work items of the general-H kernel: every weight class padded to whole wavefronts
        int off = 0;
        for (int k = 1; k <= qbp::GENERIC_MAX_ROW_CLASS; ++k) {
            h->rpad_off[k] = off;
            off += (T.row_off[k + 1] - T.row_off[k] + 63) / 64 * 64;
        }
        h->rpad_off[qbp::GENERIC_MAX_ROW_CLASS + 1] = off;
        off = 0;
        for (int k = 1; k <= qbp::GENERIC_MAX_COL_CLASS; ++k) {
            h->cpad_off[k] = off;
            off += (T.col_off[k + 1] - T.col_off[k] + 63) / 64 * 64;
        }
        h->cpad_off[qbp::GENERIC_MAX_COL_CLASS + 1] = off;
    }
    std::copy(std::begin(T.row_base), std::end(T.row_base), h->row_base);
    HIP_TRY(h->d_srow.upload(T.srow));
    HIP_TRY(h->d_srow_e0.upload(T.srow_e0));
    HIP_TRY(h->d_srow_deg.upload(T.srow_deg));
    HIP_TRY(h->d_svar.upload(T.svar));
    HIP_TRY(h->d_sedge.upload(T.sedge));
    std::copy(std::begin(T.row_off), std::end(T.row_off), h->row_off);
    std::copy(std::begin(T.col_off), std::end(T.col_off), h->col_off);
    std::copy(std::begin(T.col_edge_base), std::end(T.col_edge_base), h->col_edge_base);
    HIP_TRY(h->d_row_ptr.upload(h->row_ptr));
    HIP_TRY(h->d_col_idx.upload(h->col_idx));
    // OSD: 32-bit words per row of H, radix-sort size; its GF(2) tables now when the one-wavefront kernel takes it
    h->osd_W = (n + 31) / 32;
    h->osd_NP = 1;
    while (h->osd_NP < n) h->osd_NP <<= 1;
    h->osd_lds = (int)((qbp::osd_lds_bytes(m, n, h->osd_W, h->osd_NP) + 15) & ~(size_t)15);
    h->osd_ok = osd_one_wave(h);
    if (h->osd_ok) {
        const int rc = osd_prepare(h);
        if (rc) return rc;
    }
    HIP_TRY(h->d_work_counter.reserve(1));
    HIP_TRY(hipMemset(h->d_work_counter.p, 0, sizeof(unsigned long long)));
    HIP_TRY(h->d_fail_count.reserve(1));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    guard.h = nullptr;
    *out = h;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_plan(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, int32_t info[8],
             int32_t* tab_var, uint16_t* tab_nbr, uint32_t* tab_writer)
try {
    HostTables T;
    int rc = build_tables(row_ptr, col_idx, m, n, T, 0, tab_nbr != nullptr);
    if (rc) return rc;
    if (info) {
        info[0] = T.fused_ok ? 1 : 2; info[1] = T.dc; info[2] = T.dv; info[3] = T.max_row;
        info[4] = T.max_col; info[5] = (int32_t)T.iso.size(); info[6] = T.padded ? 1 : 0;
        info[7] = T.fused_ok ? (int32_t)fused_lds_bytes(T.dc, m, n, 1, T.r_stride) : 0;
    }
    if (T.fused_ok) {
        if (tab_var) std::memcpy(tab_var, T.tab_var.data(), T.tab_var.size() * sizeof(int32_t));
        if (tab_nbr) std::memcpy(tab_nbr, T.tab_nbr.data(), T.tab_nbr.size() * sizeof(uint16_t));
        if (tab_writer) std::memcpy(tab_writer, T.tab_writer.data(), T.tab_writer.size() * sizeof(uint32_t));
    }
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_plan_r_layout(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, int32_t col_order,
                      int32_t S, int32_t info[8], uint16_t* tab_gather, uint16_t* tab_store)
try {
    HostTables T;
    int rc = build_tables(row_ptr, col_idx, m, n, T, col_order);
    if (rc) return rc;
    if (!T.fused_ok) return fail(QBP_E_UNSUPPORTED, "the matrix does not run on the on-chip kernel");
    if (S < 1 || (long long)S * m > qbp::FUSED_MAX_THREADS)
        return fail(QBP_E_INVALID, "S = %d slots of %d checks are not a workgroup", S, m);
    if (info) {
        const size_t one = fused_lds_bytes(T.dc, m, n, S, T.r_stride), two = fused_lds_bytes(T.dc, m, n, S, T.r_stride, true);
        const size_t copy = qbp::fused_r_doubles(T.r_stride, T.dv, S);
        info[0] = T.dv; info[1] = T.r_stride; info[2] = (int32_t)copy;
        info[3] = one <= 160 * 1024 ? (int32_t)one : 0;
        info[4] = T.dc == DC_SMALL && copy * 8 <= (size_t)qbp::FUSED_R2_OFF_BYTES && two <= 160 * 1024 ? (int32_t)two : 0;
        info[5] = qbp::FUSED_R2_OFF_BYTES; info[6] = qbp::NP_LDS_BYTES; info[7] = 0;
    }
    if (tab_gather) std::memcpy(tab_gather, T.tab_gather.data(), T.tab_gather.size() * sizeof(uint16_t));
    if (tab_store) std::memcpy(tab_store, T.tab_store.data(), T.tab_store.size() * sizeof(uint16_t));
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_column_order(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, int32_t col_order,
                     int32_t* col_ptr, int32_t* col_edge)
try {
    HostTables T;
    int rc = build_tables(row_ptr, col_idx, m, n, T, col_order);
    if (rc) return rc;
    if (col_ptr) std::memcpy(col_ptr, T.col_ptr.data(), ((size_t)n + 1) * sizeof(int32_t));
    if (col_edge && row_ptr[m] > 0) std::memcpy(col_edge, T.col_edge.data(), (size_t)row_ptr[m] * sizeof(int32_t));
    return QBP_OK;
}
QBP_ABI_CATCH

void qbp_destroy(qbp_handle* h)
{
    if (!h) return;
    DeviceScope on_device(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    if (h->pin_host) (void)hipHostFree(h->pin_host);
    for (int i = 0; i < 2; ++i) {
        if (h->stage[i]) (void)hipHostFree(h->stage[i]);
        if (h->stage_ev[i]) (void)hipEventDestroy(h->stage_ev[i]);
    }
    delete h;                          // (the device buffers free themselves, on this device)
}

static int stream_launch(qbp_handle* h, const BpCall& c, hipStream_t s)
{
    // streaming kernel: one lane per syndrome, messages [edge][syndrome] in a global workspace;
    // long batches go through in chunks that keep the workspace under 16 GiB
    const long long B = c.B;
    const bool f_order = c.col_mode == 1;
    const size_t E = (size_t)std::max(h->E, 1), n = (size_t)h->n, m = (size_t)h->m;
    const size_t per_lane = 2 * E * sizeof(double) + n + m;
    long long Bc = (long long)std::min<unsigned long long>(((unsigned long long)16 << 30) / per_lane,
                                                          (unsigned long long)B);
    Bc = std::max<long long>(256, (Bc + 255) / 256 * 256);
    const size_t msg_doubles = (size_t)Bc * E;
    HIP_TRY(h->d_wsQ.reserve(msg_doubles));
    HIP_TRY(h->d_wsR.reserve(msg_doubles));
    HIP_TRY(h->d_wsC.reserve((size_t)Bc * n));
    HIP_TRY(h->d_wsS.reserve((size_t)Bc * m));
    qbp::StreamParams P{};
    P.m = h->m; P.n = h->n; P.E = h->E;
    P.syndromes = c.syndromes; P.B = B; P.Bc = Bc;
    P.max_iter = c.max_iter; P.flags = c.flags; P.alpha = c.alpha; P.damping = c.damping; P.clip_llr = c.clip_llr;
    P.hard = c.hard; P.converged = c.converged; P.iters = c.iters; P.llr = c.llr;
    P.Q = h->d_wsQ.p; P.R = h->d_wsR.p; P.cand = h->d_wsC.p; P.synT = h->d_wsS.p;
    std::copy(std::begin(h->row_off), std::end(h->row_off), P.row_off);
    std::copy(std::begin(h->col_off), std::end(h->col_off), P.col_off);
    std::copy(std::begin(h->col_edge_base), std::end(h->col_edge_base), P.col_edge_base);
    for (long long b0 = 0; b0 < B; b0 += Bc) {
        P.b0 = b0;
        const long long lanes = std::min<long long>(Bc, B - b0);
        const unsigned grid = (unsigned)((lanes + 255) / 256);
        h->last_threads = 256; h->last_lds = 0; h->last_grid = (int)grid;
        HIP_TRY(qbp::launch_stream(c.variant, grid, P, h->d_col_idx.p, h->d_col_ptr.p,
                                   f_order ? h->f_order.col_edge.p : h->d_col_edge.p, c.prior,
                                   h->d_srow.p, h->d_srow_e0.p, h->d_srow_deg.p, h->d_svar.p,
                                   f_order ? h->f_order.sedge.p : h->d_sedge.p, s));
    }
    return QBP_OK;
}

static int fused_launch(qbp_handle* h, const BpCall& c, hipStream_t s)
{
    const bool mc = c.mc != nullptr, f_order = c.col_mode == 1;
    LaunchCfg cfg;
    int rc = make_cfg(h, c.B, &cfg, (c.flags & QBP_FLAG_FORCE_FULL) != 0, mc, mc ? c.mc->n_budgets : 0,
                      mc && c.mc->spectrum ? c.max_iter + 1 : 0, mc ? c.mc->llr_lds() : 0);
    if (rc) return rc;
    FusedParams P{};
    P.m = h->m; P.n = h->n;
    P.S = cfg.S; P.slot_stride = cfg.slot_stride;
    P.r0_table = cfg.r0_table;
    P.padded = h->padded ? 1 : 0;
    P.n_words4 = (h->n + 3) / 4;
    P.tab_var = h->d_tab_var.p;
    P.tab_gather = f_order ? h->f_order.tab_gather.p : h->d_tab_gather.p;
    P.tab_store = f_order ? h->f_order.tab_store.p : h->d_tab_store.p;
    P.tab_writer = f_order ? h->f_order.tab_writer.p : h->d_tab_writer.p;
    P.iso_vars = h->d_iso.p; P.n_iso = h->n_iso;
    P.work_counter = h->d_work_counter.p;
    P.syndromes = c.syndromes; P.prior = c.prior; P.B = c.B;
    P.max_iter = c.max_iter; P.flags = c.flags;
    P.alpha = c.alpha; P.damping = c.damping; P.clip_llr = c.clip_llr;
    P.hard = c.hard; P.converged = c.converged; P.iters = c.iters; P.llr = c.llr;
    if (mc) put_mc(P, *c.mc);
    // The work counter hands out syndromes beyond the first one of each slot; when every syndrome
    // is some slot's first one (small decode calls) its value is irrelevant -- any index it yields is
    // >= B -- and the memset node is skipped (3 us of a 30 us single-syndrome call).
    if (mc || c.B > (long long)cfg.grid * cfg.S)
        HIP_TRY(hipMemsetAsync(h->d_work_counter.p, 0, sizeof(unsigned long long), s));
    const bool fast = (c.flags & QBP_FLAG_FAST_MATH) != 0;
    if (mc && P.det_bits)               // recorded shots (qbp_decode_shots): builds of their own
        HIP_TRY(fast ? qbp::launch_fused_shots_fast_math(mc, c.variant, P, cfg, s)
                     : qbp::launch_fused_shots(mc, c.variant, P, cfg, s));
    else if (mc && P.llr_hist)          // posterior-LLR histograms per budget (qbp_mc_run_llr_hist): builds of their own
        HIP_TRY(fast ? qbp::launch_fused_llrhist_fast_math(mc, c.variant, P, cfg, s)
                     : qbp::launch_fused_llrhist(mc, c.variant, P, cfg, s));
    else if (mc && P.spectrum)          // residual-weight and iteration tables (qbp_mc_run_spectrum): builds of their own
        HIP_TRY(fast ? qbp::launch_fused_spectrum_fast_math(mc, c.variant, P, cfg, s)
                     : qbp::launch_fused_spectrum(mc, c.variant, P, cfg, s));
    else if (mc && P.n_budgets)         // a ladder of iteration budgets (qbp_mc_run_budgets): builds of their own
        HIP_TRY(fast ? qbp::launch_fused_budgets_fast_math(mc, c.variant, P, cfg, s)
                     : qbp::launch_fused_budgets(mc, c.variant, P, cfg, s));
    else if (mc && P.thr_cols)          // a sampler threshold per qubit (qbp_mc_run_probs): builds of their own
        HIP_TRY(fast ? qbp::launch_fused_cols_fast_math(mc, c.variant, P, cfg, s)
                     : qbp::launch_fused_cols(mc, c.variant, P, cfg, s));
    else
        HIP_TRY(fast ? qbp::launch_fused_fast_math(mc, c.variant, P, cfg, s)
                     : qbp::launch_fused(mc, c.variant, P, cfg, s));
    return QBP_OK;
}

// (layered BP, defined with its configuration further down)
static int check_layered_flags(const qbp_handle* h, uint32_t flags, int variant, bool other_entry);
static int layered_launch(qbp_handle* h, const BpCall& c, hipStream_t s);
// (fixed-point min-sum, likewise)
static int check_quant_flags(const qbp_handle* h, uint32_t flags, int variant, bool other_entry);
static int quant_launch(qbp_handle* h, const BpCall& c, int32_t* posterior_q, hipStream_t s);

int qbp_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior,
                            int64_t B, int32_t max_iter, int32_t variant, double alpha,
                            double damping, double clip_llr, uint32_t flags, uint8_t* d_hard,
                            uint8_t* d_converged, int32_t* d_iters, double* d_llr, void* stream)
try {
    int rc = check_decode_args(h, B, max_iter, variant);
    if (rc) return rc;
    if ((rc = check_layered_flags(h, flags, variant, false)) != QBP_OK) return rc;
    if ((rc = check_quant_flags(h, flags, variant, true)) != QBP_OK) return rc;
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_prior) return fail(QBP_E_INVALID, "null input pointer");
    if (B > (int64_t)1 << 40) return fail(QBP_E_INVALID, "B too large");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & QBP_FLAG_LAYERED) {
        // the layered schedule: a kernel of its own (QBP_FLAG_FAST_MATH is ignored)
        BpCall c;
        c.syndromes = d_syndromes; c.prior = d_prior; c.B = B; c.max_iter = max_iter; c.variant = variant;
        c.alpha = alpha; c.clip_llr = clip_llr; c.flags = flags & QBP_FLAG_FORCE_FULL;
        c.hard = d_hard; c.converged = d_converged; c.iters = d_iters; c.llr = d_llr;
        h->last_kernel = 4;
        return layered_launch(h, c, s);
    }
    BpCall c;
    rc = resolve_column_order(h, flags, nullptr, &c.col_mode);
    if (rc) return rc;
    const int kernel = bp_kernel(h, B, flags, c.col_mode, false);
    if (kernel < 0) return fail(kernel, "H does not fit the on-chip kernel");
    h->last_kernel = kernel;
    c.syndromes = d_syndromes; c.prior = d_prior; c.B = B; c.max_iter = max_iter; c.variant = variant;
    c.alpha = alpha; c.damping = damping; c.clip_llr = clip_llr; c.flags = flags;
    c.hard = d_hard; c.converged = d_converged; c.iters = d_iters; c.llr = d_llr;
    if (kernel == 3) return stream_launch(h, c, s);
    if (kernel == 2) return generic_launch(h, c, s);
    return fused_launch(h, c, s);
}
QBP_ABI_CATCH

// The outputs of a large qbp_decode_batch call, b records in the handle's scratch: device -> pinned staging (DMA at
// PCIe rate) -> the caller's arrays (memcpy), in chunks of up to 32 MiB, the host copy of one chunk overlapping the
// DMA of the next.  (A direct copy into pageable memory goes through the runtime's own small staging buffers at a
// fraction of that rate.)  The two staging buffers are as large as the largest chunk any call of this handle has
// needed, never more than 32 MiB each (they used to be 32 MiB from the first 256 KiB call on).  The one
// download that is not "enqueue all, synchronise once": it does not go through HostStage, whose finish ends the call.
static int decode_copy_out(qbp_handle* h, size_t b, uint8_t* hard, uint8_t* converged, int32_t* iters, double* llr,
                           hipStream_t s)
{
    const size_t n = h->n;
    const size_t per = (hard ? n : 0) + (converged ? 1 : 0) + (iters ? 4 : 0) + (llr ? 8 * n : 0);
    constexpr size_t STAGE = (size_t)32 << 20;
    if (per == 0) return QBP_OK;
    // (pieces of at least 1 MiB, at least four of them above 4 MiB: the reference driver's 13 MB per
    // batch then overlap their DMA with the copy-out instead of running one after the other)
    const size_t quarter = std::max<size_t>((b + 3) / 4, ((size_t)1 << 20) / per + 1);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>({b, STAGE / (per + 8), quarter}));
    const size_t need = std::min<size_t>(STAGE, chunk * (per + 8) + 64);
    if (h->stage_bytes < need) {
        for (int i = 0; i < 2; ++i) {
            if (h->stage[i]) (void)hipHostFree(h->stage[i]);
            h->stage[i] = nullptr;
        }
        h->stage_bytes = 0;
        const size_t want = std::min<size_t>(STAGE, std::max<size_t>(need, (size_t)1 << 20));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(hipHostMalloc(&h->stage[i], want + 64, hipHostMallocDefault));
            if (!h->stage_ev[i]) HIP_TRY(hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming));
        }
        h->stage_bytes = want;
    }
    struct Piece { size_t b0, cnt; };
    Piece prev{0, 0};
    auto offsets = [&](size_t cnt, size_t& o_llr, size_t& o_it, size_t& o_hard, size_t& o_conv) {
        o_llr = 0;
        o_it = o_llr + (llr ? cnt * n * 8 : 0);
        o_hard = o_it + (iters ? ((cnt * 4 + 7) & ~(size_t)7) : 0);
        o_conv = o_hard + (hard ? cnt * n : 0);
    };
    auto drain = [&](const Piece& pc, int slot) -> int {
        if (pc.cnt == 0) return QBP_OK;
        HIP_TRY(hipEventSynchronize(h->stage_ev[slot]));
        const uint8_t* st = static_cast<const uint8_t*>(h->stage[slot]);
        size_t o_llr, o_it, o_hard, o_conv;
        offsets(pc.cnt, o_llr, o_it, o_hard, o_conv);
        if (llr) std::memcpy(llr + pc.b0 * n, st + o_llr, pc.cnt * n * 8);
        if (iters) std::memcpy(iters + pc.b0, st + o_it, pc.cnt * 4);
        if (hard) std::memcpy(hard + pc.b0 * n, st + o_hard, pc.cnt * n);
        if (converged) std::memcpy(converged + pc.b0, st + o_conv, pc.cnt);
        return QBP_OK;
    };
    int slot = 0;
    for (size_t b0 = 0; b0 < b; b0 += chunk, slot ^= 1) {
        const size_t cnt = std::min(chunk, b - b0);
        uint8_t* st = static_cast<uint8_t*>(h->stage[slot]);
        size_t o_llr, o_it, o_hard, o_conv;
        offsets(cnt, o_llr, o_it, o_hard, o_conv);
        if (llr) HIP_TRY(hipMemcpyAsync(st + o_llr, h->d_llr.p + b0 * n, cnt * n * 8, hipMemcpyDeviceToHost, s));
        if (iters) HIP_TRY(hipMemcpyAsync(st + o_it, h->d_iters.p + b0, cnt * 4, hipMemcpyDeviceToHost, s));
        if (hard) HIP_TRY(hipMemcpyAsync(st + o_hard, h->d_hard.p + b0 * n, cnt * n, hipMemcpyDeviceToHost, s));
        if (converged) HIP_TRY(hipMemcpyAsync(st + o_conv, h->d_conv.p + b0, cnt, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(h->stage_ev[slot], s));
        const int rc2 = drain(prev, slot ^ 1);          // the previous chunk, while this one is in flight
        if (rc2) return rc2;
        prev = Piece{b0, cnt};
    }
    return drain(prev, slot ^ 1);
}

int qbp_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B,
                     int32_t max_iter, int32_t variant, double alpha, double damping,
                     double clip_llr, uint32_t flags, uint8_t* hard, uint8_t* converged,
                     int32_t* iters, double* llr)
try {
    int rc = check_decode_args(h, B, max_iter, variant);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!syndromes || !prior) return fail(QBP_E_INVALID, "null input pointer");
    if ((rc = check_prior(h->n, prior, false)) != QBP_OK) return rc;
    if (flags & QBP_FLAG_LAYERED) {
        if ((rc = check_layered_flags(h, flags, variant, false)) != QBP_OK) return rc;
        if ((rc = check_prior(h->n, prior, true)) != QBP_OK) return rc;
    }
    if ((rc = check_quant_flags(h, flags, variant, true)) != QBP_OK) return rc;
    if (flags & QBP_FLAG_DENSE_F_COLSUM_ITER0) {     // (the shortcut is judged on the host copy of the priors)
        int mode = 0;
        unsigned fl = flags;
        rc = resolve_column_order(h, fl, prior, &mode);
        if (rc) return rc;
        if (mode == 0) flags = fl;                   // iteration 0 cannot depend on the order: plain call
    }
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t m = h->m, n = h->n, b = (size_t)B;
    {
        // Small calls (the reference's one-syndrome-per-call usage, paperResults.py:71): inputs and
        // outputs live in ONE pinned host buffer that the kernel reads and writes directly over
        // PCIe; per call: two host memcpys, a memset node, the launch and one stream sync
        // instead of six hipMemcpyAsync round trips.
        const size_t off_prior = (b * m + 7) & ~(size_t)7;
        const size_t off_llr = off_prior + n * 8;
        const size_t off_iters = off_llr + b * n * 8;
        const size_t off_hard = off_iters + ((b * 4 + 7) & ~(size_t)7);
        const size_t off_conv = off_hard + b * n;
        const size_t total = off_conv + b;
        if (total <= (size_t)256 * 1024) {
            if (h->pin_bytes < total) {
                if (h->pin_host) (void)hipHostFree(h->pin_host);
                h->pin_host = nullptr; h->pin_bytes = 0;
                const size_t want = std::max<size_t>(total, 64 * 1024);
                HIP_TRY(hipHostMalloc(&h->pin_host, want, hipHostMallocMapped));
                HIP_TRY(hipHostGetDevicePointer(&h->pin_dev, h->pin_host, 0));
                h->pin_bytes = want;
            }
            uint8_t* ph = static_cast<uint8_t*>(h->pin_host);
            uint8_t* pd = static_cast<uint8_t*>(h->pin_dev);
            std::memcpy(ph, syndromes, b * m);
            std::memcpy(ph + off_prior, prior, n * 8);
            hipStream_t s = h->stream;
            rc = qbp_decode_batch_device(
                h, pd, reinterpret_cast<const double*>(pd + off_prior), B, max_iter, variant, alpha, damping,
                clip_llr, flags, hard ? pd + off_hard : nullptr, converged ? pd + off_conv : nullptr,
                iters ? reinterpret_cast<int32_t*>(pd + off_iters) : nullptr,
                llr ? reinterpret_cast<double*>(pd + off_llr) : nullptr, s);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(s));
            if (hard) std::memcpy(hard, ph + off_hard, b * n);
            if (converged) std::memcpy(converged, ph + off_conv, b);
            if (iters) std::memcpy(iters, ph + off_iters, b * 4);
            if (llr) std::memcpy(llr, ph + off_llr, b * n * 8);
            return QBP_OK;
        }
    }
    // (the outputs leave through decode_copy_out, not through the stage's downloads: reserved only)
    if (hard) HIP_TRY(h->d_hard.reserve(b * n));
    if (converged) HIP_TRY(h->d_conv.reserve(b));
    if (iters) HIP_TRY(h->d_iters.reserve(b));
    if (llr) HIP_TRY(h->d_llr.reserve(b * n));
    hipStream_t s = h->stream;
    HostStage st(s);
    const uint8_t* d_syn = st.in(h->d_syn, syndromes, b * m);
    const double* d_prior = st.in(h->d_prior, prior, n);
    if (st.failed()) return st.error();
    rc = qbp_decode_batch_device(h, d_syn, d_prior, B, max_iter, variant, alpha, damping, clip_llr, flags,
                                 hard ? h->d_hard.p : nullptr, converged ? h->d_conv.p : nullptr,
                                 iters ? h->d_iters.p : nullptr, llr ? h->d_llr.p : nullptr, s);
    if (rc == QBP_OK) rc = decode_copy_out(h, b, hard, converged, iters, llr, s);
    return st.finish(rc);
}
QBP_ABI_CATCH

// The messages of iteration `iteration` of a B-syndrome decode (host inputs), [B][E] in h->d_llr: the work of
// qbp_check_messages and qbp_message_histograms after their argument checks.
static int dump_messages(qbp_handle* h, HostStage& st, const uint8_t* syndromes, const double* prior, int64_t B,
                         int variant, double alpha, double damping, double clip_llr, int iteration, uint32_t flags,
                         int col_mode, hipStream_t s)
{
    if (variant == QBP_SUM_PRODUCT) {
        // plain sum-product = the damped update with alpha = damping = 1 and no LLR clip: the
        // caller's alpha / damping / clip_llr are ignored, as QBP_SUM_PRODUCT ignores them everywhere
        variant = QBP_DAMPED_SP;
        alpha = 1.0; damping = 1.0; clip_llr = __builtin_inf();
    }
    const size_t m = h->m, n = h->n, b = (size_t)B, E = (size_t)std::max(h->E, 1);
    HIP_TRY(h->d_llr.reserve(b * E));
    BpCall c;
    c.syndromes = st.in(h->d_syn, syndromes, b * m);
    c.prior = st.in(h->d_prior, prior, n);
    if (st.failed()) return st.error();
    c.B = B; c.max_iter = iteration + 1; c.variant = variant;
    c.alpha = alpha; c.damping = damping; c.clip_llr = clip_llr;
    c.flags = flags | QBP_FLAG_FORCE_FULL;   // (no early exit before the dump iteration)
    c.dump = h->d_llr.p; c.dump_iter = iteration;
    // min-sum returns R_new / alpha (rework/decoding.py:58-59); damped SP the unscaled R (:168-169,
    // taken before R * alpha)
    c.dump_div = variant == QBP_MIN_SUM ? alpha : 1.0;
    c.col_mode = col_mode;
    return generic_launch(h, c, s);
}

int qbp_check_messages(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B,
                       int32_t variant, double alpha, double damping, double clip_llr,
                       int32_t iteration, uint32_t flags, double* messages)
try {
    int rc = check_decode_args(h, B, iteration + 1, variant);
    if (rc) return rc;
    if ((rc = check_layered_flags(h, flags, variant, true)) != QBP_OK) return rc;
    if ((rc = check_quant_flags(h, flags, variant, true)) != QBP_OK) return rc;
    int col_mode = 0;                    // (only the column-sum order bits of `flags` are honoured)
    flags &= QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0 | QBP_FLAG_PAIRWISE_COLSUM;
    if (prior) { rc = resolve_column_order(h, flags, prior, &col_mode); if (rc) return rc; }
    if (B == 0) return QBP_OK;
    if (!syndromes || !prior || !messages) return fail(QBP_E_INVALID, "null pointer");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    hipStream_t s = h->stream;
    HostStage st(s);
    rc = dump_messages(h, st, syndromes, prior, B, variant, alpha, damping, clip_llr, iteration, flags, col_mode, s);
    if (rc == QBP_OK) st.out(h->d_llr, messages, (size_t)B * (size_t)h->E);     // (reserved by dump_messages: the download alone)
    return st.finish(rc);
}
QBP_ABI_CATCH

int qbp_message_histograms(qbp_handle* h, const uint8_t* syndromes, const uint8_t* errors, const double* prior,
                           int64_t B, int32_t variant, double alpha, double damping, double clip_llr,
                           int32_t iteration, uint32_t flags, int32_t bins, double* edges, int64_t* hist0,
                           int64_t* hist1)
try {
    int rc = check_decode_args(h, B, iteration + 1, variant);
    if (rc) return rc;
    if (!syndromes || !errors || !prior || !edges || !hist0 || !hist1) return fail(QBP_E_INVALID, "null pointer");
    int col_mode = 0;                    // (only the column-sum order bits of `flags` are honoured)
    flags &= QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0 | QBP_FLAG_PAIRWISE_COLSUM;
    rc = resolve_column_order(h, flags, prior, &col_mode);
    if (rc) return rc;
    if (bins < 1 || bins > 4096) return fail(QBP_E_INVALID, "bins = %d out of range (1 .. 4096)", bins);
    if (B == 0 || h->E == 0) return fail(QBP_E_INVALID, "no messages to bin (B = %lld, E = %d)", (long long)B, h->E);
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t n = h->n, b = (size_t)B, E = (size_t)h->E;
    hipStream_t s = h->stream;
    HostStage st(s);                                 // (every return below leaves the stream idle)
    const uint8_t* d_errors = st.in(h->d_hard, errors, b * n);      // the true error bits
    if (st.failed()) return st.error();
    rc = dump_messages(h, st, syndromes, prior, B, variant, alpha, damping, clip_llr, iteration, flags, col_mode, s);
    if (rc) return rc;
    // range of all messages (rework/Alvarado.py:41-44: the two classes share one range)
    const int grid = (int)std::min<size_t>(1024, (b * E + 255) / 256);
    HIP_TRY(h->d_part.reserve((size_t)2 * grid));
    HIP_TRY(qbp::launch_hist_minmax(grid, h->d_llr.p, (long long)(b * E), h->d_part.p, s));
    std::vector<double> part((size_t)2 * grid);
    HIP_TRY(hipMemcpyAsync(part.data(), h->d_part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int i = 0; i < grid; ++i) {                 // (a NaN part stays: std::min / std::max would drop it)
        lo = (std::isnan(part[2 * i]) || part[2 * i] < lo) ? part[2 * i] : lo;
        hi = (std::isnan(part[2 * i + 1]) || part[2 * i + 1] > hi) ? part[2 * i + 1] : hi;
    }
    if (!(lo <= hi) || std::isinf(lo) || std::isinf(hi))
        return fail(QBP_E_INVALID, "message range [%g, %g] is not finite (np.histogram raises there too)", lo, hi);
    if (lo == hi) { lo -= 0.5; hi += 0.5; }          // np.histogram's rule for a degenerate range
    // np.linspace(lo, hi, bins + 1): start + i * step, the last edge exactly hi
    const double step = (hi - lo) / (double)bins;
    for (int i = 0; i < bins; ++i) edges[i] = (double)i * step + lo;
    edges[bins] = hi;
    std::vector<unsigned long long> hist((size_t)2 * bins);
    const double* d_edges = st.in(h->d_edges, edges, (size_t)bins + 1);
    unsigned long long* d_hist = st.out(h->d_hist, hist.data(), hist.size());
    if (st.failed()) return st.error();
    HIP_TRY(hipMemsetAsync(d_hist, 0, hist.size() * sizeof(unsigned long long), s));
    const size_t lds = (((size_t)2 * bins + 1) & ~(size_t)1) * 4 + ((size_t)bins + 1) * 8;
    HIP_TRY(qbp::launch_hist_bin(grid, lds, h->d_llr.p, d_errors, h->d_col_idx.p, (long long)B, (int)E, (int)n,
                                 d_edges, bins, d_hist, s));
    if ((rc = st.finish(QBP_OK)) != QBP_OK) return rc;
    for (int i = 0; i < bins; ++i) { hist0[i] = (int64_t)hist[i]; hist1[i] = (int64_t)hist[bins + i]; }
    return QBP_OK;
}
QBP_ABI_CATCH

static int mc_prepare(qbp_handle* h, const uint8_t* Lx, int32_t k, hipStream_t s)
{
    if (k < 0 || k > 64) return fail(QBP_E_INVALID, "k = %d logical operators (need 0..64)", k);
    if (k > 0 && !Lx) return fail(QBP_E_INVALID, "Lx is null");
    return h->mc_in.prepare_lx((size_t)h->n, Lx, k, s);
}

// probs [n] of qbp_mc_run_probs: every value in [0, 1] (host only, before any GPU work)
static int check_probs(const qbp_handle* h, const double* probs)
{
    if (!probs) return fail(QBP_E_INVALID, "probs is null");
    for (int v = 0; v < h->n; ++v)
        if (!(probs[v] >= 0.0 && probs[v] <= 1.0))
            return fail(QBP_E_INVALID, "probs[%d] = %g out of [0, 1]", v, probs[v]);
    return QBP_OK;
}

// The one-pivot-at-a-time kernel, which follows the reference's row swaps (qbp_osd.hpp, osd0_big_kernel): matrices
// beyond 8192 rows, QBP_OPT_OSD_BIG = 2, and the records a fast kernel found inconsistent.
static int osd_launch_swaps(qbp_handle* h, const qbp::OsdParams& O, long long max_grid, hipStream_t s)
{
    const size_t m = h->m, n = h->n, RS = (size_t)h->osd_W + 1, NP = (size_t)h->osd_NP;
    const int grid = (int)std::max<long long>(1, std::min<long long>(max_grid, (long long)h->num_cu * 2));
    qbp::OsdBigWorkspace Wk{};
    Wk.keys_in_lds = NP * 12 <= (size_t)96 * 1024 ? 1 : 0;
    HIP_TRY(h->d_osd_At.reserve((size_t)grid * RS * m));
    HIP_TRY(h->d_osd_piv.reserve((size_t)grid * m));
    HIP_TRY(h->d_osd_posn.reserve((size_t)grid * 2 * m));
    HIP_TRY(h->d_osd_sol.reserve((size_t)grid * n));
    if (!Wk.keys_in_lds) {
        HIP_TRY(h->d_osd_keys.reserve((size_t)grid * NP));
        HIP_TRY(h->d_osd_idx.reserve((size_t)grid * NP));
    }
    Wk.At = h->d_osd_At.p; Wk.pivcol = h->d_osd_piv.p; Wk.posn = h->d_osd_posn.p; Wk.sol = h->d_osd_sol.p;
    Wk.keys = h->d_osd_keys.p; Wk.idx = h->d_osd_idx.p;
    // (O.spectrum, here and in osd_launch: the builds that add residual weights to that table, qbp_mc_run_spectrum;
    // O.shots: the builds that predict recorded shots, qbp_decode_shots; O.order: the builds that take the column
    // order from the caller, qbp_osd_batch_ordered)
    HIP_TRY((O.order ? qbp::launch_osd_big_ordered : O.shots ? qbp::launch_osd_big_shots
             : O.spectrum ? qbp::launch_osd_big_spectrum : qbp::launch_osd_big)(
        (unsigned)grid, Wk.keys_in_lds ? NP * 12 : 0, O, Wk, s));
    return QBP_OK;
}

// Order-w OSD flags (include/qbp.h: QBP_FLAG_OSD_CS / _E, order in bits 16..23) -> method (0: OSD-0) and order.
// `mc`: flags of qbp_mc_run*, where a method needs QBP_FLAG_OSD0 and the other bits are the decoder's; elsewhere
// (qbp_osd_batch) nothing but the OSD bits may be set.
constexpr uint32_t OSD_ORDER_BITS = 0xffu << 16;
constexpr uint32_t OSD_METHOD_BITS = QBP_FLAG_OSD_CS | QBP_FLAG_OSD_E;
constexpr uint32_t OSD_ALL_BITS = OSD_ORDER_BITS | OSD_METHOD_BITS | QBP_FLAG_OSD_LARGE;   // what only the OSD launch sees

// Whether, and with which LDS layout, the eight-pivots-at-a-time kernels take the matrix (qbp_osd.hpp,
// osd0_blocked_kernel; qbp_osd_order_big.hpp): up to 8192 rows, unless QBP_OPT_OSD_BIG = 2.  osd_launch uses them
// where the one-wavefront kernels do not apply.
struct OsdBlockedPlan {
    bool ok;
    int keys_in_lds;
    size_t wc_max, want_table, region0, qs, act, lds;
};
static OsdBlockedPlan osd_blocked_plan(const qbp_handle* h)
{
    OsdBlockedPlan B{};
    const size_t m = h->m, n = h->n, NP = (size_t)h->osd_NP;
    B.wc_max = (n + 63) / 64 + 1;
    const size_t LDS_MAX = 160 * 1024 - 64;                          // (static __shared__ of the kernels: 64 bytes)
    B.qs = 8 * B.wc_max * 8;
    B.act = m * 4;                                                   // (row, D) list of a block's updates
    B.want_table = std::min<size_t>(96 * 1024, 256 * B.wc_max * 8);
    B.region0 = std::max(B.want_table, NP * 8);
    B.lds = B.region0 + B.qs + NP * 4 + ((n + 15) & ~(size_t)15) + B.act;
    B.keys_in_lds = 1;
    if (B.lds > LDS_MAX) { B.keys_in_lds = 0; B.region0 = B.want_table; B.lds = B.region0 + B.qs + B.act; }
    B.ok = h->opt_osd_big != 2 && m <= 8192 && B.lds <= LDS_MAX && 2 * B.wc_max * 8 <= B.want_table;
    return B;
}

// Order w on the one-wavefront kernel: OSD-0 runs there and osd_order_kernel's added LDS fits as well.
static bool osd_order_one_wave(const qbp_handle* h)
{
    return h->osd_ok && qbp::osd_order_lds_bytes(h->m, h->n, h->osd_W, h->osd_NP) <= 64 * 1024;
}

static int parse_osd_flags(const qbp_handle* h, uint32_t flags, bool mc, int* method, int* order)
{
    *method = 0;
    *order = (int)((flags & OSD_ORDER_BITS) >> 16);
    const uint32_t mb = flags & OSD_METHOD_BITS;
    if (!mc && (flags & ~(OSD_ALL_BITS | QBP_FLAG_OSD0)))
        return fail(QBP_E_INVALID, "osd_flags 0x%x: unknown bits", flags);
    if (mb == OSD_METHOD_BITS) return fail(QBP_E_INVALID, "QBP_FLAG_OSD_CS and QBP_FLAG_OSD_E together");
    if (!mb) {
        if (flags & QBP_FLAG_OSD_LARGE)
            return fail(QBP_E_INVALID, "QBP_FLAG_OSD_LARGE without QBP_FLAG_OSD_CS or QBP_FLAG_OSD_E");
        if (*order) return fail(QBP_E_INVALID, "an OSD order (%d) without QBP_FLAG_OSD_CS or QBP_FLAG_OSD_E", *order);
        return QBP_OK;
    }
    if (mc && !(flags & QBP_FLAG_OSD0)) return fail(QBP_E_INVALID, "an OSD method bit without QBP_FLAG_OSD0");
    *method = mb == QBP_FLAG_OSD_CS ? qbp::OSD_METHOD_CS : qbp::OSD_METHOD_E;
    const int hi = *method == qbp::OSD_METHOD_CS ? 64 : 12;
    if (*order < 1 || *order > hi)
        return fail(QBP_E_INVALID, "OSD-%s order %d out of [1, %d]", *method == qbp::OSD_METHOD_CS ? "CS" : "E",
                    *order, hi);
    // order > 0 runs on the one-wavefront kernel where its added LDS fits -- and, with QBP_FLAG_OSD_LARGE, wherever
    // the blocked kernel's conditions hold (osd_launch sends it there)
    if (osd_order_one_wave(h)) return QBP_OK;
    if (flags & QBP_FLAG_OSD_LARGE) {
        if (osd_blocked_plan(h).ok) return QBP_OK;
        return fail(QBP_E_UNSUPPORTED, "OSD of order > 0 with QBP_FLAG_OSD_LARGE needs a matrix the blocked OSD kernel "
                                       "takes (%d x %d: beyond 8192 rows or its LDS, or QBP_OPT_OSD_BIG = 2)", h->m, h->n);
    }
    return fail(QBP_E_UNSUPPORTED, "OSD of order > 0 needs a matrix whose rows fit the LDS of one wavefront "
                                   "(%d x %d does not), or QBP_FLAG_OSD_LARGE", h->m, h->n);
}

// O.order (qbp_osd_batch_ordered; null everywhere else): the column orders of the records, for the same choice of
// kernel and for the redo pass, whose list holds record indices.
// `redo`: the caller's syndromes may lie outside the column space of H (anything but the Monte-Carlo loop, whose
// syndromes come from errors): the fast kernels then list the records whose sweep says so, and the kernel that
// follows the reference's row swaps recomputes them (an empty list costs one small launch).
static int osd_launch(qbp_handle* h, qbp::OsdParams& O, long long max_items, hipStream_t s, bool redo = false,
                      int method = 0, int order = 0)
{
    O.m = h->m; O.n = h->n; O.W = h->osd_W; O.NP = h->osd_NP;
    O.row_ptr = h->d_row_ptr.p; O.col_idx = h->d_col_idx.p;
    const int rc = osd_prepare(h);
    if (rc) return rc;
    O.rank = h->osd_rank; O.hbits = h->d_hbits.p;
    const size_t m = h->m, n = h->n, NP = (size_t)h->osd_NP;
    // -- matrices beyond the LDS limit: eight pivots at a time (qbp_osd.hpp, osd0_blocked_kernel)
    qbp::OsdBigWorkspace Wk{};
    const OsdBlockedPlan B = osd_blocked_plan(h);
    const size_t wc_max = B.wc_max, want_table = B.want_table, region0 = B.region0, lds = B.lds, act = B.act;
    Wk.keys_in_lds = B.keys_in_lds;
    // (order w on a matrix OSD-0's one-wavefront kernel takes but osd_order_kernel's LDS does not fit: parse_osd_flags
    // let it pass for QBP_FLAG_OSD_LARGE alone, and the blocked order kernel serves it)
    const bool blocked = B.ok && (!h->osd_ok || (method && !osd_order_one_wave(h)));
    if (!h->osd_ok && !blocked) return osd_launch_swaps(h, O, max_items, s);
    if (redo) {
        HIP_TRY(h->d_osd_redo.reserve((size_t)max_items + 1));
        HIP_TRY(hipMemsetAsync(h->d_osd_redo.p, 0, 8, s));
        O.redo = h->d_osd_redo.p;
    }
    if (blocked) {
        const int grid = (int)std::max<long long>(1, std::min<long long>(max_items, (long long)h->num_cu));
        Wk.wc_max = (int)wc_max;
        // first sweep: the 2048 least reliable columns (a sweep ends where no unpivoted row has a syndrome
        // bit left -- after some 200 columns on the BP failures of the space-time matrices in the tests,
        // 1632 at most)
        Wk.k_first = h->opt_osd_big == 3 ? 24 : (int)std::min<size_t>(n, 2048);
        Wk.lds_act = (int)(lds - act);
        HIP_TRY(h->d_osd_next.reserve(1));
        HIP_TRY(hipMemsetAsync(h->d_osd_next.p, 0, 8, s));
        Wk.next = h->d_osd_next.p;
        Wk.lds_region0 = (int)region0; Wk.lds_table = (int)want_table;
        HIP_TRY(h->d_osd_At.reserve((size_t)grid * wc_max * m * 2));
        if (!Wk.keys_in_lds) {
            HIP_TRY(h->d_osd_sol.reserve((size_t)grid * n));
            HIP_TRY(h->d_osd_keys.reserve((size_t)grid * NP));
            HIP_TRY(h->d_osd_idx.reserve((size_t)grid * NP));
        }
        Wk.At = h->d_osd_At.p; Wk.sol = h->d_osd_sol.p; Wk.keys = h->d_osd_keys.p; Wk.idx = h->d_osd_idx.p;
        const int rpt = m <= 1024 ? 1 : m <= 2048 ? 2 : m <= 4096 ? 4 : 8;
        if (method) {
            // order w (parse_osd_flags has seen QBP_FLAG_OSD_LARGE): qbp_osd_order_big.hpp.  Its per-column table
            // (12 n bytes) overlays the LDS the sweep is done with, or goes to the workspace
            qbp::OsdOrderBigArgs X{};
            X.method = method; X.order = order;
            // (with the keys in LDS, region 0 and Qs hold 12 n bytes: n <= 8192 there and want_table >= min(96 KiB, 32 n))
            X.spill = !Wk.keys_in_lds;
            if (X.spill) { HIP_TRY(h->d_osd_keys.reserve((size_t)grid * NP)); }
            HIP_TRY(h->d_osd_tk.reserve((size_t)grid * 2 * n));
            Wk.keys = h->d_osd_keys.p; X.tk = h->d_osd_tk.p;
            HIP_TRY((O.order ? qbp::launch_osd_order_blocked_ordered : O.shots ? qbp::launch_osd_order_blocked_shots
                     : O.spectrum ? qbp::launch_osd_order_blocked_spectrum : qbp::launch_osd_order_blocked)(
                rpt, (unsigned)grid, lds, O, Wk, X, s));
        } else {
            HIP_TRY((O.order ? qbp::launch_osd_blocked_ordered : O.shots ? qbp::launch_osd_blocked_shots
                     : O.spectrum ? qbp::launch_osd_blocked_spectrum : qbp::launch_osd_blocked)(rpt, (unsigned)grid, lds, O,
                                                                                                Wk, s));
        }
    } else if (method) {
        // order w (parse_osd_flags has checked osd_ok and the LDS)
        const long long grid = std::max<long long>(1, std::min<long long>(max_items, (long long)h->num_cu * 32));
        const size_t olds = (qbp::osd_order_lds_bytes(h->m, h->n, h->osd_W, h->osd_NP) + 15) & ~(size_t)15;
        HIP_TRY((O.order ? qbp::launch_osd_order_ordered : O.shots ? qbp::launch_osd_order_shots
                 : O.spectrum ? qbp::launch_osd_order_spectrum : qbp::launch_osd_order)(h->osd_W + 1, (unsigned)grid, olds, O,
                                                                                        method, order, s));
    } else {
        const long long grid = std::max<long long>(1, std::min<long long>(max_items, (long long)h->num_cu * 32));
        HIP_TRY((O.order ? qbp::launch_osd_small_ordered : O.shots ? qbp::launch_osd_small_shots
                 : O.spectrum ? qbp::launch_osd_small_spectrum : qbp::launch_osd_small)(h->osd_W + 1, (unsigned)grid,
                                                                                        (size_t)h->osd_lds, O, s));
    }
    if (redo) {
        qbp::OsdParams R = O;
        R.redo = nullptr; R.count = 0;
        R.count_ptr = h->d_osd_redo.p; R.list = h->d_osd_redo.p + 1;
        return osd_launch_swaps(h, R, std::min<long long>(max_items, 32), s);
    }
    return QBP_OK;
}

// qbp_osd_batch_device and qbp_osd_batch_ordered_device: `d_order` null is the former
static int osd_batch_device(qbp_handle* h, uint32_t osd_flags, const uint8_t* d_syndromes, const double* d_llr,
                            const uint8_t* d_hard, const int32_t* d_order, int64_t B, uint8_t* d_solution, void* stream)
{
    if (!h) return fail(QBP_E_INVALID, "null handle");
    int method = 0, order = 0;
    int rc = parse_osd_flags(h, osd_flags, false, &method, &order);
    if (rc) return rc;
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0");
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_llr || !d_hard || !d_solution) return fail(QBP_E_INVALID, "null pointer");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    qbp::OsdParams O{};
    O.count = B; O.syndromes = d_syndromes; O.llr = d_llr; O.hard = d_hard; O.solution = d_solution;
    O.order = d_order;
    return osd_launch(h, O, B, static_cast<hipStream_t>(stream), true, method, order);
}

int qbp_osd_batch_device(qbp_handle* h, uint32_t osd_flags, const uint8_t* d_syndromes, const double* d_llr,
                         const uint8_t* d_hard, int64_t B, uint8_t* d_solution, void* stream)
try {
    return osd_batch_device(h, osd_flags, d_syndromes, d_llr, d_hard, nullptr, B, d_solution, stream);
}
QBP_ABI_CATCH

int qbp_osd_batch_ordered_device(qbp_handle* h, uint32_t osd_flags, const uint8_t* d_syndromes, const double* d_llr,
                                 const uint8_t* d_hard, const int32_t* d_order, int64_t B, uint8_t* d_solution,
                                 void* stream)
try {
    if (!d_order) return fail(QBP_E_INVALID, "null column order");
    return osd_batch_device(h, osd_flags, d_syndromes, d_llr, d_hard, d_order, B, d_solution, stream);
}
QBP_ABI_CATCH

// qbp_osd_batch and qbp_osd_batch_ordered (`ordered`): host buffers in, solutions out
static int osd_batch_host(qbp_handle* h, uint32_t osd_flags, const uint8_t* syndromes, const double* llr,
                          const uint8_t* hard, const int32_t* col_order, bool ordered, int64_t B, uint8_t* solution)
{
    if (!h) return fail(QBP_E_INVALID, "null handle");
    int method = 0, order = 0;
    int rc = parse_osd_flags(h, osd_flags, false, &method, &order);
    if (rc) return rc;
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0");
    if (B == 0) return QBP_OK;
    if (!syndromes || !llr || !hard || !solution) return fail(QBP_E_INVALID, "null pointer");
    const size_t m = h->m, n = h->n, b = (size_t)B;
    if (ordered) {
        // every row a permutation of 0..n-1: checked here, before any GPU work (the kernels only stay in bounds)
        if (!col_order) return fail(QBP_E_INVALID, "null column order");
        std::vector<uint8_t> seen(n);
        for (size_t r = 0; r < b; ++r) {
            std::fill(seen.begin(), seen.end(), (uint8_t)0);
            for (size_t i = 0; i < n; ++i) {
                const int32_t c = col_order[r * n + i];
                if (c < 0 || (size_t)c >= n)
                    return fail(QBP_E_INVALID, "column order of record %lld: entry %d at position %lld is outside [0, %d)",
                                (long long)r, (int)c, (long long)i, h->n);
                if (seen[c])
                    return fail(QBP_E_INVALID, "column order of record %lld: column %d appears twice (not a permutation)",
                                (long long)r, (int)c);
                seen[c] = 1;
            }
        }
    }
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    HostStage st(h->stream);
    const uint8_t* d_syn = st.in(h->d_syn, syndromes, b * m);
    const double* d_llr = st.in(h->d_llr, llr, b * n);
    const uint8_t* d_hard = st.in(h->d_hard, hard, b * n);
    const int32_t* d_order = ordered ? st.in(h->d_osd_order, col_order, b * n) : nullptr;
    uint8_t* d_sol = st.out(h->d_sol, solution, b * n);
    if (st.failed()) return st.error();
    return st.finish(osd_batch_device(h, osd_flags, d_syn, d_llr, d_hard, d_order, B, d_sol, h->stream));
}

int qbp_osd_batch(qbp_handle* h, uint32_t osd_flags, const uint8_t* syndromes, const double* llr, const uint8_t* hard,
                  int64_t B, uint8_t* solution)
try {
    return osd_batch_host(h, osd_flags, syndromes, llr, hard, nullptr, false, B, solution);
}
QBP_ABI_CATCH

int qbp_osd_batch_ordered(qbp_handle* h, uint32_t osd_flags, const uint8_t* syndromes, const double* llr,
                          const uint8_t* hard, const int32_t* order, int64_t B, uint8_t* solution)
try {
    return osd_batch_host(h, osd_flags, syndromes, llr, hard, order, true, B, solution);
}
QBP_ABI_CATCH

int qbp_osd0_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_llr,
                          const uint8_t* d_hard, int64_t B, uint8_t* d_solution, void* stream)
try {
    return qbp_osd_batch_device(h, 0, d_syndromes, d_llr, d_hard, B, d_solution, stream);
}
QBP_ABI_CATCH

int qbp_osd0_batch(qbp_handle* h, const uint8_t* syndromes, const double* llr, const uint8_t* hard,
                   int64_t B, uint8_t* solution)
try {
    return qbp_osd_batch(h, 0, syndromes, llr, hard, B, solution);
}
QBP_ABI_CATCH

// budgets [n_budgets] of qbp_mc_run_budgets: 1 <= n_budgets <= QBP_MC_MAX_BUDGETS values >= 1, strictly ascending
// (host only, before any GPU work)
static int check_budgets(const int32_t* budgets, int32_t n_budgets)
{
    if (!budgets) return fail(QBP_E_INVALID, "budgets is null");
    if (n_budgets < 1 || n_budgets > QBP_MC_MAX_BUDGETS)
        return fail(QBP_E_INVALID, "n_budgets = %d out of [1, %d]", n_budgets, QBP_MC_MAX_BUDGETS);
    for (int j = 0; j < n_budgets; ++j) {
        if (budgets[j] < 1) return fail(QBP_E_INVALID, "budgets[%d] = %d must be >= 1", j, budgets[j]);
        if (j > 0 && budgets[j] <= budgets[j - 1])
            return fail(QBP_E_INVALID, "budgets must be strictly ascending (budgets[%d] = %d after %d)", j, budgets[j],
                        budgets[j - 1]);
    }
    return QBP_OK;
}

// With QBP_FLAG_OSD0 a call keeps a record per trial and counter row (m + 10 n bytes each): at most
// QBP_MC_OSD_MAX_TRIALS records and 16 GiB (host only, before any GPU work)
static int check_mc_osd_trials(const qbp_handle* h, int64_t T, size_t rows)
{
    const size_t t = (size_t)T * rows, m = h->m, n = h->n;
    if (t > QBP_MC_OSD_MAX_TRIALS || t * (m + 10 * n) > ((size_t)16 << 30))
        return fail(QBP_E_INVALID, "with QBP_FLAG_OSD0 a call covers at most %lld trials of this matrix "
                                   "(got %lld); split the range",
                    (long long)(std::min<size_t>(QBP_MC_OSD_MAX_TRIALS, ((size_t)16 << 30) / (m + 10 * n)) / rows),
                    (long long)T);
    return QBP_OK;
}

// ---- layered BP (qbp_layered.hpp) --------------------------------------------------------------------------------
// The order and the levels of the layered schedule (include/qbp.h, qbp_layered_plan): host only.
//   order_in null: greedy colouring -- checks in ascending index, each the smallest colour no earlier neighbour holds --
//   ordered by (colour, index); else a permutation of the checks.
//   level of a check: 1 + the largest level of the checks that share a variable with it and come earlier in the order.
//   order_out: the order sorted by level (stable); level_ptr [n_levels + 1] into it.
static int layered_plan(const int32_t* row_ptr, const int32_t* col_idx, int m, int n, const int32_t* order_in,
                        std::vector<int32_t>& order_out, std::vector<int32_t>& level_ptr)
{
    std::vector<int32_t> order((size_t)m);
    if (order_in) {
        std::vector<uint8_t> seen((size_t)m, 0);
        for (int i = 0; i < m; ++i) {
            const int c = order_in[i];
            if (c < 0 || c >= m) return fail(QBP_E_INVALID, "order[%d] = %d is not a check (m = %d)", i, c, m);
            if (seen[c]) return fail(QBP_E_INVALID, "order holds check %d twice: not a permutation", c);
            seen[c] = 1;
            order[i] = c;
        }
    } else {
        // colours held by the earlier checks of each variable, as a list per variable (column weights are small)
        std::vector<std::vector<int>> var_colours((size_t)n);
        std::vector<int> colour((size_t)m, 0);
        std::vector<uint8_t> used;
        int n_colours = 0;
        for (int c = 0; c < m; ++c) {
            used.assign((size_t)n_colours + 1, 0);
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e)
                for (int k : var_colours[col_idx[e]]) used[k] = 1;
            int k = 0;
            while (used[k]) ++k;
            colour[c] = k;
            n_colours = std::max(n_colours, k + 1);
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) var_colours[col_idx[e]].push_back(k);
        }
        for (int c = 0; c < m; ++c) order[c] = c;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return colour[a] < colour[b]; });
    }
    std::vector<int> var_level((size_t)n, 0), level((size_t)m, 1);
    int n_levels = m > 0 ? 1 : 0;
    for (int i = 0; i < m; ++i) {
        const int c = order[i];
        int lv = 0;
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) lv = std::max(lv, var_level[col_idx[e]]);
        level[c] = lv + 1;
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) var_level[col_idx[e]] = lv + 1;
        n_levels = std::max(n_levels, lv + 1);
    }
    order_out = order;
    std::stable_sort(order_out.begin(), order_out.end(), [&](int a, int b) { return level[a] < level[b]; });
    level_ptr.assign((size_t)n_levels + 1, 0);
    for (int c = 0; c < m; ++c) level_ptr[level[c]] += 1;
    for (int l = 0; l < n_levels; ++l) level_ptr[l + 1] += level_ptr[l];
    return QBP_OK;
}

static int check_csr(const int32_t* row_ptr, const int32_t* col_idx, int m, int n)
{
    if (!row_ptr || !col_idx) return fail(QBP_E_INVALID, "null pointer");
    if (m < 1 || n < 1) return fail(QBP_E_INVALID, "m = %d, n = %d (need >= 1)", m, n);
    if (row_ptr[0] != 0) return fail(QBP_E_INVALID, "row_ptr[0] must be 0");
    for (int c = 0; c < m; ++c) {
        if (row_ptr[c + 1] < row_ptr[c]) return fail(QBP_E_INVALID, "row_ptr decreases at row %d", c);
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n) return fail(QBP_E_INVALID, "column %d out of range in row %d", col_idx[e], c);
            if (e > row_ptr[c] && col_idx[e] <= col_idx[e - 1])
                return fail(QBP_E_INVALID, "columns of row %d are not strictly ascending", c);
        }
    }
    return QBP_OK;
}

// The workspace step of a large launch: `count` doubles in ws, grown when a launch needs more, never shrunk.
static int large_workspace(DevBuf<double>& ws, size_t count, double** out)
{
    HIP_TRY(ws.reserve(count));
    *out = ws.p;
    return QBP_OK;
}

// Dynamic LDS of a workgroup with S slots in the build `large`
static size_t layered_build_lds(const qbp_handle* h, bool large, int S, bool tables)
{
    return large ? qbp::layered_large_lds_bytes(h->m, h->n, S, tables)
                 : qbp::layered_lds_bytes(h->m, h->n, h->E, S, tables);
}

// Slots per workgroup: about one work item per thread in the widest level, at most LAYERED_MAX_SLOTS and what keeps
// two workgroups' LDS on a CU; one slot always (qbp_layered_configure refuses what does not fit with one).
static int layered_slots(const qbp_handle* h, long long B, bool tables, bool large)
{
    int S = h->opt_layered_slots;
    if (S <= 0) {
        S = std::max(1, std::min(qbp::LAYERED_MAX_SLOTS, qbp::LAYERED_THREADS / std::max(1, h->layered_max_width)));
        while (S > 1 && layered_build_lds(h, large, S, tables) > (size_t)80 * 1024) --S;
    }
    while (S > 1 && layered_build_lds(h, large, S, tables) > (size_t)160 * 1024) --S;
    return (int)std::max<long long>(1, std::min<long long>(S, B));
}

// QBP_OPT_LAYERED_MEM (qbp_msg_mem.hpp), decided on the single-slot state by the sum-product size.  Matrices beyond
// the LDS of the build the option allows are QBP_E_UNSUPPORTED (host only); *large: the build of a launch.
static int layered_build(const qbp_handle* h, bool* large = nullptr)
{
    const qbp::MsgMemChoice c = qbp::msg_mem_choose(
        h->opt_msg_mem[qbp::MSG_MEM_LAYERED], layered_build_lds(h, false, 1, true), layered_build_lds(h, true, 1, true),
        [h](bool large_build, size_t need) {
            if (!large_build) {
                fail(QBP_E_UNSUPPORTED, "layered BP keeps the messages, the posterior and the prior of a record in LDS: "
                                        "%d x %d with %d entries needs %zu B (limit 160 KiB)", h->m, h->n, h->E, need);
                return;
            }
            const size_t fixed = qbp::layered_large_lds_bytes(h->m, 0, 1, true);
            fail(QBP_E_UNSUPPORTED, "layered BP with the messages in global memory keeps the posterior, n doubles, "
                                    "in LDS: %d x %d needs %zu B (limit 160 KiB: n <= %zu with %d checks)",
                 h->m, h->n, need, fixed < qbp::MSG_MEM_LDS_LIMIT ? (qbp::MSG_MEM_LDS_LIMIT - fixed) / 8 : (size_t)0, h->m);
        });
    if (large) *large = c.large;
    return c.ok ? QBP_OK : QBP_E_UNSUPPORTED;
}

// QBP_FLAG_LAYERED of a call (host only, before any GPU work).  `other_entry`: the entries without a layered build
// (budgets, spectra, recorded shots, message dumps).
static int check_layered_flags(const qbp_handle* h, uint32_t flags, int variant, bool other_entry)
{
    if (!(flags & QBP_FLAG_LAYERED)) return QBP_OK;
    if (other_entry)
        return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_LAYERED is not available with iteration budgets, spectra, recorded shots "
                                       "or message dumps");
    if (!h->layered_ready) return fail(QBP_E_INVALID, "QBP_FLAG_LAYERED without qbp_layered_configure");
    if (variant == QBP_DAMPED_SP) return fail(QBP_E_INVALID, "QBP_FLAG_LAYERED with QBP_DAMPED_SP: no damped layered schedule");
    if (flags & (QBP_FLAG_PAIRWISE_COLSUM | QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0))
        return fail(QBP_E_INVALID, "QBP_FLAG_LAYERED with a column-sum order flag: the layered schedule has no column sum");
    return layered_build(h);            // (QBP_OPT_LAYERED_MEM may have changed since qbp_layered_configure)
}

// One launch of bp_layered_kernel (device pointers): the batch build, or (c.mc) the Monte-Carlo build on stored errors
static int layered_launch(qbp_handle* h, const BpCall& c, hipStream_t s)
{
    constexpr long long MAX_LAUNCH = (long long)1 << 30;       // (records are handed out through a 32-bit counter)
    if (c.B > MAX_LAUNCH)
        return fail(QBP_E_UNSUPPORTED, "layered BP decodes at most 2^30 syndromes per call (got %lld)", c.B);
    bool large = false;
    const int rc0 = layered_build(h, &large);
    if (rc0) return rc0;
    const bool tables = c.variant == QBP_SUM_PRODUCT;
    const int S = layered_slots(h, c.B, tables, large);
    const size_t lds = layered_build_lds(h, large, S, tables);
    // resident workgroups per CU: the LDS, and five wavefronts per SIMD at the kernel's registers
    int per_cu = (int)std::max<size_t>(1, std::min<size_t>(5, ((size_t)160 * 1024) / lds));
    if (h->opt_blocks_per_cu > 0) per_cu = h->opt_blocks_per_cu;
    const long long groups = (c.B + S - 1) / S;
    const int grid = (int)std::max<long long>(1, std::min<long long>(groups, (long long)h->num_cu * per_cu));
    HIP_TRY(hipMemsetAsync(h->d_work_counter.p, 0, sizeof(unsigned long long), s));
    qbp::LayeredParams P{};
    P.m = h->m; P.n = h->n; P.E = h->E; P.n_levels = h->layered_levels; P.S = S;
    P.row_ptr = h->d_row_ptr.p; P.col_idx = h->d_col_idx.p;
    P.order = h->d_layered_order.p; P.level_ptr = h->d_layered_level_ptr.p;
    P.prior = c.prior; P.work_counter = reinterpret_cast<unsigned*>(h->d_work_counter.p);
    P.max_iter = c.max_iter; P.flags = (c.flags & QBP_FLAG_FORCE_FULL) ? qbp::LAYERED_FORCE_FULL : 0u;
    P.alpha = c.alpha; P.clip_llr = c.clip_llr; P.B = c.B;
    P.syndromes = c.syndromes; P.hard = c.hard; P.converged = c.converged; P.iters = c.iters; P.llr = c.llr;
    if (c.mc) {
        P.errors_in = c.mc->errors_in; P.lx_cols = c.mc->lx_cols; P.half_distance = c.mc->half_distance;
        P.counters = c.mc->counters;
        P.fail_list = c.mc->fail_list; P.fail_count = c.mc->fail_count; P.fail_syn = c.mc->fail_syn;
        P.fail_hard = c.mc->fail_hard; P.fail_err = c.mc->fail_err; P.fail_llr = c.mc->fail_llr;
    }
    if (large) {                 // a slice of E doubles per slot of every workgroup
        const int rc = large_workspace(h->d_layered_wsR, (size_t)grid * (size_t)S * (size_t)h->E, &P.wsR);
        if (rc) return rc;
    }
    h->last_threads = qbp::LAYERED_THREADS; h->last_lds = (int)lds; h->last_grid = grid;
    HIP_TRY(qbp::launch_layered(c.mc != nullptr, large, c.variant, P, grid, lds, s));
    return QBP_OK;
}

int qbp_layered_plan(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, const int32_t* order_in,
                     int32_t* order_out, int32_t* level_ptr, int32_t* n_levels)
try {
    int rc = check_csr(row_ptr, col_idx, m, n);
    if (rc) return rc;
    if (!order_out || !level_ptr || !n_levels) return fail(QBP_E_INVALID, "null output pointer");
    std::vector<int32_t> order, lptr;
    if ((rc = layered_plan(row_ptr, col_idx, m, n, order_in, order, lptr)) != QBP_OK) return rc;
    std::copy(order.begin(), order.end(), order_out);
    std::fill(level_ptr, level_ptr + m + 1, (int32_t)m);
    std::copy(lptr.begin(), lptr.end(), level_ptr);
    *n_levels = (int32_t)lptr.size() - 1;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_layered_configure(qbp_handle* h, const int32_t* order)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    int rc = layered_build(h);
    if (rc) return rc;
    std::vector<int32_t> ord, lptr;
    if ((rc = layered_plan(h->row_ptr.data(), h->col_idx.data(), h->m, h->n, order, ord, lptr)) != QBP_OK) return rc;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    HIP_TRY(hipStreamSynchronize(h->stream));       // (a launch of this handle's stream may still read the old tables)
    h->layered_ready = false;
    HIP_TRY(h->d_layered_order.upload(ord));
    HIP_TRY(h->d_layered_level_ptr.upload(lptr));
    h->layered_levels = (int)lptr.size() - 1;
    h->layered_max_width = 1;
    for (size_t l = 0; l + 1 < lptr.size(); ++l) h->layered_max_width = std::max(h->layered_max_width, lptr[l + 1] - lptr[l]);
    h->layered_ready = true;
    return QBP_OK;
}
QBP_ABI_CATCH

// ---- fixed-point min-sum (qbp_quant.hpp) -------------------------------------------------------------------------
// Slots per workgroup: about four work items per thread in the variable step, at most QUANT_MAX_SLOTS and what keeps
// two workgroups' LDS on a CU; one slot always (qbp_quant_configure refuses what does not fit with one).
static int quant_slots(const qbp_handle* h, long long B)
{
    const bool wide = h->quant_bits > 8;
    int S = h->opt_quant_slots;
    if (S <= 0) {
        S = std::max(1, std::min(qbp::QUANT_MAX_SLOTS, 4 * qbp::QUANT_THREADS / std::max(1, h->n)));
        while (S > 1 && qbp::quant_lds_bytes(h->m, h->n, h->E, S, wide) > (size_t)80 * 1024) --S;
    }
    while (S > 1 && qbp::quant_lds_bytes(h->m, h->n, h->E, S, wide) > (size_t)160 * 1024) --S;
    return (int)std::max<long long>(1, std::min<long long>(S, B));
}

// QBP_FLAG_QUANT of a call (host only, before any GPU work).  `other_entry`: the entries without a fixed-point build
// (double-precision batch decodes, budgets, spectra, histograms, recorded shots, message dumps).
static int check_quant_flags(const qbp_handle* h, uint32_t flags, int variant, bool other_entry)
{
    if (!(flags & QBP_FLAG_QUANT)) return QBP_OK;
    if (other_entry)
        return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_QUANT is a first stage of qbp_mc_run, _errors, _probs and _weight only "
                                       "(batches: qbp_quant_decode_batch)");
    if (!h->quant_ready) return fail(QBP_E_INVALID, "QBP_FLAG_QUANT without qbp_quant_configure");
    if (flags & QBP_FLAG_LAYERED) return fail(QBP_E_INVALID, "QBP_FLAG_QUANT with QBP_FLAG_LAYERED: one first stage per call");
    if (variant != QBP_MIN_SUM) return fail(QBP_E_INVALID, "QBP_FLAG_QUANT with variant %d: fixed-point BP is QBP_MIN_SUM", variant);
    if (flags & (QBP_FLAG_PAIRWISE_COLSUM | QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0))
        return fail(QBP_E_INVALID, "QBP_FLAG_QUANT with a column-sum order flag: integer sums have no order");
    return QBP_OK;
}

// One launch of bp_quant_kernel (device pointers): the batch build, or (c.mc) the Monte-Carlo build on stored errors
static int quant_launch(qbp_handle* h, const BpCall& c, int32_t* posterior_q, hipStream_t s)
{
    constexpr long long MAX_LAUNCH = (long long)1 << 30;       // (records are handed out through a 32-bit counter)
    if (c.B > MAX_LAUNCH)
        return fail(QBP_E_UNSUPPORTED, "fixed-point BP decodes at most 2^30 syndromes per call (got %lld)", c.B);
    const bool wide = h->quant_bits > 8;
    const int S = quant_slots(h, c.B);
    const size_t lds = qbp::quant_lds_bytes(h->m, h->n, h->E, S, wide);
    // resident workgroups per CU: the LDS, and eight wavefronts per SIMD
    int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, ((size_t)160 * 1024) / lds));
    if (h->opt_blocks_per_cu > 0) per_cu = h->opt_blocks_per_cu;
    const long long groups = (c.B + S - 1) / S;
    const int grid = (int)std::max<long long>(1, std::min<long long>(groups, (long long)h->num_cu * per_cu));
    HIP_TRY(hipMemsetAsync(h->d_work_counter.p, 0, sizeof(unsigned long long), s));
    qbp::QuantParams P{};
    P.m = h->m; P.n = h->n; P.E = h->E; P.S = S;
    P.row_ptr = h->d_row_ptr.p; P.col_idx = h->d_col_idx.p; P.col_ptr = h->d_col_ptr.p; P.col_edge = h->d_col_edge.p;
    P.prior = c.prior; P.work_counter = reinterpret_cast<unsigned*>(h->d_work_counter.p);
    P.max_iter = c.max_iter; P.flags = (c.flags & QBP_FLAG_FORCE_FULL) ? qbp::QUANT_FORCE_FULL : 0u;
    P.M = (1 << (h->quant_bits - 1)) - 1; P.scale = h->quant_scale;
    P.alpha_num = h->quant_num; P.alpha_shift = h->quant_shift; P.beta = h->quant_beta; P.B = c.B;
    P.syndromes = c.syndromes; P.hard = c.hard; P.converged = c.converged; P.iters = c.iters;
    P.posterior_q = posterior_q; P.llr = c.llr;
    if (c.mc) {
        P.errors_in = c.mc->errors_in; P.lx_cols = c.mc->lx_cols; P.half_distance = c.mc->half_distance;
        P.counters = c.mc->counters;
        P.fail_list = c.mc->fail_list; P.fail_count = c.mc->fail_count; P.fail_syn = c.mc->fail_syn;
        P.fail_hard = c.mc->fail_hard; P.fail_err = c.mc->fail_err; P.fail_llr = c.mc->fail_llr;
    }
    h->last_threads = qbp::QUANT_THREADS; h->last_lds = (int)lds; h->last_grid = grid; h->last_kernel = 5;
    HIP_TRY(qbp::launch_quant(c.mc != nullptr, wide, P, grid, lds, s));
    return QBP_OK;
}

int qbp_quant_configure(qbp_handle* h, int32_t bits, double scale, int32_t alpha_num, int32_t alpha_shift, int32_t beta)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (bits < 2 || bits > 16) return fail(QBP_E_INVALID, "bits = %d out of [2, 16]", bits);
    const int M = (1 << (bits - 1)) - 1;
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail(QBP_E_INVALID, "scale = %g must be finite and > 0", scale);
    if (alpha_shift < 0 || alpha_shift > 15) return fail(QBP_E_INVALID, "alpha_shift = %d out of [0, 15]", alpha_shift);
    if (alpha_num < 1 || alpha_num > (1 << alpha_shift))
        return fail(QBP_E_INVALID, "alpha_num = %d out of [1, 2^%d]", alpha_num, alpha_shift);
    if (beta < 0 || beta > M) return fail(QBP_E_INVALID, "beta = %d out of [0, %d]", beta, M);
    if (h->max_col_deg > 32767)
        return fail(QBP_E_UNSUPPORTED, "fixed-point BP sums a column in int32: columns of at most 32767 entries (got %d)",
                    h->max_col_deg);
    const size_t lds = qbp::quant_lds_bytes(h->m, h->n, h->E, 1, bits > 8);
    if (lds > (size_t)160 * 1024)
        return fail(QBP_E_UNSUPPORTED, "fixed-point BP keeps the messages, the posterior and the prior of a record in LDS: "
                                       "%d x %d with %d entries at %d bits needs %zu B (limit 160 KiB)", h->m, h->n, h->E,
                    bits, lds);
    h->quant_bits = bits; h->quant_scale = scale; h->quant_num = alpha_num; h->quant_shift = alpha_shift;
    h->quant_beta = beta;
    h->quant_ready = true;
    return QBP_OK;
}
QBP_ABI_CATCH

// Everything qbp_quant_decode_batch refuses apart from null pointers and NaN priors: host only, before any GPU work.
static int quant_check_batch(qbp_handle* h, int64_t B, int32_t max_iter, uint32_t flags)
{
    const int rc = check_decode_args(h, B, max_iter, QBP_MIN_SUM);
    if (rc) return rc;
    if (!h->quant_ready) return fail(QBP_E_INVALID, "qbp_quant_decode_batch without qbp_quant_configure");
    if (flags & ~(uint32_t)(QBP_FLAG_FORCE_FULL | QBP_FLAG_FAST_MATH))
        return fail(QBP_E_INVALID, "flags 0x%x: qbp_quant_decode_batch takes QBP_FLAG_FORCE_FULL only", flags);
    return QBP_OK;
}

int qbp_quant_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                                  int32_t max_iter, uint32_t flags, uint8_t* d_hard, uint8_t* d_converged,
                                  int32_t* d_iters, int32_t* d_posterior_q, double* d_llr, void* stream)
try {
    const int rc = quant_check_batch(h, B, max_iter, flags);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_prior) return fail(QBP_E_INVALID, "null input pointer");
    if (!d_hard) return fail(QBP_E_INVALID, "hard is null");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    BpCall c;
    c.syndromes = d_syndromes; c.prior = d_prior; c.B = B; c.max_iter = max_iter; c.variant = QBP_MIN_SUM;
    c.flags = flags & QBP_FLAG_FORCE_FULL;
    c.hard = d_hard; c.converged = d_converged; c.iters = d_iters; c.llr = d_llr;
    return quant_launch(h, c, d_posterior_q, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_quant_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, int32_t max_iter,
                           uint32_t flags, uint8_t* hard, uint8_t* converged, int32_t* iters, int32_t* posterior_q,
                           double* llr)
try {
    int rc = quant_check_batch(h, B, max_iter, flags);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!syndromes || !prior) return fail(QBP_E_INVALID, "null input pointer");
    if (!hard) return fail(QBP_E_INVALID, "hard is null");
    if ((rc = check_prior(h->n, prior, false)) != QBP_OK) return rc;
    if (B > (int64_t)1 << 30) return fail(QBP_E_UNSUPPORTED, "fixed-point BP decodes at most 2^30 syndromes per call");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t m = h->m, n = h->n, b = (size_t)B;
    HostStage st(h->stream);
    const uint8_t* d_syn = st.in(h->d_syn, syndromes, b * m);
    const double* d_prior = st.in(h->d_prior, prior, n);
    uint8_t* d_hard = st.out(h->d_hard, hard, b * n);
    uint8_t* d_conv = st.out(h->d_conv, converged, b);
    int32_t* d_iters = st.out(h->d_iters, iters, b);
    int32_t* d_post = st.out(h->d_quant_post, posterior_q, b * n);
    double* d_llr = st.out(h->d_llr, llr, b * n);
    if (st.failed()) return st.error();
    return st.finish(qbp_quant_decode_batch_device(h, d_syn, d_prior, B, max_iter, flags, d_hard, d_conv, d_iters, d_post,
                                                   d_llr, h->stream));
}
QBP_ABI_CATCH

// ---- Relay-BP (qbp_relay.hpp) ------------------------------------------------------------------------------------
// Dynamic LDS of a workgroup in the build `large`
static size_t relay_build_lds(const qbp_handle* h, bool large, bool records)
{
    return large ? qbp::relay_large_lds_bytes(h->m, h->n, records) : qbp::relay_lds_bytes(h->m, h->n, h->E, records);
}

// QBP_OPT_RELAY_MEM (qbp_msg_mem.hpp), decided on the batch or the records build.  Matrices beyond the LDS of the build
// the option allows are QBP_E_UNSUPPORTED (host only); *large: the build of a launch.
static int relay_build(const qbp_handle* h, bool records, bool* large = nullptr)
{
    const qbp::MsgMemChoice c = qbp::msg_mem_choose(
        h->opt_msg_mem[qbp::MSG_MEM_RELAY], relay_build_lds(h, false, records), relay_build_lds(h, true, records),
        [h](bool large_build, size_t need) {
            if (large_build)
                fail(QBP_E_UNSUPPORTED, "Relay-BP with the messages in global memory keeps a row of n doubles in LDS: "
                                        "%d x %d needs %zu B (limit 160 KiB)", h->m, h->n, need);
            else
                fail(QBP_E_UNSUPPORTED, "Relay-BP keeps the messages and three rows of n doubles in LDS: %d x %d with %d "
                                        "entries needs %zu B (limit 160 KiB)", h->m, h->n, h->E, need);
        });
    if (large) *large = c.large;
    return c.ok ? QBP_OK : QBP_E_UNSUPPORTED;
}

// QBP_FLAG_RELAY of a Monte-Carlo call (host only, before any GPU work).  `other_entry`: the budgets, spectrum and
// shots entries, which have no Relay stage.
static int check_relay_flags(const qbp_handle* h, uint32_t flags, bool other_entry)
{
    if (!(flags & QBP_FLAG_RELAY)) return QBP_OK;
    if (flags & (QBP_FLAG_OSD0 | OSD_ALL_BITS))
        return fail(QBP_E_INVALID, "QBP_FLAG_RELAY together with an OSD bit: one second stage per call");
    if (other_entry)
        return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_RELAY is not available with iteration budgets, spectra or recorded shots");
    if (!h->relay_ready) return fail(QBP_E_INVALID, "QBP_FLAG_RELAY without qbp_relay_configure");
    return relay_build(h, true);        // (QBP_OPT_RELAY_MEM may have changed since qbp_relay_configure)
}

// One launch of bp_relay_kernel or bp_gd_kernel (device pointers): a batch of syndromes, or the failure records of a
// Monte-Carlo launch
struct RecordCall {
    const double* prior = nullptr;
    long long max_items = 0;            // B, or the most records the list can hold
    const uint8_t* syndromes = nullptr;
    uint8_t* hard = nullptr;
    uint8_t* converged = nullptr;
    int32_t* iters = nullptr;
    double* llr = nullptr;
    int32_t* extra[2] = {nullptr, nullptr};     // Relay-BP: legs, solutions; BP guided decimation: rounds
    const unsigned long long* fail_count = nullptr;
    const long long* fail_list = nullptr;
    const uint8_t* fail_syn = nullptr;
    const uint8_t* fail_err = nullptr;
    int half_distance = 0;
    long long* counters = nullptr;
};

// What the launches of the two kernels share: the limit of a call, the grid -- resident workgroups per CU: `waves`
// wavefronts at the kernel's registers, and the LDS; QBP_OPT_BLOCKS_PER_CU overrides where the decoder honours it --,
// the workspace, the sorted prior, the work counter, the tables of the general-H kernel (P) and the inputs and outputs of
// the call (io).  *grid: the workgroups to launch.
struct RecordGeometry {
    const char* name;           // of the decoder, for messages
    size_t lds;
    int threads, waves;
    bool honours_blocks_per_cu;
};
static int record_launch_setup(qbp_handle* h, const RecordCall& c, bool records, const RecordGeometry& g, hipStream_t s,
                               qbp::RecordTables& P, qbp::RecordIo& io, int* grid_out)
{
    constexpr int RC = qbp::GENERIC_MAX_ROW_CLASS;
    constexpr long long MAX_LAUNCH = (long long)1 << 30;       // (records are handed out through a 32-bit counter)
    if (c.max_items > MAX_LAUNCH)
        return fail(QBP_E_UNSUPPORTED, "%s decodes at most 2^30 syndromes per call (got %lld)", g.name, c.max_items);
    const size_t n = (size_t)h->n;
    int per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)(g.waves / (g.threads / 64)), ((size_t)160 * 1024) / g.lds));
    if (g.honours_blocks_per_cu && h->opt_blocks_per_cu > 0) per_cu = h->opt_blocks_per_cu;
    const int grid = (int)std::max<long long>(1, std::min<long long>(c.max_items, (long long)h->num_cu * per_cu));
    const size_t n_long = (size_t)(h->row_off[RC + 2] - h->row_off[RC + 1]);
    HIP_TRY(h->d_wsL.reserve((size_t)grid * 3 * std::max<size_t>(n_long, 1)));
    HIP_TRY(h->d_prior_sorted.reserve(n));
    HIP_TRY(qbp::launch_permute_prior(c.prior, h->d_svar.p, h->d_prior_sorted.p, (int)n, s));
    HIP_TRY(hipMemsetAsync(h->d_work_counter.p, 0, sizeof(unsigned long long), s));
    P.m = h->m; P.n = h->n; P.E = h->E;
    P.srow = h->d_srow.p; P.srow_e0 = h->d_srow_e0.p; P.srow_deg = h->d_srow_deg.p; P.epos = h->d_epos.p;
    P.long_edge_row = h->d_long_edge_row.p; P.svar = h->d_svar.p; P.vpos = h->d_vpos.p; P.vrow = h->d_vrow.p;
    P.lcol_ptr = h->d_lcol_ptr.p;
    std::copy(std::begin(h->row_off), std::end(h->row_off), P.row_off);
    std::copy(std::begin(h->row_base), std::end(h->row_base), P.row_base);
    std::copy(std::begin(h->rpad_off), std::end(h->rpad_off), P.rpad_off);
    std::copy(std::begin(h->col_off), std::end(h->col_off), P.col_off);
    std::copy(std::begin(h->gcol_base), std::end(h->gcol_base), P.col_base);
    std::copy(std::begin(h->cpad_off), std::end(h->cpad_off), P.cpad_off);
    P.prior_sorted = h->d_prior_sorted.p; P.wsL = h->d_wsL.p;
    P.work_counter = reinterpret_cast<unsigned*>(h->d_work_counter.p);
    io.syndromes = c.syndromes; io.B = records ? 0 : c.max_items;
    io.hard = c.hard; io.converged = c.converged; io.iters = c.iters; io.llr = c.llr;
    io.fail_count = c.fail_count; io.fail_list = c.fail_list; io.fail_syn = c.fail_syn; io.fail_err = c.fail_err;
    io.lx_cols = h->mc_in.d_lx_cols.p; io.half_distance = c.half_distance; io.counters = c.counters;
    h->last_threads = g.threads; h->last_lds = (int)g.lds; h->last_grid = grid;
    *grid_out = grid;
    return QBP_OK;
}

extern "C++" {       // (a template: not in the C linkage of the entry points around it)
// The host-pointer entry of both decoders after its argument checks: finite prior, staging, the device entry
// (entry(d_hard, d_converged, d_iters, d_llr, d_extra0, d_extra1, stream)), download.  extra / d_extra: the decoder's
// own int32 columns and their scratch (a slot it does not have is null).
template <class Entry>
static int record_decode_batch_host(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, uint8_t* hard,
                                    uint8_t* converged, int32_t* iters, double* llr, int32_t* const (&extra)[2],
                                    DevBuf<int32_t>* const (&d_extra)[2], const Entry& entry)
{
    const int rc = check_prior(h->n, prior, true);
    if (rc) return rc;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t m = h->m, n = h->n, b = (size_t)B;
    HostStage st(h->stream);
    st.in(h->d_syn, syndromes, b * m);          // (the entries read h->d_syn.p and h->d_prior.p)
    st.in(h->d_prior, prior, n);
    uint8_t* d_hard = st.out(h->d_hard, hard, b * n);
    uint8_t* d_conv = st.out(h->d_conv, converged, b);
    int32_t* d_iters = st.out(h->d_iters, iters, b);
    double* d_llr = st.out(h->d_llr, llr, b * n);
    int32_t* d_x[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k)
        if (d_extra[k]) d_x[k] = st.out(*d_extra[k], extra[k], b);
    if (st.failed()) return st.error();
    return st.finish(entry(d_hard, d_conv, d_iters, d_llr, d_x[0], d_x[1], h->stream));
}

}  // extern "C++"

static int relay_launch(qbp_handle* h, const RecordCall& c, bool records, hipStream_t s)
{
    constexpr int RC = qbp::GENERIC_MAX_ROW_CLASS, CC = qbp::GENERIC_MAX_COL_CLASS;
    // (QBP_OPT_RELAY_MEM may have changed since qbp_relay_configure)
    bool large = false;
    const int rc0 = relay_build(h, records, &large);
    if (rc0) return rc0;
    const size_t lds = relay_build_lds(h, large, records);
    const int threads = qbp::record_threads(h->rpad_off[RC + 1], h->cpad_off[CC + 1], qbp::RELAY_MAX_THREADS);
    qbp::RelayParams P{};
    int grid = 0;
    // wavefronts per CU at the kernel's registers: 28, large build 24; QBP_OPT_BLOCKS_PER_CU is not honoured
    const int rc = record_launch_setup(h, c, records, {"Relay-BP", lds, threads, large ? 24 : 28, false}, s, P.tab, P.io,
                                       &grid);
    if (rc) return rc;
    if (large) {
        const int rcw = large_workspace(h->d_wsM, (size_t)grid * (size_t)h->E, &P.wsM);
        if (rcw) return rcw;
    }
    P.vinv = h->d_relay_vinv.p; P.prior = c.prior;
    P.gammas_sorted = h->d_relay_gammas.p; P.leg_iters = h->d_relay_iters.p;
    P.L = h->relay_L; P.stop_after = h->relay_stop_after; P.alpha = h->relay_alpha; P.clip_llr = h->relay_clip;
    P.legs = c.extra[0]; P.solutions = c.extra[1];
    HIP_TRY(qbp::launch_relay(records, large, P, grid, threads, lds, s));
    return QBP_OK;
}

int qbp_relay_configure(qbp_handle* h, const double* gammas, int32_t L, const int32_t* leg_iters, int32_t stop_after,
                        double alpha, double clip_llr)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (!gammas || !leg_iters) return fail(QBP_E_INVALID, "null pointer");
    if (L < 1) return fail(QBP_E_INVALID, "L = %d legs (need >= 1)", L);
    if (stop_after < 1) return fail(QBP_E_INVALID, "stop_after = %d (need >= 1)", stop_after);
    if (!std::isfinite(alpha) || !std::isfinite(clip_llr))
        return fail(QBP_E_INVALID, "alpha = %g, clip_llr = %g: both must be finite", alpha, clip_llr);
    const size_t n = (size_t)h->n;
    for (int l = 0; l < L; ++l) {
        if (leg_iters[l] < 1) return fail(QBP_E_INVALID, "leg_iters[%d] = %d (need >= 1)", l, leg_iters[l]);
        for (size_t v = 0; v < n; ++v)
            if (!std::isfinite(gammas[(size_t)l * n + v]))
                return fail(QBP_E_INVALID, "gammas[%d][%zu] is not finite", l, v);
    }
    const int rc = relay_build(h, false);
    if (rc) return rc;
    // the tables follow the kernel's variable order: sorted by column weight (build_tables)
    HostTables T;
    const int rc2 = build_tables(h->row_ptr.data(), h->col_idx.data(), h->m, h->n, T);
    if (rc2) return rc2;
    std::vector<double> sorted((size_t)L * n);
    std::vector<int32_t> vinv(n);
    for (size_t x = 0; x < n; ++x) {
        vinv[T.svar[x]] = (int32_t)x;
        for (int l = 0; l < L; ++l) sorted[(size_t)l * n + x] = gammas[(size_t)l * n + T.svar[x]];
    }
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    HIP_TRY(hipStreamSynchronize(h->stream));       // (a launch of this handle's stream may still read the old tables)
    h->relay_ready = false;
    HIP_TRY(h->d_relay_gammas.upload(sorted));
    HIP_TRY(h->d_relay_vinv.upload(vinv));
    HIP_TRY(h->d_relay_iters.upload(std::vector<int32_t>(leg_iters, leg_iters + L)));
    h->relay_L = L; h->relay_stop_after = stop_after; h->relay_alpha = alpha; h->relay_clip = clip_llr;
    h->relay_ready = true;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_relay_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                                  uint8_t* d_hard, uint8_t* d_converged, int32_t* d_iters, double* d_llr,
                                  int32_t* d_legs, int32_t* d_solutions, void* stream)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", (long long)B);
    if (!h->relay_ready) return fail(QBP_E_INVALID, "qbp_relay_decode_batch without qbp_relay_configure");
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_prior) return fail(QBP_E_INVALID, "null input pointer");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    RecordCall c;
    c.prior = d_prior; c.max_items = B; c.syndromes = d_syndromes;
    c.hard = d_hard; c.converged = d_converged; c.iters = d_iters; c.llr = d_llr;
    c.extra[0] = d_legs; c.extra[1] = d_solutions;
    return relay_launch(h, c, false, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_relay_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, uint8_t* hard,
                           uint8_t* converged, int32_t* iters, double* llr, int32_t* legs, int32_t* solutions)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", (long long)B);
    if (!h->relay_ready) return fail(QBP_E_INVALID, "qbp_relay_decode_batch without qbp_relay_configure");
    if (B == 0) return QBP_OK;
    if (!syndromes || !prior) return fail(QBP_E_INVALID, "null input pointer");
    int32_t* const extra[2] = {legs, solutions};
    DevBuf<int32_t>* const d_extra[2] = {&h->d_relay_legs, &h->d_relay_sol};
    return record_decode_batch_host(h, syndromes, prior, B, hard, converged, iters, llr, extra, d_extra,
                                    [&](uint8_t* d_hard, uint8_t* d_conv, int32_t* d_iters, double* d_llr, int32_t* d_legs,
                                        int32_t* d_sol, hipStream_t s) {
                                        return qbp_relay_decode_batch_device(h, h->d_syn.p, h->d_prior.p, B, d_hard, d_conv,
                                                                             d_iters, d_llr, d_legs, d_sol, s);
                                    });
}
QBP_ABI_CATCH

// ---- BP guided decimation (qbp_gd.hpp) ---------------------------------------------------------------------------
// Dynamic LDS of a workgroup in the build `large`
static size_t gd_build_lds(const qbp_handle* h, bool large, bool sp)
{
    return large ? qbp::gd_large_lds_bytes(h->m, h->n, sp) : qbp::gd_lds_bytes(h->m, h->n, h->E, sp);
}

// QBP_OPT_GD_MEM (qbp_msg_mem.hpp), decided on the variant.  Matrices beyond the LDS of the build the option allows
// are QBP_E_UNSUPPORTED (host only); *large: the build of a launch.
static int gd_build(const qbp_handle* h, int variant, bool* large = nullptr)
{
    const bool sp = variant == QBP_SUM_PRODUCT;
    const qbp::MsgMemChoice c = qbp::msg_mem_choose(
        h->opt_msg_mem[qbp::MSG_MEM_GD], gd_build_lds(h, false, sp), gd_build_lds(h, true, sp),
        [h](bool large_build, size_t need) {
            if (large_build)
                fail(QBP_E_UNSUPPORTED, "BP guided decimation with the messages in global memory keeps a row of n "
                                        "doubles in LDS: %d x %d needs %zu B (limit 160 KiB)", h->m, h->n, need);
            else
                fail(QBP_E_UNSUPPORTED, "BP guided decimation keeps the messages and two rows of n doubles in LDS: %d x %d "
                                        "with %d entries needs %zu B (limit 160 KiB)", h->m, h->n, h->E, need);
        });
    if (large) *large = c.large;
    return c.ok ? QBP_OK : QBP_E_UNSUPPORTED;
}

// QBP_FLAG_GD of a Monte-Carlo call (host only, before any GPU work).  `other_entry`: the budgets, spectrum and shots
// entries, which have no such stage.
static int check_gd_flags(const qbp_handle* h, uint32_t flags, bool other_entry)
{
    if (!(flags & QBP_FLAG_GD)) return QBP_OK;
    if (flags & (QBP_FLAG_OSD0 | OSD_ALL_BITS | QBP_FLAG_RELAY))
        return fail(QBP_E_INVALID, "QBP_FLAG_GD together with an OSD bit or QBP_FLAG_RELAY: one second stage per call");
    if (other_entry)
        return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_GD is not available with iteration budgets, spectra or recorded shots");
    if (!h->gd_ready) return fail(QBP_E_INVALID, "QBP_FLAG_GD without qbp_gd_configure");
    return gd_build(h, h->gd_variant);          // (QBP_OPT_GD_MEM may have changed since qbp_gd_configure)
}

static int gd_launch(qbp_handle* h, const RecordCall& c, bool records, hipStream_t s)
{
    constexpr int RC = qbp::GENERIC_MAX_ROW_CLASS, CC = qbp::GENERIC_MAX_COL_CLASS;
    const bool sp = h->gd_variant == QBP_SUM_PRODUCT;
    // (QBP_OPT_GD_MEM may have changed since qbp_gd_configure)
    bool large = false;
    const int rc0 = gd_build(h, h->gd_variant, &large);
    if (rc0) return rc0;
    const size_t lds = gd_build_lds(h, large, sp);
    const int threads = qbp::record_threads(h->rpad_off[RC + 1], h->cpad_off[CC + 1], qbp::GD_MAX_THREADS);
    qbp::GdParams P{};
    int grid = 0;
    // the wavefronts a CU holds at the kernel's registers: min-sum 7 per SIMD, sum-product 5; the large build 6 and 4
    // (80 and 109 registers); QBP_OPT_BLOCKS_PER_CU overrides
    const int waves = large ? (sp ? 16 : 24) : (sp ? 20 : 28);
    const int rc = record_launch_setup(h, c, records, {"BP guided decimation", lds, threads, waves, true}, s, P.tab, P.io,
                                       &grid);
    if (rc) return rc;
    P.iters_per_round = h->gd_iters; P.max_rounds = h->gd_max_rounds; P.decim_llr = h->gd_llr;
    P.alpha = h->gd_alpha; P.clip_llr = h->gd_clip;
    P.rounds = c.extra[0];
    if (large) {                 // (Relay's buffer: qbp_handle says why)
        const int rcw = large_workspace(h->d_wsM, (size_t)grid * (size_t)h->E, &P.wsM);
        if (rcw) return rcw;
    }
    HIP_TRY(qbp::launch_gd(records, large, h->gd_variant, P, grid, threads, lds, s));
    return QBP_OK;
}

int qbp_gd_configure(qbp_handle* h, int32_t iters_per_round, int32_t max_rounds, double decim_llr, int32_t variant,
                     double alpha, double clip_llr)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (iters_per_round < 1) return fail(QBP_E_INVALID, "iters_per_round = %d (need >= 1)", iters_per_round);
    if (max_rounds < 0) return fail(QBP_E_INVALID, "max_rounds = %d (need >= 0)", max_rounds);
    if (!(decim_llr > 0.0) || !std::isfinite(decim_llr))
        return fail(QBP_E_INVALID, "decim_llr = %g (need > 0 and finite)", decim_llr);
    if (variant != QBP_SUM_PRODUCT && variant != QBP_MIN_SUM)
        return fail(QBP_E_INVALID, "variant = %d: BP guided decimation runs QBP_SUM_PRODUCT or QBP_MIN_SUM", variant);
    if (!std::isfinite(alpha) || !std::isfinite(clip_llr))
        return fail(QBP_E_INVALID, "alpha = %g, clip_llr = %g: both must be finite", alpha, clip_llr);
    const int rc = gd_build(h, variant);
    if (rc) return rc;
    h->gd_iters = iters_per_round; h->gd_max_rounds = max_rounds; h->gd_llr = decim_llr; h->gd_variant = variant;
    h->gd_alpha = alpha; h->gd_clip = clip_llr;
    h->gd_ready = true;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_gd_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                               uint8_t* d_hard, uint8_t* d_converged, int32_t* d_iters, double* d_llr, int32_t* d_rounds,
                               void* stream)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", (long long)B);
    if (!h->gd_ready) return fail(QBP_E_INVALID, "qbp_gd_decode_batch without qbp_gd_configure");
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_prior) return fail(QBP_E_INVALID, "null input pointer");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    RecordCall c;
    c.prior = d_prior; c.max_items = B; c.syndromes = d_syndromes;
    c.hard = d_hard; c.converged = d_converged; c.iters = d_iters; c.llr = d_llr; c.extra[0] = d_rounds;
    return gd_launch(h, c, false, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_gd_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, uint8_t* hard,
                        uint8_t* converged, int32_t* iters, double* llr, int32_t* rounds)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", (long long)B);
    if (!h->gd_ready) return fail(QBP_E_INVALID, "qbp_gd_decode_batch without qbp_gd_configure");
    if (B == 0) return QBP_OK;
    if (!syndromes || !prior) return fail(QBP_E_INVALID, "null input pointer");
    int32_t* const extra[2] = {rounds, nullptr};
    DevBuf<int32_t>* const d_extra[2] = {&h->d_gd_rounds, nullptr};
    return record_decode_batch_host(h, syndromes, prior, B, hard, converged, iters, llr, extra, d_extra,
                                    [&](uint8_t* d_hard, uint8_t* d_conv, int32_t* d_iters, double* d_llr, int32_t* d_rounds,
                                        int32_t*, hipStream_t s) {
                                        return qbp_gd_decode_batch_device(h, h->d_syn.p, h->d_prior.p, B, d_hard, d_conv,
                                                                          d_iters, d_llr, d_rounds, s);
                                    });
}
QBP_ABI_CATCH

// ---- Localized statistics decoding (qbp_lsd.hpp) ------------------------------------------------------------------
// Dynamic LDS of a workgroup in the build `large` (lsd_kernel: before rounding up to 16)
static size_t lsd_build_lds(const qbp_handle* h, bool large)
{
    return large ? qbp::lsd_large_lds_bytes(h->m, h->n, h->osd_NP) : qbp::lsd_lds_bytes(h->m, h->n, h->osd_W, h->osd_NP);
}

// QBP_OPT_LSD_MEM (qbp_msg_mem.hpp).  lsd_kernel keeps a record's rows of [H | syndrome] and its cluster tables in LDS,
// a lane tracks its rows in a 32-bit mask, and columns are 16-bit in both kernels; lsd_large_kernel keeps the tables
// alone in LDS.  A limit that is no byte count enters the choice as a size beyond the LDS: 2049 rows are a matter for
// the large build.  Matrices beyond the limits of the build the option allows are QBP_E_UNSUPPORTED (host only);
// *large: the build of a launch.
static int lsd_build(const qbp_handle* h, bool* large = nullptr)
{
    const size_t beyond = qbp::MSG_MEM_LDS_LIMIT + 1;
    const size_t lds = lsd_build_lds(h, false), lds_large = lsd_build_lds(h, true);
    const bool wide = h->n > 65535;
    const qbp::MsgMemChoice c = qbp::msg_mem_choose(
        h->opt_msg_mem[qbp::MSG_MEM_LSD], h->m > 64 * 32 || wide ? std::max(lds, beyond) : lds,
        wide ? std::max(lds_large, beyond) : lds_large, [&](bool large_build, size_t) {
            if (large_build)
                fail(QBP_E_UNSUPPORTED, "localized statistics decoding with the rows in global memory keeps its cluster "
                                        "tables in LDS: %d x %d needs %zu B (limits: 160 KiB, 65535 columns)",
                     h->m, h->n, lds_large);
            else
                fail(QBP_E_UNSUPPORTED, "localized statistics decoding keeps the bit-packed rows of H and its cluster tables "
                                        "in LDS: %d x %d needs %zu B (limits: 160 KiB, 2048 rows, 65535 columns)",
                     h->m, h->n, lds);
        });
    if (large) *large = c.large;
    return c.ok ? QBP_OK : QBP_E_UNSUPPORTED;
}

// QBP_FLAG_LSD of a Monte-Carlo call (host only, before any GPU work).  `other_entry`: the budgets, spectrum and shots
// entries, which have no such stage.
static int check_lsd_flags(const qbp_handle* h, uint32_t flags, bool other_entry)
{
    if (!(flags & QBP_FLAG_LSD)) return QBP_OK;
    if (flags & (QBP_FLAG_OSD0 | OSD_ALL_BITS | QBP_FLAG_RELAY | QBP_FLAG_GD))
        return fail(QBP_E_INVALID, "QBP_FLAG_LSD together with an OSD bit, QBP_FLAG_RELAY or QBP_FLAG_GD: one second stage "
                                   "per call");
    if (other_entry)
        return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_LSD is not available with iteration budgets, spectra or recorded shots");
    if (!h->lsd_ready) return fail(QBP_E_INVALID, "QBP_FLAG_LSD without qbp_lsd_configure");
    return lsd_build(h);                // (QBP_OPT_LSD_MEM may have changed since qbp_lsd_configure)
}

// One launch of lsd_kernel or lsd_large_kernel (device pointers in P: a batch, or the failure records of a Monte-Carlo
// launch)
static int lsd_launch(qbp_handle* h, qbp::LsdParams& P, long long max_items, bool records, hipStream_t s)
{
    // (QBP_OPT_LSD_MEM may have changed since qbp_lsd_configure)
    bool large = false;
    const int rc0 = lsd_build(h, &large);
    if (rc0) return rc0;
    const int rc = osd_prepare(h);      // (the bit-packed rows of H)
    if (rc) return rc;
    P.m = h->m; P.n = h->n; P.W = h->osd_W; P.NP = h->osd_NP;
    P.hbits = h->d_hbits.p; P.row_ptr = h->d_row_ptr.p; P.col_idx = h->d_col_idx.p;
    P.col_ptr = h->d_col_ptr.p; P.col_row = h->d_lsd_col_row.p;
    P.bits_per_step = h->lsd_bits;
    if (large) {
        // one workgroup of four wavefronts per record; per CU the least of: two (the rows stay within the workspace of
        // osd_launch_swaps, d_osd_At [2 num_cu][(W + 1) m] -- 2592 x 7776: one per CU by its LDS, 650 MB on 256 CUs), what
        // the LDS holds, and QBP_OPT_BLOCKS_PER_CU where it is set
        const qbp::LsdLargeLayout L = qbp::lsd_large_layout(h->m, h->n, h->osd_NP);
        long long per_cu = std::max<long long>(1, std::min<long long>(2, (long long)(qbp::MSG_MEM_LDS_LIMIT / L.bytes)));
        if (h->opt_blocks_per_cu > 0) per_cu = std::min<long long>(per_cu, h->opt_blocks_per_cu);
        const long long grid = std::max<long long>(1, std::min<long long>(max_items, (long long)h->num_cu * per_cu));
        qbp::LsdLargeWorkspace Wk{};
        Wk.keys_in_lds = L.keys_in_lds; Wk.region0 = (int)L.region0;
        HIP_TRY(h->d_osd_At.reserve((size_t)grid * (size_t)h->m * ((size_t)h->osd_W + 1)));
        if (!L.keys_in_lds) { HIP_TRY(h->d_osd_keys.reserve((size_t)grid * (size_t)h->osd_NP)); }
        Wk.rows = h->d_osd_At.p; Wk.keys = h->d_osd_keys.p;
        h->last_threads = qbp::LSD_LARGE_THREADS; h->last_lds = (int)L.bytes; h->last_grid = (int)grid;
        HIP_TRY(qbp::launch_lsd_large(records, P, Wk, (unsigned)grid, L.bytes, s));
        return QBP_OK;
    }
    const size_t lds = (qbp::lsd_lds_bytes(h->m, h->n, h->osd_W, h->osd_NP) + 15) & ~(size_t)15;
    // one wavefront per workgroup: as many per CU as the LDS holds, up to osd0_kernel's 32; QBP_OPT_BLOCKS_PER_CU overrides
    long long per_cu = std::max<long long>(1, std::min<long long>(32, (long long)(((size_t)160 * 1024) / lds)));
    if (h->opt_blocks_per_cu > 0) per_cu = h->opt_blocks_per_cu;
    const long long grid = std::max<long long>(1, std::min<long long>(max_items, (long long)h->num_cu * per_cu));
    h->last_threads = 64; h->last_lds = (int)lds; h->last_grid = (int)grid;
    HIP_TRY(qbp::launch_lsd(records, P, (unsigned)grid, lds, s));
    return QBP_OK;
}

int qbp_lsd_configure(qbp_handle* h, int32_t bits_per_step)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (bits_per_step < 0) return fail(QBP_E_INVALID, "bits_per_step = %d (need >= 0)", bits_per_step);
    int rc = lsd_build(h);
    if (rc) return rc;
    if (!h->d_lsd_col_row.p) {
        // the checks of every column in ascending order, at the offsets of d_col_ptr
        DeviceScope on_device(h->device);
        HIP_TRY(on_device.err);
        std::vector<int32_t> at((size_t)h->n + 1, 0), col_row((size_t)std::max(h->E, 1), 0);
        for (int e = 0; e < h->E; ++e) ++at[(size_t)h->col_idx[e] + 1];
        for (int v = 0; v < h->n; ++v) at[(size_t)v + 1] += at[v];
        for (int c = 0; c < h->m; ++c)
            for (int e = h->row_ptr[c]; e < h->row_ptr[c + 1]; ++e) col_row[(size_t)at[h->col_idx[e]]++] = c;
        HIP_TRY(h->d_lsd_col_row.upload(col_row));
        if ((rc = osd_prepare(h)) != QBP_OK) return rc;
    }
    h->lsd_bits = bits_per_step;
    h->lsd_ready = true;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_lsd_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_llr, const uint8_t* d_hard,
                         int64_t B, uint8_t* d_solution, int32_t* d_stats, void* stream)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", (long long)B);
    if (!h->lsd_ready) return fail(QBP_E_INVALID, "qbp_lsd_batch without qbp_lsd_configure");
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_llr || !d_hard || !d_solution) return fail(QBP_E_INVALID, "null pointer");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    qbp::LsdParams P{};
    P.count = B; P.syndromes = d_syndromes; P.llr = d_llr; P.hard = d_hard; P.solution = d_solution; P.stats = d_stats;
    return lsd_launch(h, P, B, false, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_lsd_batch(qbp_handle* h, const uint8_t* syndromes, const double* llr, const uint8_t* hard, int64_t B,
                  uint8_t* solution, int32_t* stats)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (B < 0) return fail(QBP_E_INVALID, "B must be >= 0 (got %lld)", (long long)B);
    if (!h->lsd_ready) return fail(QBP_E_INVALID, "qbp_lsd_batch without qbp_lsd_configure");
    if (B == 0) return QBP_OK;
    if (!syndromes || !llr || !hard || !solution) return fail(QBP_E_INVALID, "null pointer");
    const int rc = lsd_build(h);        // (QBP_OPT_LSD_MEM may have changed since qbp_lsd_configure: before any copy)
    if (rc) return rc;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t m = h->m, n = h->n, b = (size_t)B;
    HostStage st(h->stream);
    const uint8_t* d_syn = st.in(h->d_syn, syndromes, b * m);
    const double* d_llr = st.in(h->d_llr, llr, b * n);
    const uint8_t* d_hard = st.in(h->d_hard, hard, b * n);
    uint8_t* d_sol = st.out(h->d_sol, solution, b * n);
    int32_t* d_stats = st.out(h->d_lsd_stats, stats, b * 4);
    if (st.failed()) return st.error();
    return st.finish(qbp_lsd_batch_device(h, d_syn, d_llr, d_hard, B, d_sol, d_stats, h->stream));
}
QBP_ABI_CATCH

// ---- Distance upper bound (qbp_distance.hpp) ------------------------------------------------------------------------
// rows [count][n] 0/1 bytes -> [count][W] words, bit v & 31 of word v >> 5
static std::vector<uint32_t> dist_pack_rows(const uint8_t* rows, size_t count, size_t n, size_t W)
{
    std::vector<uint32_t> bits(count * W, 0u);
    for (size_t i = 0; i < count; ++i)
        for (size_t v = 0; v < n; ++v)
            if (rows[i * n + v] & 1u) bits[i * W + (v >> 5)] |= 1u << (v & 31);
    return bits;
}

int qbp_distance_search(qbp_handle* h, const uint8_t* G, int32_t r, const uint8_t* L, int32_t k, uint64_t seed,
                        int64_t trial_begin, int64_t trial_end, int64_t result[4], int64_t* hist, uint8_t* codeword,
                        uint64_t* logical_mask)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (!G || !L || !result || !hist) return fail(QBP_E_INVALID, "null pointer");
    if (r < 1) return fail(QBP_E_INVALID, "r = %d (need >= 1)", r);
    if (k < 1 || k > 64) return fail(QBP_E_INVALID, "k must be in 1..64 (got %d)", k);
    if (trial_end < trial_begin)
        return fail(QBP_E_INVALID, "trial_end %lld < trial_begin %lld", (long long)trial_end, (long long)trial_begin);
    const unsigned long long total = (unsigned long long)trial_end - (unsigned long long)trial_begin;
    if (total > (1ull << qbp::DIST_TRIAL_BITS))
        return fail(QBP_E_INVALID, "%llu trials in one call (at most 2^%d)", total, qbp::DIST_TRIAL_BITS);
    const size_t n = (size_t)h->n;
    const int W = (h->n + 31) / 32;
    int NP = 4;
    while (NP < h->n) NP <<= 1;
    const size_t lds = (qbp::dist_lds_bytes(r, W, NP) + 15) & ~(size_t)15;
    if (r > qbp::DIST_MAX_ROWS || h->n > qbp::DIST_MAX_COLS || lds > (size_t)160 * 1024)
        return fail(QBP_E_UNSUPPORTED, "the distance search keeps the bit-packed rows of G and its sort keys in LDS: %d x %d "
                                       "needs %zu B (limits: 160 KiB, %d rows, %d columns)",
                    r, h->n, lds, qbp::DIST_MAX_ROWS, qbp::DIST_MAX_COLS);
    // H g = 0 for every row g of G: what makes the weight found an upper bound
    for (int i = 0; i < r; ++i) {
        const uint8_t* g = G + (size_t)i * n;
        for (int c = 0; c < h->m; ++c) {
            unsigned par = 0;
            for (int e = h->row_ptr[c]; e < h->row_ptr[c + 1]; ++e) par ^= g[h->col_idx[e]] & 1u;
            if (par) return fail(QBP_E_INVALID, "row %d of G is not in ker H (check %d)", i, c);
        }
    }
    if (total == 0) {
        result[0] = 0; result[1] = result[2] = result[3] = -1;
        return QBP_OK;
    }
    const std::vector<uint32_t> gbits = dist_pack_rows(G, (size_t)r, n, (size_t)W);
    const std::vector<uint32_t> lbits = dist_pack_rows(L, (size_t)k, n, (size_t)W);
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    hipStream_t s = h->stream;
    HostStage st(s);
    qbp::DistParams P{};
    P.r = r; P.n = h->n; P.W = W; P.NP = NP; P.k = k;
    P.gbits = st.in(h->d_dist_gbits, gbits.data(), gbits.size());
    P.lbits = st.in(h->d_dist_lbits, lbits.data(), lbits.size());
    P.seed = seed; P.trial_begin = trial_begin; P.count = (long long)total;
    // d_dist_out: hist [n + 1] | best | found [2] | logical mask
    long long* d_out = st.zeroed(h->d_dist_out, n + 5);
    if (st.failed()) return st.error();
    HIP_TRY(h->d_dist_codeword.reserve(n));
    P.hist = reinterpret_cast<unsigned long long*>(d_out);
    P.best = P.hist + n + 1;
    P.found = d_out + n + 2;
    P.codeword = h->d_dist_codeword.p;
    P.logical_mask = P.hist + n + 4;
    HIP_TRY(hipMemsetAsync(P.best, 0xff, sizeof(unsigned long long), s));
    // one wavefront per workgroup: as many per CU as the LDS holds, up to osd0_kernel's 32; QBP_OPT_BLOCKS_PER_CU overrides
    long long per_cu = std::max<long long>(1, std::min<long long>(32, (long long)(((size_t)160 * 1024) / lds)));
    if (h->opt_blocks_per_cu > 0) per_cu = h->opt_blocks_per_cu;
    const long long grid = std::max<long long>(1, std::min<long long>((long long)total, (long long)h->num_cu * per_cu));
    h->last_threads = 64; h->last_lds = (int)lds; h->last_grid = (int)grid;
    HIP_TRY(qbp::launch_dist_search(false, P, (unsigned)grid, lds, s));
    unsigned long long best = ~0ull;
    HIP_TRY(hipMemcpyAsync(&best, P.best, sizeof(best), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    long long found[2] = {-1, -1};
    unsigned long long lm = 0;
    std::vector<uint8_t> row;
    if (best != ~0ull) {
        // the best trial once more, by one wavefront that stores its row: nothing races for codeword and logical_mask
        P.trial_begin = trial_begin + (long long)(best & ((1ull << qbp::DIST_TRIAL_BITS) - 1ull));
        P.count = 1;
        HIP_TRY(qbp::launch_dist_search(true, P, 1u, lds, s));
        row.resize(n);
        HIP_TRY(hipMemcpyAsync(found, P.found, sizeof(found), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&lm, P.logical_mask, sizeof(lm), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(row.data(), P.codeword, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (found[0] != (long long)(best >> qbp::DIST_TRIAL_BITS))
            return fail(QBP_E_HIP, "the repeated trial %lld gave weight %lld, the search %llu", P.trial_begin, found[0],
                        best >> qbp::DIST_TRIAL_BITS);
    }
    st.add(hist, d_out, n + 1);
    const int rc = st.finish(QBP_OK);
    if (rc) return rc;
    result[0] = (int64_t)total;
    result[1] = result[2] = result[3] = -1;
    if (best != ~0ull) {
        result[1] = found[0]; result[2] = P.trial_begin; result[3] = found[1];
        if (codeword) std::memcpy(codeword, row.data(), n);
        if (logical_mask) *logical_mask = lm;
    }
    return QBP_OK;
}
QBP_ABI_CATCH

// ---- Pauli-frame simulation of CSS circuits (include/qbp.h: qbp_frame_*; qbp_frame.hpp) ----------------------------
struct qbp_frame {
    int device = 0, nq = 0, m = 0, k = 0, n_classes = 0;
    long long n_ops = 0, n_sites = 0, n_faults = 0, n_rec = 0;
    DevBuf<int4> d_ops;
    DevBuf<uint32_t> d_site_info;
    DevBuf<long long> d_site_base;
    DevBuf<int32_t> d_det_ptr, d_det_idx, d_obs_ptr, d_obs_idx;
    DevBuf<uint32_t> d_work;                 // frame [2 nq][W] | rec [n_rec][W] of one chunk
    DevBuf<uint8_t> d_out_det;               // host entries
    DevBuf<unsigned long long> d_out_obs;
    hipStream_t stream = nullptr;
    int num_cu = 1;
    long long opt_chunk_lanes = 0, last_chunks = 0;
};

void qbp_frame_destroy(qbp_frame* f)
try {
    if (!f) return;
    DeviceScope on_device(f->device);
    if (f->stream) { (void)hipStreamSynchronize(f->stream); (void)hipStreamDestroy(f->stream); }
    delete f;
}
catch (...) {
}

// a CSR list of measurement-record indices: `what` names it in the message
static int frame_check_csr(const int32_t* ptr, const int32_t* idx, int32_t rows, long long n_rec, const char* what)
{
    if (rows == 0) return QBP_OK;
    if (!ptr) return fail(QBP_E_INVALID, "null %s pointer array", what);
    if (ptr[0] != 0) return fail(QBP_E_INVALID, "%s_ptr[0] = %d (need 0)", what, ptr[0]);
    for (int32_t c = 0; c < rows; ++c)
        if (ptr[c + 1] < ptr[c]) return fail(QBP_E_INVALID, "%s_ptr decreases at %d", what, c);
    if (ptr[rows] > 0 && !idx) return fail(QBP_E_INVALID, "null %s index array", what);
    for (int32_t e = 0; e < ptr[rows]; ++e)
        if (idx[e] < 0 || idx[e] >= n_rec)
            return fail(QBP_E_INVALID, "%s_idx[%d] = %d is outside the %lld measurement records", what, e, idx[e], n_rec);
    return QBP_OK;
}

int qbp_frame_create(int32_t nq, const int32_t* ops, int64_t n_ops, const int32_t* det_ptr, const int32_t* det_idx,
                     int32_t m, const int32_t* obs_ptr, const int32_t* obs_idx, int32_t k, int32_t device,
                     qbp_frame** out)
try {
    if (!out) return fail(QBP_E_INVALID, "out is null");
    *out = nullptr;
    if (nq < 1) return fail(QBP_E_INVALID, "nq = %d (need >= 1)", nq);
    if (n_ops < 0 || (n_ops > 0 && !ops)) return fail(QBP_E_INVALID, "null op table or n_ops < 0");
    if (m < 0) return fail(QBP_E_INVALID, "m = %d (need >= 0)", m);
    if (k < 0 || k > 64) return fail(QBP_E_INVALID, "k must be in 0..64 (got %d)", k);
    std::vector<int4> rows((size_t)n_ops);
    std::vector<uint32_t> site_info;
    std::vector<long long> site_base;
    long long n_rec = 0, n_faults = 0;
    int n_classes = 0;
    for (int64_t i = 0; i < n_ops; ++i) {
        const int32_t kind = ops[4 * i], q0 = ops[4 * i + 1], q1 = ops[4 * i + 2], cls = ops[4 * i + 3];
        if (kind < QBP_FRAME_RZ || kind > QBP_FRAME_DEP2) return fail(QBP_E_INVALID, "op %lld: kind %d", (long long)i, kind);
        const bool pair = kind == QBP_FRAME_CX || kind == QBP_FRAME_DEP2;
        if (q0 < 0 || q0 >= nq || (pair && (q1 < 0 || q1 >= nq)))
            return fail(QBP_E_INVALID, "op %lld: a qubit outside [0, %d)", (long long)i, nq);
        if (pair && q0 == q1) return fail(QBP_E_INVALID, "op %lld: a pair of equal qubits (%d)", (long long)i, q0);
        int4 r{kind, q0, pair ? q1 : 0, 0};
        if (kind == QBP_FRAME_MZ || kind == QBP_FRAME_MX) {
            if (n_rec >= 2147483647ll) return fail(QBP_E_UNSUPPORTED, "more than 2^31 - 1 measurements");
            r.w = (int)n_rec++;
        } else if (kind >= QBP_FRAME_XERR) {
            if (cls < 0 || cls >= QBP_FRAME_MAX_CLASSES)
                return fail(QBP_E_INVALID, "op %lld: rate class %d outside [0, %d)", (long long)i, cls, QBP_FRAME_MAX_CLASSES);
            if (site_info.size() >= 4294967292ull) return fail(QBP_E_UNSUPPORTED, "more than 2^32 - 4 sites");
            const uint32_t K = kind == QBP_FRAME_DEP1 ? 3u : kind == QBP_FRAME_DEP2 ? 15u : 1u;
            const uint32_t fixed = kind == QBP_FRAME_XERR ? 1u : kind == QBP_FRAME_ZERR ? 2u : 0u;
            r.w = (int)(uint32_t)site_info.size();
            site_info.push_back(K | fixed << 4 | (uint32_t)cls << 8);
            site_base.push_back(n_faults);
            n_faults += K;
            n_classes = std::max(n_classes, cls + 1);
        }
        rows[(size_t)i] = r;
    }
    int rc = frame_check_csr(det_ptr, det_idx, m, n_rec, "det");
    if (rc) return rc;
    if ((rc = frame_check_csr(obs_ptr, obs_idx, k, n_rec, "obs")) != QBP_OK) return rc;
    struct Guard {
        qbp_frame* f;
        ~Guard() { if (f) qbp_frame_destroy(f); }
    } guard{new qbp_frame()};
    qbp_frame* f = guard.f;
    f->device = device; f->nq = nq; f->m = m; f->k = k; f->n_classes = n_classes;
    f->n_ops = n_ops; f->n_sites = (long long)site_info.size(); f->n_faults = n_faults; f->n_rec = n_rec;
    site_info.resize((site_info.size() + 3) / 4 * 4 + 4, 0u);      // the sampler reads whole groups of four
    site_base.push_back(n_faults);
    DeviceScope on_device(device);
    HIP_TRY(on_device.err);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    f->num_cu = std::max(1, prop.multiProcessorCount);
    HIP_TRY(f->d_ops.upload(rows));
    HIP_TRY(f->d_site_info.upload(site_info));
    HIP_TRY(f->d_site_base.upload(site_base));
    HIP_TRY(f->d_det_ptr.upload(m ? std::vector<int32_t>(det_ptr, det_ptr + m + 1) : std::vector<int32_t>(1, 0)));
    HIP_TRY(f->d_det_idx.upload(m ? std::vector<int32_t>(det_idx, det_idx + det_ptr[m]) : std::vector<int32_t>()));
    HIP_TRY(f->d_obs_ptr.upload(k ? std::vector<int32_t>(obs_ptr, obs_ptr + k + 1) : std::vector<int32_t>(1, 0)));
    HIP_TRY(f->d_obs_idx.upload(k ? std::vector<int32_t>(obs_idx, obs_idx + obs_ptr[k]) : std::vector<int32_t>()));
    HIP_TRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    guard.f = nullptr;
    *out = f;
    return QBP_OK;
}
QBP_ABI_CATCH

// lanes of 32 records a chunk holds at the most: QBP_FRAME_OPT_CHUNK_LANES, else what 256 MiB of workspace hold
static long long frame_chunk_lanes(const qbp_frame* f)
{
    const long long words = 2ll * f->nq + f->n_rec;
    long long lanes = f->opt_chunk_lanes > 0 ? f->opt_chunk_lanes : ((256ll << 20) / 4) / words;
    lanes = std::min<long long>(lanes, 1ll << 20);
    return std::max<long long>(64, (lanes + 63) / 64 * 64);
}

// Everything a frame call refuses, host only; sample: the thresholds of the rates
static int frame_check_call(qbp_frame* f, bool sample, const double* rates, int32_t n_rates, int64_t begin, int64_t T,
                            unsigned thr[QBP_FRAME_MAX_CLASSES])
{
    if (!f) return fail(QBP_E_INVALID, "null frame simulator");
    if (T < 0) return fail(QBP_E_INVALID, "T = %lld (need >= 0)", (long long)T);
    if (begin < 0 || begin > INT64_MAX - T) return fail(QBP_E_INVALID, "a record range outside [0, 2^63)");
    if (!sample) {
        if (begin + T > f->n_faults)
            return fail(QBP_E_INVALID, "faults [%lld, %lld) of %lld", (long long)begin, (long long)(begin + T), f->n_faults);
        return QBP_OK;
    }
    if (!rates || n_rates < 0) return fail(QBP_E_INVALID, "null rates");
    if (f->n_classes > n_rates)
        return fail(QBP_E_INVALID, "the circuit has rate class %d, the call %d rates", f->n_classes - 1, n_rates);
    for (int c = 0; c < QBP_FRAME_MAX_CLASSES; ++c) thr[c] = 0u;
    for (int c = 0; c < n_rates; ++c) {
        if (!(rates[c] >= 0.0 && rates[c] < 1.0)) return fail(QBP_E_INVALID, "rates[%d] = %g is not in [0, 1)", c, rates[c]);
        if (c < QBP_FRAME_MAX_CLASSES) thr[c] = mc_threshold(rates[c]);
    }
    return QBP_OK;
}

// The chunks of one call, enqueued on s: per chunk frame_sim_kernel, then frame_assemble_kernel.
static int frame_run(qbp_frame* f, bool sample, const unsigned* thr, uint64_t seed, int64_t begin, int64_t T,
                     uint8_t* d_det_bits, uint64_t* d_obs, hipStream_t s)
{
    if (T == 0 || (!d_det_bits && !d_obs)) return QBP_OK;
    DeviceScope on_device(f->device);
    HIP_TRY(on_device.err);
    const long long lanes_all = (T + 31) / 32, cap = frame_chunk_lanes(f);
    const long long W = std::min<long long>(cap, (lanes_all + 63) / 64 * 64);
    const long long words = 2ll * f->nq + f->n_rec;
    HIP_TRY(f->d_work.reserve((size_t)(words * W)));
    const long long rb = (f->m + 7) / 8;
    qbp::FrameParams P{};
    P.ops = f->d_ops.p; P.n_ops = f->n_ops; P.site_info = f->d_site_info.p; P.site_base = f->d_site_base.p;
    P.nq = f->nq; P.n_rec = (int)f->n_rec; P.W = W;
    P.frame = f->d_work.p; P.rec = f->d_work.p + 2ll * f->nq * W;
    P.seed = seed;
    if (sample) std::copy(thr, thr + QBP_FRAME_MAX_CLASSES, P.thr);
    P.det_ptr = f->d_det_ptr.p; P.det_idx = f->d_det_idx.p; P.m = f->m;
    P.obs_ptr = f->d_obs_ptr.p; P.obs_idx = f->d_obs_idx.p; P.k = f->k;
    f->last_chunks = 0;
    for (long long a = 0; a < T; a += 32 * W) {
        const long long t = std::min<long long>(32 * W, T - a);
        P.begin = (unsigned long long)begin + (unsigned long long)a;
        P.T = t;
        P.det_bits = d_det_bits && rb ? d_det_bits + a * rb : nullptr;
        P.obs = d_obs ? reinterpret_cast<unsigned long long*>(d_obs) + a : nullptr;
        HIP_TRY(qbp::launch_frame_sim(sample, P, s));
        const long long items = (P.det_bits ? t * rb : 0) + (P.obs ? t : 0);
        const long long grid = std::min<long long>((items + qbp::FRAME_THREADS - 1) / qbp::FRAME_THREADS, 16ll * f->num_cu);
        if (grid > 0) HIP_TRY(qbp::launch_frame_assemble(P, (unsigned)grid, s));
        ++f->last_chunks;
    }
    return QBP_OK;
}

static int frame_host(qbp_frame* f, bool sample, const unsigned* thr, uint64_t seed, int64_t begin, int64_t T,
                      uint8_t* det_bits, uint64_t* obs)
{
    if (T == 0) return QBP_OK;
    DeviceScope on_device(f->device);
    HIP_TRY(on_device.err);
    HostStage st(f->stream);
    const size_t rb = (size_t)(f->m + 7) / 8;
    uint8_t* d_det = rb ? st.out(f->d_out_det, det_bits, (size_t)T * rb) : nullptr;
    unsigned long long* d_obs = st.out(f->d_out_obs, reinterpret_cast<unsigned long long*>(obs), (size_t)T);
    if (st.failed()) return st.error();
    return st.finish(frame_run(f, sample, thr, seed, begin, T, d_det, reinterpret_cast<uint64_t*>(d_obs), f->stream));
}

int qbp_frame_sample_device(qbp_frame* f, const double* rates, int32_t n_rates, uint64_t seed, int64_t shot_begin,
                            int64_t T, uint8_t* d_det_bits, uint64_t* d_obs, void* stream)
try {
    unsigned thr[QBP_FRAME_MAX_CLASSES];
    const int rc = frame_check_call(f, true, rates, n_rates, shot_begin, T, thr);
    if (rc) return rc;
    return frame_run(f, true, thr, seed, shot_begin, T, d_det_bits, d_obs, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_frame_sample(qbp_frame* f, const double* rates, int32_t n_rates, uint64_t seed, int64_t shot_begin, int64_t T,
                     uint8_t* det_bits, uint64_t* obs)
try {
    unsigned thr[QBP_FRAME_MAX_CLASSES];
    const int rc = frame_check_call(f, true, rates, n_rates, shot_begin, T, thr);
    if (rc) return rc;
    return frame_host(f, true, thr, seed, shot_begin, T, det_bits, obs);
}
QBP_ABI_CATCH

int qbp_frame_faults_device(qbp_frame* f, int64_t fault_begin, int64_t T, uint8_t* d_det_bits, uint64_t* d_obs,
                            void* stream)
try {
    const int rc = frame_check_call(f, false, nullptr, 0, fault_begin, T, nullptr);
    if (rc) return rc;
    return frame_run(f, false, nullptr, 0, fault_begin, T, d_det_bits, d_obs, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_frame_faults(qbp_frame* f, int64_t fault_begin, int64_t T, uint8_t* det_bits, uint64_t* obs)
try {
    const int rc = frame_check_call(f, false, nullptr, 0, fault_begin, T, nullptr);
    if (rc) return rc;
    return frame_host(f, false, nullptr, 0, fault_begin, T, det_bits, obs);
}
QBP_ABI_CATCH

int qbp_frame_set_option(qbp_frame* f, int32_t option, int64_t value)
try {
    if (!f) return fail(QBP_E_INVALID, "null frame simulator");
    if (option != QBP_FRAME_OPT_CHUNK_LANES) return fail(QBP_E_INVALID, "unknown frame option %d", option);
    if (value < 0) return fail(QBP_E_INVALID, "QBP_FRAME_OPT_CHUNK_LANES = %lld (need >= 0)", (long long)value);
    f->opt_chunk_lanes = value;
    return QBP_OK;
}
QBP_ABI_CATCH

int64_t qbp_frame_get_info(qbp_frame* f, int32_t what)
try {
    if (!f) return -1;
    switch (what) {
    case QBP_FRAME_INFO_QUBITS: return f->nq;
    case QBP_FRAME_INFO_SITES: return f->n_sites;
    case QBP_FRAME_INFO_FAULTS: return f->n_faults;
    case QBP_FRAME_INFO_RECORDS: return f->n_rec;
    case QBP_FRAME_INFO_DETECTORS: return f->m;
    case QBP_FRAME_INFO_OBSERVABLES: return f->k;
    case QBP_FRAME_INFO_CHUNK_LANES: return frame_chunk_lanes(f);
    case QBP_FRAME_INFO_WORKSPACE_BYTES: return (int64_t)(f->d_work.cap * sizeof(uint32_t));
    case QBP_FRAME_INFO_CHUNKS: return f->last_chunks;
    case QBP_FRAME_INFO_CLASSES: return f->n_classes;
    default: return -1;
    }
}
catch (...) { return -1; }

// ---- Monte-Carlo (include/qbp.h: qbp_mc_run*) --------------------------------------------------------------------

// Where the errors of a Monte-Carlo call come from; only the fields of `kind` are read.
struct McErrors {
    enum Kind { P, PROBS, WEIGHT, STORED, ENUM, FAULT } kind = P;
    int32_t draws = 1;                       // P, PROBS
    uint64_t seed = 0;                       // all but STORED and ENUM
    double p = 0.0;                          // P: every column fails with p
    const double* probs = nullptr;           // PROBS: a probability per column, host [n]
    int32_t weight = 0;                      // WEIGHT: exactly this many ones, uniform among the patterns
                                             // ENUM: the patterns of this weight by rank (the trial index is the rank)
                                             // FAULT: exactly this many firing sites of the handle's fault table
    const uint8_t* d_errors = nullptr;       // STORED: device [trials, n]; the trial range starts at 0
};

struct McDecoder {
    int32_t max_iter = 0;                    // (McCall::LADDER: the last budget instead)
    int32_t variant = 0;
    double alpha = 1.0, damping = 1.0, clip_llr = 0.0;
    uint32_t flags = 0;
};

// One Monte-Carlo call, whichever entry it came through (device pointers but Lx, errors.probs and budgets).
struct McCall {
    McErrors errors;
    int64_t trial_begin = 0, trial_end = 0;
    const uint8_t* Lx = nullptr;             // host [k, n]
    int32_t k = 0, distance = 0;
    McDecoder dec;
    const double* d_prior = nullptr;
    // the outputs, all added to
    // qbp_mc_run_budgets*: LADDER, qbp_mc_run*_spectrum*: SPECTRUM, qbp_mc_run*_llr_hist*: LLRHIST (a ladder too)
    enum Out { COUNTERS, LADDER, SPECTRUM, LLRHIST } out = COUNTERS;
    int64_t* d_counters = nullptr;           // [rows()][QBP_NUM_COUNTERS]
    const int32_t* budgets = nullptr;        // ladder(): host [n_budgets], a counter row each
    int32_t n_budgets = 0;
    int64_t* d_llr_hist = nullptr;           // LLRHIST: [n_budgets][QBP_LLR_HIST_ROWS][llr_bins + 3]
    double llr_lo = 0.0, llr_hi = 0.0;       // LLRHIST: the range of the bins
    int32_t llr_bins = 0;
    int64_t* d_spectrum = nullptr;           // SPECTRUM: [QBP_SPECTRUM_ROWS][n + 1]
    int64_t* d_iter_hist = nullptr;          // SPECTRUM: [max_iter + 1], may be null

    int64_t trials() const { return trial_end - trial_begin; }
    bool ladder() const { return out == LADDER || out == LLRHIST; }
    size_t rows() const { return ladder() ? (size_t)n_budgets : 1; }          // counter rows = failure-record planes
    int32_t last_iter() const { return ladder() ? budgets[n_budgets - 1] : dec.max_iter; }
    size_t llr_cells() const { return out == LLRHIST ? (size_t)QBP_LLR_HIST_WORDS(n_budgets, llr_bins) : 0; }
    // fixed weight, of columns (sampled or enumerated) or of fault sites: filled chunk by chunk
    bool fixed_weight() const
    {
        return errors.kind == McErrors::WEIGHT || errors.kind == McErrors::ENUM || errors.kind == McErrors::FAULT;
    }
    // trials that no BP kernel draws itself: fixed weight, and the layered and fixed-point kernels, which decode stored
    // errors only
    bool chunked() const
    {
        return fixed_weight() ||
               (errors.kind != McErrors::STORED && (dec.flags & (QBP_FLAG_LAYERED | QBP_FLAG_QUANT)));
    }
};

// Trials sampled into the handle's buffer and decoded per chunk of a chunked() call of T trials
static long long mc_chunk_trials(const qbp_handle* h, int64_t T)
{
    const long long dflt = std::max<long long>(1, std::min<long long>(1 << 20, ((long long)1 << 28) / (long long)h->n));
    return std::min<long long>(h->opt_weight_chunk > 0 ? h->opt_weight_chunk : dflt, T);
}

// C(n, w), or false above 2^62 (qbp_enum_count)
static bool enum_count(int n, int w, int64_t* count)
{
    const int k = std::min(w, n - w);
    unsigned __int128 c = 1;
    for (int i = 0; i < k; ++i) {
        c = c * (unsigned)(n - i) / (unsigned)(i + 1);          // C(n, i + 1): exact at every step
        if (c > ((unsigned __int128)1 << 62)) return false;
    }
    *count = (int64_t)c;
    return true;
}

// The rank range of an enumeration: weight in [0, n], C(n, weight) <= 2^62, 0 <= rank_begin <= rank_end <= C(n, weight)
static int check_enum_range(const qbp_handle* h, int32_t weight, int64_t rank_begin, int64_t rank_end)
{
    if (weight < 0 || weight > h->n)
        return fail(QBP_E_INVALID, "weight = %d out of [0, %d] (n columns)", weight, h->n);
    int64_t count = 0;
    if (!enum_count(h->n, weight, &count))
        return fail(QBP_E_INVALID, "C(%d, %d) patterns are beyond 2^62", h->n, weight);
    if (rank_begin < 0 || rank_end < rank_begin || rank_end > count)
        return fail(QBP_E_INVALID, "ranks [%lld, %lld) out of [0, C(%d, %d) = %lld]", (long long)rank_begin,
                    (long long)rank_end, h->n, weight, (long long)count);
    return QBP_OK;
}

// The table mc_enum_weight_kernel searches, on the device: C(j, t) at t * (n + 1) + j for t <= w, j <= n, saturated at
// 2^63 - 1.  Cached per weight (n is the handle's); uploaded as the tables of McInputs are.
static int enum_prepare(qbp_handle* h, int32_t w, hipStream_t s)
{
    if (h->binom_w == w) return QBP_OK;
    const size_t stride = (size_t)h->n + 1;
    const unsigned long long sat = 0x7fffffffffffffffull;
    std::vector<unsigned long long> tab(((size_t)w + 1) * stride, 0ull);
    for (size_t j = 0; j < stride; ++j) tab[j] = 1ull;                       // C(j, 0)
    for (size_t t = 1; t <= (size_t)w; ++t)
        for (size_t j = 1; j < stride; ++j) {                                // C(0, t) = 0
            const unsigned long long a = tab[t * stride + j - 1], b = tab[(t - 1) * stride + j - 1];
            tab[t * stride + j] = a > sat - b ? sat : a + b;
        }
    h->binom_w = -1;
    HIP_TRY(h->d_binom.reserve(tab.size()));
    HIP_TRY(hipMemcpyAsync(h->d_binom.p, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->binom_w = w;
    return QBP_OK;
}

// `trial_end`: the end of the range (an enumeration's ranks have an upper bound; no sampler's trials do)
static int check_mc_errors(const qbp_handle* h, const McErrors& e, int64_t trial_begin, int64_t trial_end)
{
    if (e.kind == McErrors::STORED) return e.d_errors ? QBP_OK : fail(QBP_E_INVALID, "null pointer");
    if (e.kind == McErrors::ENUM) return check_enum_range(h, e.weight, trial_begin, trial_end);
    if (e.kind == McErrors::WEIGHT) {
        if (e.weight < 0 || e.weight > h->n)
            return fail(QBP_E_INVALID, "weight = %d out of [0, %d] (n columns)", e.weight, h->n);
    } else if (e.kind == McErrors::FAULT) {
        if (h->fault_sites == 0) return fail(QBP_E_INVALID, "no fault table: call qbp_fault_table_set first");
        const long long top = std::min<long long>(h->fault_sites, QBP_FAULT_WEIGHT_MAX);
        if (e.weight < 0 || e.weight > top)
            return fail(QBP_E_INVALID, "weight = %d out of [0, %lld] (min of %lld fault sites and QBP_FAULT_WEIGHT_MAX)",
                        e.weight, top, h->fault_sites);
    } else {
        if (e.draws != 1 && e.draws != 2) return fail(QBP_E_INVALID, "draws must be 1 or 2 (got %d)", e.draws);
        if (e.kind == McErrors::P && !(e.p >= 0.0 && e.p <= 1.0)) return fail(QBP_E_INVALID, "p = %g out of [0, 1]", e.p);
        const int rc = e.kind == McErrors::PROBS ? check_probs(h, e.probs) : QBP_OK;
        if (rc) return rc;
    }
    if (trial_begin < 0) return fail(QBP_E_INVALID, "trial_begin must be >= 0");
    return QBP_OK;
}

// second stages that are no OSD: never a BP launch's bit
constexpr uint32_t SECOND_BP_BITS = QBP_FLAG_RELAY | QBP_FLAG_GD | QBP_FLAG_LSD;

// Everything a Monte-Carlo call refuses: host only, once per public call, for the whole range and before any GPU work.
// `host_prior`: the priors when they are a host array (no NaN; finite for the layered schedule), else null.
static int check_mc_call(qbp_handle* h, const McCall& c, const double* host_prior)
{
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (!c.d_prior || !c.d_counters) return fail(QBP_E_INVALID, "null pointer");
    int rc = QBP_OK;
    if (c.out == McCall::SPECTRUM) {
        if (!c.d_spectrum) return fail(QBP_E_INVALID, "spectrum is null");
        if (c.dec.max_iter > QBP_MC_SPECTRUM_MAX_ITER)
            return fail(QBP_E_INVALID, "max_iter = %d beyond QBP_MC_SPECTRUM_MAX_ITER = %d", c.dec.max_iter,
                        QBP_MC_SPECTRUM_MAX_ITER);
    }
    if (c.out == McCall::LLRHIST) {
        if (!c.d_llr_hist) return fail(QBP_E_INVALID, "hist is null");
        if (c.llr_bins < 1) return fail(QBP_E_INVALID, "bins = %d must be >= 1", c.llr_bins);
        if (!std::isfinite(c.llr_lo) || !std::isfinite(c.llr_hi) || !(c.llr_lo < c.llr_hi))
            return fail(QBP_E_INVALID, "the LLR range [%g, %g] must be finite with llr_lo < llr_hi", c.llr_lo, c.llr_hi);
    }
    if (c.ladder() && (rc = check_budgets(c.budgets, c.n_budgets)) != QBP_OK) return rc;
    if (c.out == McCall::LLRHIST && QBP_LLR_HIST_WORDS(c.n_budgets, c.llr_bins) > QBP_LLR_HIST_MAX_WORDS)
        return fail(QBP_E_INVALID, "%d budgets x %d rows x (%d bins + 3) = %lld words beyond QBP_LLR_HIST_MAX_WORDS = %d",
                    c.n_budgets, QBP_LLR_HIST_ROWS, c.llr_bins, (long long)QBP_LLR_HIST_WORDS(c.n_budgets, c.llr_bins),
                    QBP_LLR_HIST_MAX_WORDS);
    if ((rc = check_mc_errors(h, c.errors, c.trial_begin, c.trial_end)) != QBP_OK) return rc;
    if ((rc = check_decode_args(h, c.trials(), c.last_iter(), c.dec.variant)) != QBP_OK) return rc;
    // ladders and spectra have neither a Relay or guided-decimation stage nor a layered build
    if ((rc = check_relay_flags(h, c.dec.flags, c.out != McCall::COUNTERS)) != QBP_OK) return rc;
    if ((rc = check_gd_flags(h, c.dec.flags, c.out != McCall::COUNTERS)) != QBP_OK) return rc;
    if ((rc = check_lsd_flags(h, c.dec.flags, c.out != McCall::COUNTERS)) != QBP_OK) return rc;
    if ((rc = check_layered_flags(h, c.dec.flags, c.dec.variant, c.out != McCall::COUNTERS)) != QBP_OK) return rc;
    if ((rc = check_quant_flags(h, c.dec.flags, c.dec.variant, c.out != McCall::COUNTERS)) != QBP_OK) return rc;
    if (host_prior && (rc = check_prior(h->n, host_prior, (c.dec.flags & QBP_FLAG_LAYERED) != 0)) != QBP_OK) return rc;
    int osd_method = 0, osd_order = 0;
    if ((rc = parse_osd_flags(h, c.dec.flags & ~SECOND_BP_BITS, true, &osd_method, &osd_order)) != QBP_OK) return rc;
    if (c.k < 0 || c.k > 64) return fail(QBP_E_INVALID, "k = %d logical operators (need 0..64)", c.k);
    if (c.k > 0 && !c.Lx) return fail(QBP_E_INVALID, "Lx is null");
    if (c.dec.flags & (QBP_FLAG_OSD0 | SECOND_BP_BITS)) {
        // QBP_MC_OSD_MAX_TRIALS bounds the records of one launch.  That is the whole call -- a fixed-weight call too,
        // sampled or enumerated, although it launches chunk by chunk -- except for layered sampled calls, which have always been held to it
        // per chunk only: a longer range of those goes through.
        const bool per_chunk = c.chunked() && !c.fixed_weight();
        rc = check_mc_osd_trials(h, per_chunk ? mc_chunk_trials(h, c.trials()) : c.trials(), c.rows());
    }
    return rc;
}

// Per-trial records of the trials the BP launch leaves unconverged, read by the second kernel (OSD or Relay-BP):
// room for `t` trials in each of `rows` planes, the planes' counts zeroed, all of it named in `mc`.  `error_rows`:
// the trial's error as well (recorded shots have none).
static int mc_fail_records(qbp_handle* h, McArgs& mc, size_t rows, size_t t, bool error_rows, hipStream_t s)
{
    const size_t m = h->m, n = h->n;
    t *= rows;
    HIP_TRY(h->d_fail_count.reserve(rows));
    HIP_TRY(h->d_fail_list.reserve(t));
    HIP_TRY(h->d_fail_syn.reserve(t * m));
    HIP_TRY(h->d_fail_llr.reserve(t * n));
    HIP_TRY(h->d_fail_hard.reserve(t * n));
    if (error_rows) HIP_TRY(h->d_fail_err.reserve(t * n));
    HIP_TRY(hipMemsetAsync(h->d_fail_count.p, 0, rows * sizeof(unsigned long long), s));
    mc.fail_list = h->d_fail_list.p; mc.fail_count = h->d_fail_count.p;
    mc.fail_syn = h->d_fail_syn.p; mc.fail_llr = h->d_fail_llr.p; mc.fail_hard = h->d_fail_hard.p;
    if (error_rows) mc.fail_err = h->d_fail_err.p;
    return QBP_OK;
}

// The launches of a checked call whose BP kernel draws the errors itself, or reads stored ones: BP and
// classification, then the second stage on the trials BP left unconverged.  The Lx columns (mc_prepare) and the
// thresholds of errors.probs (mc_prepare_thr) are on the device.
static int mc_launch(qbp_handle* h, const McCall& c, hipStream_t s)
{
    const int64_t T = c.trials();
    const size_t rows = c.rows();
    const bool ladder = c.ladder(), spectrum = c.out == McCall::SPECTRUM;
    const int32_t max_iter = c.last_iter();
    // Relay-BP instead of OSD on the trials the first stage leaves unconverged: its bit goes to no BP launch
    const bool relay = (c.dec.flags & QBP_FLAG_RELAY) != 0;
    // likewise BP guided decimation
    const bool gd = (c.dec.flags & QBP_FLAG_GD) != 0;
    // and localized statistics decoding, which reads the records OSD-0 reads
    const bool lsd = (c.dec.flags & QBP_FLAG_LSD) != 0;
    // order-w OSD: its bits go to the OSD launch only, never to the decoder's launch or column-order logic
    int osd_method = 0, osd_order = 0;
    int rc = parse_osd_flags(h, c.dec.flags & ~SECOND_BP_BITS, true, &osd_method, &osd_order);
    if (rc) return rc;
    const uint32_t flags = c.dec.flags & ~(SECOND_BP_BITS | OSD_ALL_BITS);
    const bool layered = (flags & QBP_FLAG_LAYERED) != 0;
    const bool osd = (flags & QBP_FLAG_OSD0) != 0 || relay || gd || lsd;
    McArgs mc{};
    // (qbp_mc_run_budgets: a record per trial and budget)
    if (osd && (rc = mc_fail_records(h, mc, rows, (size_t)T, true, s)) != QBP_OK) return rc;
    mc.n_budgets = ladder ? c.n_budgets : 0; mc.budgets = ladder ? c.budgets : nullptr;
    mc.spectrum = reinterpret_cast<long long*>(c.d_spectrum); mc.iter_hist = reinterpret_cast<long long*>(c.d_iter_hist);
    if (c.out == McCall::LLRHIST) {
        mc.llr_hist = reinterpret_cast<long long*>(c.d_llr_hist); mc.llr_edges = h->mc_in.d_llr_edges.p; mc.llr_bins = c.llr_bins;
    }
    mc.lx_cols = h->mc_in.d_lx_cols.p; mc.trial_begin = c.trial_begin; mc.seed = c.errors.seed;
    mc.threshold = mc_threshold(c.errors.p); mc.draws = c.errors.draws; mc.half_distance = c.distance / 2;
    mc.thr_cols = c.errors.kind == McErrors::PROBS ? h->mc_in.d_thr.p : nullptr;
    mc.counters = reinterpret_cast<long long*>(c.d_counters);
    mc.errors_in = c.errors.d_errors;
    BpCall b;
    b.prior = c.d_prior; b.B = T; b.max_iter = max_iter; b.variant = c.dec.variant;
    b.alpha = c.dec.alpha; b.damping = c.dec.damping; b.clip_llr = c.dec.clip_llr; b.flags = flags;
    b.mc = &mc;
    // (a ladder's counter rows -- and the table of qbp_mc_run_llr_hist -- need LDS of their own: a matrix that fills
    // the on-chip kernel's to the last kilobyte goes to the general-H kernel)
    const bool ladder_fits = !ladder || fused_lds_bytes(h->dc, h->m, h->n, 1, h->r_stride, false, false,
                                                        2 * c.n_budgets * qbp::NUM_COUNTERS, 0, mc.llr_lds()) <= 160 * 1024;
    // (likewise the iteration histogram of qbp_mc_run_spectrum)
    const bool hist_fits = !spectrum || fused_lds_bytes(h->dc, h->m, h->n, 1, h->r_stride, false, false, qbp::NUM_COUNTERS,
                                                        max_iter + 1) <= 160 * 1024;
    if (flags & QBP_FLAG_QUANT) {
        b.flags = 0;                 // (likewise; alpha, damping and the clip of the call are not read)
        rc = quant_launch(h, b, nullptr, s);
    } else if (layered) {
        b.flags = 0;                 // (forced iterations cannot change a count: the kernel's Monte-Carlo build exits early)
        h->last_kernel = 4;
        rc = layered_launch(h, b, s);
    } else if (bp_kernel(h, T, flags, 0, true) == 2 || !ladder_fits || !hist_fits) {
        h->last_kernel = 2;
        rc = generic_launch(h, b, s);
    } else {
        rc = fused_launch(h, b, s);
        if (rc == QBP_OK) h->last_kernel = 1;
    }
    if (rc || !osd) return rc;
    if (relay || gd) {
        // second kernel: Relay-BP or BP guided decimation + classification of the trials the first stage left unconverged
        RecordCall r;
        r.prior = c.d_prior; r.max_items = T;
        r.fail_count = h->d_fail_count.p; r.fail_list = h->d_fail_list.p;
        r.fail_syn = h->d_fail_syn.p; r.fail_err = h->d_fail_err.p;
        r.half_distance = c.distance / 2; r.counters = reinterpret_cast<long long*>(c.d_counters);
        return relay ? relay_launch(h, r, true, s) : gd_launch(h, r, true, s);
    }
    if (lsd) {
        // second kernel: localized statistics decoding + classification of the same records
        qbp::LsdParams P{};
        P.count_ptr = reinterpret_cast<const long long*>(h->d_fail_count.p); P.list = h->d_fail_list.p;
        P.syndromes = h->d_fail_syn.p; P.llr = h->d_fail_llr.p; P.hard = h->d_fail_hard.p;
        P.errors = h->d_fail_err.p; P.lx_cols = h->mc_in.d_lx_cols.p; P.half_distance = c.distance / 2;
        P.counters = reinterpret_cast<long long*>(c.d_counters);
        return lsd_launch(h, P, T, true, s);
    }
    // second kernel: OSD-0 + classification of the trials BP left unconverged; their number is
    // read from device memory by the kernel itself (no host round trip)
    // (qbp_mc_run_budgets: once per row, on that row's list, records and counters)
    const size_t m = h->m, n = h->n;
    for (size_t j = 0; j < rows; ++j) {
        const size_t r0 = j * (size_t)T;                     // first record of plane j
        qbp::OsdParams O{};
        O.count_ptr = reinterpret_cast<const long long*>(h->d_fail_count.p + j);
        O.list = h->d_fail_list.p + r0;
        O.syndromes = h->d_fail_syn.p + r0 * m; O.llr = h->d_fail_llr.p + r0 * n; O.hard = h->d_fail_hard.p + r0 * n;
        O.errors = h->d_fail_err.p + r0 * n; O.lx_cols = h->mc_in.d_lx_cols.p; O.half_distance = c.distance / 2;
        O.counters = reinterpret_cast<long long*>(c.d_counters) + j * qbp::NUM_COUNTERS;
        O.spectrum = reinterpret_cast<long long*>(c.d_spectrum);
        rc = osd_launch(h, O, T, s, false, osd_method, osd_order);
        if (rc) return rc;
    }
    return QBP_OK;
}

static hipError_t mc_sample(qbp_handle* h, const McErrors& e, uint8_t* errors, long long t, int64_t trial_begin,
                            hipStream_t s)
{
    // (the samplers do not depend on H: any matrix, whichever kernel decodes it)
    if (e.kind == McErrors::WEIGHT) return qbp::launch_mc_sample_weight(errors, h->n, e.weight, t, trial_begin, e.seed, s);
    if (e.kind == McErrors::ENUM) return qbp::launch_mc_enum_weight(errors, h->n, e.weight, t, trial_begin, h->d_binom.p, s);
    if (e.kind == McErrors::FAULT) {
        // the picks of one launch: at most 2^26 words, and never fewer than a workgroup's trials
        const long long stride = std::min<long long>(t, std::max<long long>(256, ((long long)1 << 26) / std::max(e.weight, 1)));
        const hipError_t err = h->d_fault_picks.reserve((size_t)e.weight * (size_t)stride);
        if (err != hipSuccess) return err;
        return qbp::launch_mc_sample_fault_weight(errors, h->n, e.weight, t, trial_begin, e.seed, h->d_fault_first.p,
                                                  h->d_fault_k.p, h->d_fault_col.p, (unsigned)h->fault_sites,
                                                  h->d_fault_picks.p, stride, s);
    }
    if (e.kind == McErrors::PROBS)
        return qbp::launch_mc_sample_cols(errors, h->n, t, trial_begin, e.draws, e.seed, h->mc_in.d_thr.p, s);
    return qbp::launch_mc_sample(errors, h->n, t, trial_begin, e.draws, e.seed, mc_threshold(e.p), s);
}

// A checked call (check_mc_call) on the stream.
static int mc_run(qbp_handle* h, const McCall& c, hipStream_t s)
{
    if (c.trials() == 0) return QBP_OK;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    int rc = mc_prepare(h, c.Lx, c.k, s);
    if (rc) return rc;
    if (c.errors.kind == McErrors::PROBS && (rc = h->mc_in.prepare_thr((size_t)h->n, c.errors.probs, s)) != QBP_OK) return rc;
    if (c.errors.kind == McErrors::ENUM && (rc = enum_prepare(h, c.errors.weight, s)) != QBP_OK) return rc;
    if (c.out == McCall::LLRHIST) {
        if ((rc = h->mc_in.prepare_edges(c.llr_bins, c.llr_lo, c.llr_hi, s)) != QBP_OK) return rc;
        // A workgroup keeps 32-bit counts, and one launch adds at most n per trial to a cell of one workgroup -- all of
        // the launch's trials, should one workgroup decode them all: n * (trials of a launch) <= 2^32 - 1.
        const long long bound = std::max<long long>(1, 0xffffffffll / std::max(h->n, 1));
        const long long step = h->opt_llr_hist_chunk > 0 ? std::min(h->opt_llr_hist_chunk, bound) : bound;
        if (c.trials() > step) {
            const bool stored = c.errors.kind == McErrors::STORED;      // (its range starts at 0: the rows move instead)
            for (int64_t a = c.trial_begin; a < c.trial_end; a += step) {
                McCall part = c;
                const int64_t len = std::min<int64_t>(step, c.trial_end - a);
                part.trial_begin = stored ? 0 : a;
                part.trial_end = part.trial_begin + len;
                if (stored) part.errors.d_errors = c.errors.d_errors + (size_t)(a - c.trial_begin) * (size_t)h->n;
                if ((rc = mc_launch(h, part, s)) != QBP_OK) return rc;
            }
            return QBP_OK;
        }
    }
    if (!c.chunked()) return mc_launch(h, c, s);
    // the errors qbp_mc_sample_errors* returns, drawn chunk by chunk into the handle's buffer and run as stored errors:
    // the global trial index lives in the sampler only, the pipeline indexes a chunk's trials from 0
    const long long chunk = mc_chunk_trials(h, c.trials());
    HIP_TRY(h->d_weight_err.reserve((size_t)chunk * (size_t)h->n));
    McCall part = c;
    part.errors = {McErrors::STORED};
    part.errors.d_errors = h->d_weight_err.p;
    part.trial_begin = 0;
    for (int64_t a = c.trial_begin; a < c.trial_end; a += chunk) {
        part.trial_end = std::min<long long>(chunk, c.trial_end - a);
        HIP_TRY(mc_sample(h, c.errors, h->d_weight_err.p, part.trial_end, a, s));
        if ((rc = mc_launch(h, part, s)) != QBP_OK) return rc;
    }
    return QBP_OK;
}

// Every _device entry: the check, then the launches.
static int mc_run_device(qbp_handle* h, const McCall& c, void* stream)
{
    const int rc = check_mc_call(h, c, nullptr);
    return rc ? rc : mc_run(h, c, static_cast<hipStream_t>(stream));
}

// Every host-array entry: the check, the prior (and stored errors) uploaded, counters (and spectrum tables) zeroed on
// the device, the launches, and the results copied back and ADDED to the caller's arrays.  Stored-error entries SET the
// counters: the caller's are zeroed first, also when there is no pattern.  A failed run synchronises, then returns.
// `spectrum`: the first table of the call -- spectrum of a SPECTRUM call, hist of an LLRHIST call -- else null.
static int mc_run_host(qbp_handle* h, McCall c, const double* prior, const uint8_t* errors, int64_t* counters,
                       int64_t* spectrum, int64_t* iter_hist)
{
    // (the check asks of these only whether they are null: the handle's buffers take their place below)
    c.d_prior = prior; c.d_counters = counters; c.errors.d_errors = errors;
    (c.out == McCall::LLRHIST ? c.d_llr_hist : c.d_spectrum) = spectrum;
    int rc = check_mc_call(h, c, prior);
    if (rc) return rc;
    const bool stored = c.errors.kind == McErrors::STORED, tables = c.out == McCall::SPECTRUM;
    const size_t n = (size_t)h->n, T = (size_t)c.trials(), cells = c.rows() * qbp::NUM_COUNTERS;
    const size_t spec_cells = tables ? (size_t)QBP_SPECTRUM_ROWS * (n + 1) : 0, hist_cells = tables ? (size_t)c.dec.max_iter + 1 : 0;
    if (stored) std::fill(counters, counters + cells, (int64_t)0);
    if (T == 0) return QBP_OK;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    HostStage st(h->stream);
    c.d_prior = st.in(h->d_prior, prior, n);
    long long* d_cnt = st.zeroed(h->d_counters, cells);
    st.add(counters, d_cnt, cells);
    c.d_counters = reinterpret_cast<int64_t*>(d_cnt);
    if (stored) c.errors.d_errors = st.in(h->d_hard, errors, T * n);     // (scratch of the host-pointer entries)
    if (tables) {
        long long* d_tab = st.zeroed(h->d_spectrum, spec_cells + hist_cells);
        st.add(spectrum, d_tab, spec_cells);
        st.add(iter_hist, d_tab + spec_cells, hist_cells);
        c.d_spectrum = reinterpret_cast<int64_t*>(d_tab);
        c.d_iter_hist = iter_hist ? c.d_spectrum + spec_cells : nullptr;
    }
    if (c.out == McCall::LLRHIST) {
        long long* d_tab = st.zeroed(h->d_spectrum, c.llr_cells());
        st.add(spectrum, d_tab, c.llr_cells());
        c.d_llr_hist = reinterpret_cast<int64_t*>(d_tab);
    }
    if (st.failed()) return st.error();
    return st.finish(mc_run(h, c, h->stream));
}

// The four qbp_mc_sample_errors* entries: errors [T, n] of trials trial_begin .. + T, as the runs draw them.
static int mc_sample_host(qbp_handle* h, const McErrors& e, int64_t trial_begin, int64_t T, uint8_t* errors)
{
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (T < 0) return fail(QBP_E_INVALID, "T must be >= 0");
    if (!errors) return fail(QBP_E_INVALID, "errors is null");
    // (a rank beyond 2^62 is refused before this sum is looked at)
    int rc = check_mc_errors(h, e, trial_begin, trial_begin <= INT64_MAX - T ? trial_begin + T : INT64_MAX);
    if (rc) return rc;
    if (T == 0) return QBP_OK;
    if (T > ((int64_t)1 << 31)) return fail(QBP_E_INVALID, "at most 2^31 trials per call");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    hipStream_t s = h->stream;
    if (e.kind == McErrors::PROBS && (rc = h->mc_in.prepare_thr((size_t)h->n, e.probs, s)) != QBP_OK) return rc;
    if (e.kind == McErrors::ENUM && (rc = enum_prepare(h, e.weight, s)) != QBP_OK) return rc;
    HIP_TRY(h->d_hard.reserve((size_t)T * (size_t)h->n));
    HIP_TRY(mc_sample(h, e, h->d_hard.p, T, trial_begin, s));
    HIP_TRY(hipMemcpyAsync(errors, h->d_hard.p, (size_t)T * (size_t)h->n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QBP_OK;
}

// The arguments every qbp_mc_run* entry has, in the order of their parameter lists
static McCall mc_call(const uint8_t* Lx, int32_t k, int32_t distance, const McErrors& errors, int64_t trial_begin,
                      int64_t trial_end, const McDecoder& dec, const double* d_prior = nullptr,
                      int64_t* d_counters = nullptr)
{
    McCall c;
    c.Lx = Lx; c.k = k; c.distance = distance; c.errors = errors; c.trial_begin = trial_begin; c.trial_end = trial_end;
    c.dec = dec; c.d_prior = d_prior; c.d_counters = d_counters;
    return c;
}

int qbp_mc_run_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                      double p, int32_t draws, uint64_t seed, int64_t trial_begin,
                      int64_t trial_end, const double* d_prior, int32_t max_iter,
                      int32_t variant, double alpha, double damping, double clip_llr,
                      uint32_t flags, int64_t* d_counters, void* stream)
try {
    return mc_run_device(h, mc_call(Lx_host, k, distance, {McErrors::P, draws, seed, p}, trial_begin, trial_end,
                                    {max_iter, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters), stream);
}
QBP_ABI_CATCH

int qbp_mc_run(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, double p,
               int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
               const double* prior, int32_t max_iter, int32_t variant, double alpha,
               double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS])
try {
    return mc_run_host(h, mc_call(Lx, k, distance, {McErrors::P, draws, seed, p}, trial_begin, trial_end,
                                  {max_iter, variant, alpha, damping, clip_llr, flags}), prior, nullptr, counters,
                       nullptr, nullptr);
}
QBP_ABI_CATCH

// (T patterns instead of a sampler: counters SET, not added to)
int qbp_mc_run_errors(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                      int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                      double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS])
try {
    return mc_run_host(h, mc_call(Lx, k, distance, {McErrors::STORED}, 0, T,
                                  {max_iter, variant, alpha, damping, clip_llr, flags}), prior, errors, counters,
                       nullptr, nullptr);
}
QBP_ABI_CATCH

int qbp_mc_sample_errors(qbp_handle* h, double p, int32_t draws, uint64_t seed,
                         int64_t trial_begin, int64_t T, uint8_t* errors)
try {
    return mc_sample_host(h, {McErrors::P, draws, seed, p}, trial_begin, T, errors);
}
QBP_ABI_CATCH

int qbp_mc_run_weight_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance, int32_t weight,
                             uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* d_prior,
                             int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                             uint32_t flags, int64_t* d_counters, void* stream)
try {
    return mc_run_device(h, mc_call(Lx_host, k, distance, {McErrors::WEIGHT, 1, seed, 0.0, nullptr, weight}, trial_begin,
                                    trial_end, {max_iter, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters),
                         stream);
}
QBP_ABI_CATCH

int qbp_mc_run_weight(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, int32_t weight, uint64_t seed,
                      int64_t trial_begin, int64_t trial_end, const double* prior, int32_t max_iter,
                      int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                      int64_t counters[QBP_NUM_COUNTERS])
try {
    return mc_run_host(h, mc_call(Lx, k, distance, {McErrors::WEIGHT, 1, seed, 0.0, nullptr, weight}, trial_begin,
                                  trial_end, {max_iter, variant, alpha, damping, clip_llr, flags}), prior, nullptr,
                       counters, nullptr, nullptr);
}
QBP_ABI_CATCH

int qbp_mc_sample_errors_weight(qbp_handle* h, int32_t weight, uint64_t seed, int64_t trial_begin, int64_t T,
                                uint8_t* errors)
try {
    return mc_sample_host(h, {McErrors::WEIGHT, 1, seed, 0.0, nullptr, weight}, trial_begin, T, errors);
}
QBP_ABI_CATCH

int qbp_enum_count(int32_t n, int32_t weight, int64_t* count)
try {
    if (!count) return fail(QBP_E_INVALID, "count is null");
    if (n < 0 || weight < 0 || weight > n) return fail(QBP_E_INVALID, "weight = %d out of [0, %d] (n columns)", weight, n);
    int64_t c = 0;
    if (!enum_count(n, weight, &c)) return fail(QBP_E_INVALID, "C(%d, %d) patterns are beyond 2^62", n, weight);
    *count = c;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_mc_run_enum_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance, int32_t weight,
                           int64_t rank_begin, int64_t rank_end, const double* d_prior, int32_t max_iter,
                           int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                           int64_t* d_counters, void* stream)
try {
    return mc_run_device(h, mc_call(Lx_host, k, distance, {McErrors::ENUM, 1, 0, 0.0, nullptr, weight}, rank_begin,
                                    rank_end, {max_iter, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters),
                         stream);
}
QBP_ABI_CATCH

int qbp_mc_run_enum(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, int32_t weight, int64_t rank_begin,
                    int64_t rank_end, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                    double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS])
try {
    return mc_run_host(h, mc_call(Lx, k, distance, {McErrors::ENUM, 1, 0, 0.0, nullptr, weight}, rank_begin, rank_end,
                                  {max_iter, variant, alpha, damping, clip_llr, flags}), prior, nullptr, counters,
                       nullptr, nullptr);
}
QBP_ABI_CATCH

int qbp_mc_sample_errors_enum(qbp_handle* h, int32_t weight, int64_t rank_begin, int64_t T, uint8_t* errors)
try {
    return mc_sample_host(h, {McErrors::ENUM, 1, 0, 0.0, nullptr, weight}, rank_begin, T, errors);
}
QBP_ABI_CATCH

int qbp_fault_table_set(qbp_handle* h, int64_t n_sites, const int64_t* first_fault, const uint8_t* K, int64_t n_faults,
                        const int32_t* fault_column)
try {
    if (!h) return fail(QBP_E_INVALID, "null handle");
    if (n_sites < 0 || n_sites > (int64_t)0xfffffffcll)
        return fail(QBP_E_INVALID, "n_sites = %lld out of [0, 2^32 - 4]", (long long)n_sites);
    if (n_sites > 0) {
        if (!first_fault || !K || !fault_column) return fail(QBP_E_INVALID, "null pointer");
        if (n_faults < 0) return fail(QBP_E_INVALID, "n_faults must be >= 0");
        for (int64_t s = 0; s < n_sites; ++s) {
            if (K[s] != 1 && K[s] != 3 && K[s] != 15)
                return fail(QBP_E_INVALID, "K[%lld] = %d (a site has 1, 3 or 15 faults)", (long long)s, (int)K[s]);
            if (first_fault[s] < 0 || first_fault[s] > n_faults - (int64_t)K[s])
                return fail(QBP_E_INVALID, "site %lld: faults [%lld, %lld + %d) out of [0, %lld)", (long long)s,
                            (long long)first_fault[s], (long long)first_fault[s], (int)K[s], (long long)n_faults);
        }
        for (int64_t f = 0; f < n_faults; ++f)
            if (fault_column[f] < -1 || fault_column[f] >= h->n)
                return fail(QBP_E_INVALID, "fault_column[%lld] = %d out of [-1, %d)", (long long)f, fault_column[f], h->n);
    }
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    HIP_TRY(hipDeviceSynchronize());          // (a sampler that still reads the table it replaces)
    h->fault_sites = 0;
    if (n_sites == 0) return QBP_OK;
    HIP_TRY(h->d_fault_first.reserve((size_t)n_sites));
    HIP_TRY(h->d_fault_k.reserve((size_t)n_sites));
    HIP_TRY(h->d_fault_col.reserve((size_t)n_faults));
    HIP_TRY(hipMemcpy(h->d_fault_first.p, first_fault, (size_t)n_sites * sizeof(long long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_fault_k.p, K, (size_t)n_sites, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_fault_col.p, fault_column, (size_t)n_faults * sizeof(int32_t), hipMemcpyHostToDevice));
    h->fault_sites = n_sites;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_mc_run_fault_weight_device(qbp_handle* h, const uint8_t* L_host, int32_t k, int32_t distance, int32_t weight,
                                   uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* d_prior,
                                   int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                                   uint32_t flags, int64_t* d_counters, void* stream)
try {
    return mc_run_device(h, mc_call(L_host, k, distance, {McErrors::FAULT, 1, seed, 0.0, nullptr, weight}, trial_begin,
                                    trial_end, {max_iter, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters),
                         stream);
}
QBP_ABI_CATCH

int qbp_mc_run_fault_weight(qbp_handle* h, const uint8_t* L, int32_t k, int32_t distance, int32_t weight, uint64_t seed,
                            int64_t trial_begin, int64_t trial_end, const double* prior, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                            int64_t counters[QBP_NUM_COUNTERS])
try {
    return mc_run_host(h, mc_call(L, k, distance, {McErrors::FAULT, 1, seed, 0.0, nullptr, weight}, trial_begin,
                                  trial_end, {max_iter, variant, alpha, damping, clip_llr, flags}), prior, nullptr,
                       counters, nullptr, nullptr);
}
QBP_ABI_CATCH

int qbp_mc_sample_errors_fault_weight(qbp_handle* h, int32_t weight, uint64_t seed, int64_t trial_begin, int64_t T,
                                      uint8_t* errors)
try {
    return mc_sample_host(h, {McErrors::FAULT, 1, seed, 0.0, nullptr, weight}, trial_begin, T, errors);
}
QBP_ABI_CATCH

int qbp_mc_run_probs_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                            const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                            int64_t trial_end, const double* d_prior, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr,
                            uint32_t flags, int64_t* d_counters, void* stream)
try {
    return mc_run_device(h, mc_call(Lx_host, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin,
                                    trial_end, {max_iter, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters),
                         stream);
}
QBP_ABI_CATCH

int qbp_mc_run_probs(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                     int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                     const double* prior, int32_t max_iter, int32_t variant, double alpha,
                     double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS])
try {
    return mc_run_host(h, mc_call(Lx, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin, trial_end,
                                  {max_iter, variant, alpha, damping, clip_llr, flags}), prior, nullptr, counters,
                       nullptr, nullptr);
}
QBP_ABI_CATCH

int qbp_mc_run_budgets_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                              const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                              int64_t trial_end, const double* d_prior, const int32_t* budgets, int32_t n_budgets,
                              int32_t variant, double alpha, double damping, double clip_llr,
                              uint32_t flags, int64_t* d_counters, void* stream)
try {
    McCall c = mc_call(Lx_host, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin, trial_end,
                       {0, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters);
    c.out = McCall::LADDER; c.budgets = budgets; c.n_budgets = n_budgets;
    return mc_run_device(h, c, stream);
}
QBP_ABI_CATCH

int qbp_mc_run_budgets(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                       int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                       const double* prior, const int32_t* budgets, int32_t n_budgets, int32_t variant,
                       double alpha, double damping, double clip_llr, uint32_t flags, int64_t* counters)
try {
    McCall c = mc_call(Lx, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin, trial_end,
                       {0, variant, alpha, damping, clip_llr, flags});
    c.out = McCall::LADDER; c.budgets = budgets; c.n_budgets = n_budgets;
    return mc_run_host(h, c, prior, nullptr, counters, nullptr, nullptr);
}
QBP_ABI_CATCH

// A ladder call that also fills the posterior-LLR table
static McCall llr_hist_call(McCall c, const int32_t* budgets, int32_t n_budgets, double llr_lo, double llr_hi, int32_t bins,
                            int64_t* d_hist = nullptr)
{
    c.out = McCall::LLRHIST; c.budgets = budgets; c.n_budgets = n_budgets;
    c.llr_lo = llr_lo; c.llr_hi = llr_hi; c.llr_bins = bins; c.d_llr_hist = d_hist;
    return c;
}

int qbp_mc_run_llr_hist_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance, const double* probs,
                               int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                               const double* d_prior, const int32_t* budgets, int32_t n_budgets, int32_t variant,
                               double alpha, double damping, double clip_llr, uint32_t flags, double llr_lo,
                               double llr_hi, int32_t bins, int64_t* d_counters, int64_t* d_hist, void* stream)
try {
    return mc_run_device(h, llr_hist_call(mc_call(Lx_host, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs},
                                                  trial_begin, trial_end, {0, variant, alpha, damping, clip_llr, flags},
                                                  d_prior, d_counters),
                                          budgets, n_budgets, llr_lo, llr_hi, bins, d_hist), stream);
}
QBP_ABI_CATCH

int qbp_mc_run_llr_hist(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                        int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* prior,
                        const int32_t* budgets, int32_t n_budgets, int32_t variant, double alpha, double damping,
                        double clip_llr, uint32_t flags, double llr_lo, double llr_hi, int32_t bins, int64_t* counters,
                        int64_t* hist)
try {
    return mc_run_host(h, llr_hist_call(mc_call(Lx, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin,
                                                trial_end, {0, variant, alpha, damping, clip_llr, flags}),
                                        budgets, n_budgets, llr_lo, llr_hi, bins), prior, nullptr, counters, hist, nullptr);
}
QBP_ABI_CATCH

// (T patterns instead of a sampler: counters SET, hist added to)
int qbp_mc_run_errors_llr_hist(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                               int64_t T, const double* prior, const int32_t* budgets, int32_t n_budgets,
                               int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                               double llr_lo, double llr_hi, int32_t bins, int64_t* counters, int64_t* hist)
try {
    return mc_run_host(h, llr_hist_call(mc_call(Lx, k, distance, {McErrors::STORED}, 0, T,
                                                {0, variant, alpha, damping, clip_llr, flags}),
                                        budgets, n_budgets, llr_lo, llr_hi, bins), prior, errors, counters, hist, nullptr);
}
QBP_ABI_CATCH

int qbp_mc_run_spectrum_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                               const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                               int64_t trial_end, const double* d_prior, int32_t max_iter,
                               int32_t variant, double alpha, double damping, double clip_llr,
                               uint32_t flags, int64_t* d_counters, int64_t* d_spectrum, int64_t* d_iter_hist,
                               void* stream)
try {
    McCall c = mc_call(Lx_host, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin, trial_end,
                       {max_iter, variant, alpha, damping, clip_llr, flags}, d_prior, d_counters);
    c.out = McCall::SPECTRUM; c.d_spectrum = d_spectrum; c.d_iter_hist = d_iter_hist;
    return mc_run_device(h, c, stream);
}
QBP_ABI_CATCH

int qbp_mc_run_spectrum(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                        int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                        const double* prior, int32_t max_iter, int32_t variant, double alpha,
                        double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS],
                        int64_t* spectrum, int64_t* iter_hist)
try {
    McCall c = mc_call(Lx, k, distance, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin, trial_end,
                       {max_iter, variant, alpha, damping, clip_llr, flags});
    c.out = McCall::SPECTRUM;
    return mc_run_host(h, c, prior, nullptr, counters, spectrum, iter_hist);
}
QBP_ABI_CATCH

int qbp_mc_run_errors_spectrum(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                               int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                               double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS],
                               int64_t* spectrum, int64_t* iter_hist)
try {
    McCall c = mc_call(Lx, k, distance, {McErrors::STORED}, 0, T, {max_iter, variant, alpha, damping, clip_llr, flags});
    c.out = McCall::SPECTRUM;
    return mc_run_host(h, c, prior, errors, counters, spectrum, iter_hist);
}
QBP_ABI_CATCH

int qbp_mc_sample_errors_probs(qbp_handle* h, const double* probs, int32_t draws, uint64_t seed,
                               int64_t trial_begin, int64_t T, uint8_t* errors)
try {
    return mc_sample_host(h, {McErrors::PROBS, draws, seed, 0.0, probs}, trial_begin, T, errors);
}
QBP_ABI_CATCH

// ---- recorded shots (include/qbp.h: qbp_decode_shots) -----------------------------------------------------------

// Everything qbp_decode_shots refuses, host only and before any GPU work.  `host_prior`: the priors when they are a
// host array (NaN check), else null.
static int check_shots_args(qbp_handle* h, const uint8_t* Lx, int32_t k, const uint8_t* det_bits, int64_t T,
                            const double* prior, const double* host_prior, int32_t max_iter, int32_t variant,
                            uint32_t flags, const int64_t* counters, int* osd_method, int* osd_order)
{
    int rc = check_decode_args(h, T, max_iter, variant);
    if (rc) return rc;
    if (!Lx || !det_bits || !prior || !counters) return fail(QBP_E_INVALID, "null pointer");
    if (k < 1 || k > 64) return fail(QBP_E_INVALID, "k = %d observables (need 1..64)", k);
    if ((rc = check_relay_flags(h, flags, true)) != QBP_OK) return rc;
    if ((rc = check_gd_flags(h, flags, true)) != QBP_OK) return rc;
    if ((rc = check_lsd_flags(h, flags, true)) != QBP_OK) return rc;
    if ((rc = check_layered_flags(h, flags, 0, true)) != QBP_OK) return rc;
    if ((rc = check_quant_flags(h, flags, 0, true)) != QBP_OK) return rc;
    if (host_prior && (rc = check_prior(h->n, host_prior, false)) != QBP_OK) return rc;
    rc = parse_osd_flags(h, flags, true, osd_method, osd_order);
    if (rc) return rc;
    if (flags & QBP_FLAG_OSD0) {
        // per-shot records of the shots BP leaves unconverged, as qbp_mc_run's (without the error row)
        const size_t t = (size_t)T, m = h->m, n = h->n;
        if (t > QBP_MC_OSD_MAX_TRIALS || t * (m + 10 * n) > ((size_t)16 << 30))
            return fail(QBP_E_INVALID, "with QBP_FLAG_OSD0 a call covers at most %lld shots of this matrix (got %lld); "
                                       "split the range",
                        (long long)std::min<size_t>(QBP_MC_OSD_MAX_TRIALS, ((size_t)16 << 30) / (m + 10 * n)), (long long)T);
    }
    return QBP_OK;
}

// All pointers but Lx_host are device pointers; arguments already checked.
static int decode_shots_impl(qbp_handle* h, const uint8_t* Lx_host, int32_t k, const uint8_t* d_det_bits,
                             const uint64_t* d_actual, int64_t T, const double* d_prior, int32_t max_iter,
                             int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                             int osd_method, int osd_order, uint64_t* d_predictions, uint8_t* d_converged,
                             int64_t* d_counters, hipStream_t s)
{
    flags &= ~OSD_ALL_BITS;
    BpCall c;
    int rc = resolve_column_order(h, flags, nullptr, &c.col_mode);      // the column-sum bits of qbp_decode_batch
    if (rc) return rc;
    rc = mc_prepare(h, Lx_host, k, s);
    if (rc) return rc;
    const bool osd = (flags & QBP_FLAG_OSD0) != 0;
    McArgs mc{};
    if (osd && (rc = mc_fail_records(h, mc, 1, (size_t)T, false, s)) != QBP_OK) return rc;
    mc.lx_cols = h->mc_in.d_lx_cols.p;
    mc.counters = reinterpret_cast<long long*>(d_counters);
    mc.det_bits = d_det_bits; mc.det_row_bytes = (h->m + 7) / 8;
    mc.actual = reinterpret_cast<const unsigned long long*>(d_actual);
    mc.predictions = reinterpret_cast<unsigned long long*>(d_predictions);
    c.prior = d_prior; c.B = T; c.max_iter = max_iter; c.variant = variant;
    c.alpha = alpha; c.damping = damping; c.clip_llr = clip_llr; c.flags = flags;
    c.converged = d_converged;
    c.mc = &mc;
    // (two column orders in one launch: the general-H kernel only, as in bp_kernel)
    if (bp_kernel(h, T, flags, c.col_mode, true) == 2 || c.col_mode == 2) {
        h->last_kernel = 2;
        rc = generic_launch(h, c, s);
    } else {
        rc = fused_launch(h, c, s);
        if (rc == QBP_OK) h->last_kernel = 1;
    }
    if (rc || !osd) return rc;
    // second kernel: OSD on the shots BP left unconverged (their number is read on the device), predicting them;
    // recorded syndromes may lie outside the column space of H: with the redo pass of qbp_osd_batch
    qbp::OsdParams O{};
    O.count_ptr = reinterpret_cast<const long long*>(h->d_fail_count.p);
    O.list = h->d_fail_list.p;
    O.syndromes = h->d_fail_syn.p; O.llr = h->d_fail_llr.p; O.hard = h->d_fail_hard.p;
    O.lx_cols = h->mc_in.d_lx_cols.p;
    O.counters = reinterpret_cast<long long*>(d_counters);
    O.shots = 1; O.actual = mc.actual; O.predictions = mc.predictions;
    return osd_launch(h, O, T, s, true, osd_method, osd_order);
}

int qbp_decode_shots_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, const uint8_t* d_det_bits,
                            const uint64_t* d_actual, int64_t T, const double* d_prior, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                            uint64_t* d_predictions, uint8_t* d_converged, int64_t* d_counters, void* stream)
try {
    int osd_method = 0, osd_order = 0;
    const int rc = check_shots_args(h, Lx_host, k, d_det_bits, T, d_prior, nullptr, max_iter, variant, flags,
                                    d_counters, &osd_method, &osd_order);
    if (rc) return rc;
    if (T == 0) return QBP_OK;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    return decode_shots_impl(h, Lx_host, k, d_det_bits, d_actual, T, d_prior, max_iter, variant, alpha, damping,
                             clip_llr, flags, osd_method, osd_order, d_predictions, d_converged, d_counters,
                             static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_decode_shots(qbp_handle* h, const uint8_t* Lx, int32_t k, const uint8_t* det_bits, const uint64_t* actual,
                     int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha, double damping,
                     double clip_llr, uint32_t flags, uint64_t* predictions, uint8_t* converged,
                     int64_t counters[QBP_NUM_COUNTERS])
try {
    int osd_method = 0, osd_order = 0;
    int rc = check_shots_args(h, Lx, k, det_bits, T, prior, prior, max_iter, variant, flags, counters, &osd_method,
                              &osd_order);
    if (rc) return rc;
    if (T == 0) return QBP_OK;
    if (flags & QBP_FLAG_DENSE_F_COLSUM_ITER0) {     // (the shortcut is judged on the host copy of the priors)
        int mode = 0;
        unsigned fl = flags;
        rc = resolve_column_order(h, fl, prior, &mode);
        if (rc) return rc;
        if (mode == 0) flags = fl;
    }
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t n = h->n, t = (size_t)T, rb = ((size_t)h->m + 7) / 8;
    HostStage st(h->stream);
    const uint8_t* d_det = st.in(h->d_syn, det_bits, t * rb);
    const double* d_prior = st.in(h->d_prior, prior, n);
    const unsigned long long* d_actual =
        actual ? st.in(h->d_shot_actual, reinterpret_cast<const unsigned long long*>(actual), t) : nullptr;
    unsigned long long* d_pred = st.out(h->d_shot_pred, reinterpret_cast<unsigned long long*>(predictions), t);
    uint8_t* d_conv = st.out(h->d_conv, converged, t);
    long long* d_cnt = st.zeroed(h->d_counters, qbp::NUM_COUNTERS);
    st.add(counters, d_cnt, qbp::NUM_COUNTERS);           // (ADDED to the caller's)
    if (st.failed()) return st.error();
    return st.finish(decode_shots_impl(h, Lx, k, d_det, reinterpret_cast<const uint64_t*>(d_actual), T, d_prior, max_iter,
                                       variant, alpha, damping, clip_llr, flags, osd_method, osd_order,
                                       reinterpret_cast<uint64_t*>(d_pred), d_conv, reinterpret_cast<int64_t*>(d_cnt),
                                       h->stream));
}
QBP_ABI_CATCH

// ---- failing patterns of an enumerated weight class (include/qbp.h: qbp_enum_failures) ----------------------------

// Patterns per chunk of a qbp_enum_failures call over T ranks: the chunk of the Monte-Carlo entries, and with OSD no
// more than the records of one shots call may take (16 GiB; QBP_MC_OSD_MAX_TRIALS is the largest chunk there is)
static long long enum_failures_chunk(const qbp_handle* h, int64_t T, uint32_t flags)
{
    long long chunk = mc_chunk_trials(h, T);
    if (flags & QBP_FLAG_OSD0)
        chunk = std::min<long long>(chunk, (long long)(((size_t)16 << 30) / ((size_t)h->m + 10 * (size_t)h->n)));
    return std::max<long long>(chunk, 1);
}

// Everything qbp_enum_failures and qbp_fault_weight_failures refuse, host only and before any GPU work; `e`: the filler,
// ENUM or FAULT
static int check_enum_failures(qbp_handle* h, const uint8_t* Lx, int32_t k, const McErrors& e, int64_t rank_begin,
                               int64_t rank_end, const double* prior, const double* host_prior, int32_t max_iter,
                               int32_t variant, uint32_t flags, int32_t what, int64_t cap, const int64_t* ranks,
                               const uint8_t* kinds, const int64_t* found, const int64_t* counters, int* osd_method,
                               int* osd_order)
{
    if (!h) return fail(QBP_E_INVALID, "null handle");
    int rc = check_mc_errors(h, e, rank_begin, rank_end);
    if (rc) return rc;
    if (rank_end < rank_begin) return fail(QBP_E_INVALID, "trial_end must be >= trial_begin");
    if (what < 1 || what > 3) return fail(QBP_E_INVALID, "what = %d (need 1 logical, 2 unconverged, or 3 either)", what);
    if (cap < 0) return fail(QBP_E_INVALID, "cap must be >= 0 (got %lld)", (long long)cap);
    if (!found) return fail(QBP_E_INVALID, "found is null");
    if (cap > 0 && (!ranks || !kinds)) return fail(QBP_E_INVALID, "ranks or kinds is null with cap > 0");
    // the shots calls of the chunks: what qbp_decode_shots refuses (its rows are the handle's: Lx stands for them)
    return check_shots_args(h, Lx, k, Lx, enum_failures_chunk(h, rank_end - rank_begin, flags), prior, host_prior, max_iter,
                            variant, flags, counters, osd_method, osd_order);
}

// A checked call on the stream, every pointer but Lx_host a device pointer: chunk by chunk the enumeration, the shot
// of every row, the launches of qbp_decode_shots, the capture.  Nothing returns to the host in between.  `e`: the filler
// of the rows (mc_sample), the enumeration or the fixed-weight fault sampler, whose trial index is captured instead.
static int enum_failures_run(qbp_handle* h, const uint8_t* Lx_host, int32_t k, const McErrors& e, int64_t rank_begin,
                             int64_t rank_end, const double* d_prior, int32_t max_iter, int32_t variant, double alpha,
                             double damping, double clip_llr, uint32_t flags, int osd_method, int osd_order, int32_t what,
                             int64_t cap, int64_t* d_ranks, uint8_t* d_kinds, int64_t* d_found, int64_t* d_counters,
                             hipStream_t s)
{
    if (rank_end == rank_begin) return QBP_OK;
    int rc = mc_prepare(h, Lx_host, k, s);
    if (rc) return rc;
    if (e.kind == McErrors::ENUM && (rc = enum_prepare(h, e.weight, s)) != QBP_OK) return rc;
    const long long chunk = enum_failures_chunk(h, rank_end - rank_begin, flags);
    const size_t c = (size_t)chunk, n = (size_t)h->n, rb = ((size_t)h->m + 7) / 8;
    HIP_TRY(h->d_weight_err.reserve(c * n));
    HIP_TRY(h->d_enum_det.reserve(c * rb));
    HIP_TRY(h->d_enum_actual.reserve(c));
    HIP_TRY(h->d_enum_pred.reserve(c));
    HIP_TRY(h->d_enum_conv.reserve(c));
    for (int64_t a = rank_begin; a < rank_end; a += chunk) {
        const long long t = std::min<long long>(chunk, rank_end - a);
        HIP_TRY(mc_sample(h, e, h->d_weight_err.p, t, a, s));
        HIP_TRY(qbp::launch_enum_pack(h->d_weight_err.p, t, h->m, h->n, h->d_row_ptr.p, h->d_col_idx.p,
                                      h->mc_in.d_lx_cols.p, h->d_enum_det.p, h->d_enum_actual.p, s));
        rc = decode_shots_impl(h, Lx_host, k, h->d_enum_det.p, reinterpret_cast<const uint64_t*>(h->d_enum_actual.p), t,
                               d_prior, max_iter, variant, alpha, damping, clip_llr, flags, osd_method, osd_order,
                               reinterpret_cast<uint64_t*>(h->d_enum_pred.p), h->d_enum_conv.p, d_counters, s);
        if (rc) return rc;
        HIP_TRY(qbp::launch_enum_capture(h->d_enum_pred.p, h->d_enum_actual.p, h->d_enum_conv.p, t, a, what, cap,
                                         reinterpret_cast<long long*>(d_ranks), d_kinds,
                                         reinterpret_cast<unsigned long long*>(d_found), s));
    }
    return QBP_OK;
}

// The _device entries of the two fillers: the check, then the launches.
static int failures_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, const McErrors& e, int64_t rank_begin,
                           int64_t rank_end, const double* d_prior, int32_t max_iter, int32_t variant, double alpha,
                           double damping, double clip_llr, uint32_t flags, int32_t what, int64_t cap,
                           int64_t* d_ranks, uint8_t* d_kinds, int64_t* d_found, int64_t* d_counters, void* stream)
{
    int osd_method = 0, osd_order = 0;
    const int rc = check_enum_failures(h, Lx_host, k, e, rank_begin, rank_end, d_prior, nullptr, max_iter, variant,
                                       flags, what, cap, d_ranks, d_kinds, d_found, d_counters, &osd_method, &osd_order);
    if (rc) return rc;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    return enum_failures_run(h, Lx_host, k, e, rank_begin, rank_end, d_prior, max_iter, variant, alpha, damping,
                             clip_llr, flags, osd_method, osd_order, what, cap, d_ranks, d_kinds, d_found, d_counters,
                             static_cast<hipStream_t>(stream));
}

// The host-array entries of the two fillers: the check, the prior uploaded, the run on the handle's stream and buffers,
// the captured entries sorted and copied back.
static int failures_host(qbp_handle* h, const uint8_t* Lx, int32_t k, const McErrors& e, int64_t rank_begin,
                         int64_t rank_end, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                         double damping, double clip_llr, uint32_t flags, int32_t what, int64_t cap, int64_t* ranks,
                         uint8_t* kinds, int64_t* found, int64_t* counters)
{
    int osd_method = 0, osd_order = 0;
    int rc = check_enum_failures(h, Lx, k, e, rank_begin, rank_end, prior, prior, max_iter, variant, flags, what,
                                 cap, ranks, kinds, found, counters, &osd_method, &osd_order);
    if (rc) return rc;
    if (rank_end == rank_begin) { found[0] = 0; return QBP_OK; }
    if (flags & QBP_FLAG_DENSE_F_COLSUM_ITER0) {     // (as qbp_decode_shots: judged on the host copy of the priors)
        int mode = 0;
        unsigned fl = flags;
        rc = resolve_column_order(h, fl, prior, &mode);
        if (rc) return rc;
        if (mode == 0) flags = fl;
    }
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    // (no more can be captured than the range holds)
    const size_t room = (size_t)std::min<int64_t>(cap, rank_end - rank_begin);
    std::vector<std::pair<long long, uint8_t>> hits;
    unsigned long long n_found = 0;
    {
        HostStage st(h->stream);
        const double* d_prior = st.in(h->d_prior, prior, (size_t)h->n);
        long long* d_cnt = st.zeroed(h->d_counters, qbp::NUM_COUNTERS);
        st.add(counters, d_cnt, qbp::NUM_COUNTERS);           // (ADDED to the caller's)
        if (st.failed()) return st.error();
        HIP_TRY(h->d_enum_ranks.reserve(room));
        HIP_TRY(h->d_enum_kinds.reserve(room));
        HIP_TRY(h->d_enum_found.reserve(1));
        HIP_TRY(hipMemsetAsync(h->d_enum_found.p, 0, sizeof(unsigned long long), h->stream));
        rc = st.finish(enum_failures_run(h, Lx, k, e, rank_begin, rank_end, d_prior, max_iter, variant, alpha,
                                         damping, clip_llr, flags, osd_method, osd_order, what, (int64_t)room,
                                         reinterpret_cast<int64_t*>(h->d_enum_ranks.p), h->d_enum_kinds.p,
                                         reinterpret_cast<int64_t*>(h->d_enum_found.p),
                                         reinterpret_cast<int64_t*>(d_cnt), h->stream));
        if (rc) return rc;
    }
    // (the stream is idle: finish synchronised)
    HIP_TRY(hipMemcpy(&n_found, h->d_enum_found.p, sizeof(n_found), hipMemcpyDeviceToHost));
    const size_t kept = (size_t)std::min<unsigned long long>(n_found, room);
    std::vector<long long> r(kept);
    std::vector<uint8_t> kd(kept);
    if (kept) {
        HIP_TRY(hipMemcpy(r.data(), h->d_enum_ranks.p, kept * sizeof(long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(kd.data(), h->d_enum_kinds.p, kept, hipMemcpyDeviceToHost));
    }
    hits.resize(kept);
    for (size_t i = 0; i < kept; ++i) hits[i] = {r[i], kd[i]};
    std::sort(hits.begin(), hits.end());                       // (ascending rank: specified when all were kept)
    for (size_t i = 0; i < kept; ++i) { ranks[i] = hits[i].first; kinds[i] = hits[i].second; }
    found[0] = (int64_t)n_found;
    return QBP_OK;
}

int qbp_enum_failures_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t weight, int64_t rank_begin,
                             int64_t rank_end, const double* d_prior, int32_t max_iter, int32_t variant, double alpha,
                             double damping, double clip_llr, uint32_t flags, int32_t what, int64_t cap,
                             int64_t* d_ranks, uint8_t* d_kinds, int64_t* d_found, int64_t* d_counters, void* stream)
try {
    return failures_device(h, Lx_host, k, {McErrors::ENUM, 1, 0, 0.0, nullptr, weight}, rank_begin, rank_end, d_prior,
                           max_iter, variant, alpha, damping, clip_llr, flags, what, cap, d_ranks, d_kinds, d_found,
                           d_counters, stream);
}
QBP_ABI_CATCH

int qbp_enum_failures(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t weight, int64_t rank_begin, int64_t rank_end,
                      const double* prior, int32_t max_iter, int32_t variant, double alpha, double damping,
                      double clip_llr, uint32_t flags, int32_t what, int64_t cap, int64_t* ranks, uint8_t* kinds,
                      int64_t found[1], int64_t counters[QBP_NUM_COUNTERS])
try {
    return failures_host(h, Lx, k, {McErrors::ENUM, 1, 0, 0.0, nullptr, weight}, rank_begin, rank_end, prior, max_iter,
                         variant, alpha, damping, clip_llr, flags, what, cap, ranks, kinds, found, counters);
}
QBP_ABI_CATCH

int qbp_fault_weight_failures_device(qbp_handle* h, const uint8_t* L_host, int32_t k, int32_t weight, uint64_t seed,
                                     int64_t trial_begin, int64_t trial_end, const double* d_prior, int32_t max_iter,
                                     int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                                     int32_t what, int64_t cap, int64_t* d_trials, uint8_t* d_kinds, int64_t* d_found,
                                     int64_t* d_counters, void* stream)
try {
    return failures_device(h, L_host, k, {McErrors::FAULT, 1, seed, 0.0, nullptr, weight}, trial_begin, trial_end,
                           d_prior, max_iter, variant, alpha, damping, clip_llr, flags, what, cap, d_trials, d_kinds,
                           d_found, d_counters, stream);
}
QBP_ABI_CATCH

int qbp_fault_weight_failures(qbp_handle* h, const uint8_t* L, int32_t k, int32_t weight, uint64_t seed,
                              int64_t trial_begin, int64_t trial_end, const double* prior, int32_t max_iter,
                              int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                              int32_t what, int64_t cap, int64_t* trials, uint8_t* kinds, int64_t found[1],
                              int64_t counters[QBP_NUM_COUNTERS])
try {
    return failures_host(h, L, k, {McErrors::FAULT, 1, seed, 0.0, nullptr, weight}, trial_begin, trial_end, prior,
                         max_iter, variant, alpha, damping, clip_llr, flags, what, cap, trials, kinds, found, counters);
}
QBP_ABI_CATCH

int qbp_set_option(qbp_handle* h, int32_t option, int64_t value)
try {
    if (option == QBP_OPT_DEBUG_THROW) {          // tests: what an exception inside an entry point turns into
        if (value == 1) throw std::bad_alloc();
        if (value == 2) throw std::runtime_error("requested by QBP_OPT_DEBUG_THROW");
        if (value == 3) throw 3;
        return QBP_OK;
    }
    if (!h) return fail(QBP_E_INVALID, "null handle");
    switch (option) {
        case QBP_OPT_SLOTS_PER_BLOCK:
            if (value < 0 || value * h->m > qbp::FUSED_MAX_THREADS) return fail(QBP_E_INVALID, "slots*m must be <= %d", qbp::FUSED_MAX_THREADS);
            h->opt_slots = (int)value; return QBP_OK;
        case QBP_OPT_BLOCKS_PER_CU:
            if (value < 0 || value > 32) return fail(QBP_E_INVALID, "blocks per CU out of range");
            h->opt_blocks_per_cu = (int)value; return QBP_OK;
        case QBP_OPT_FORCE_GENERIC:
            h->opt_force_generic = value != 0; return QBP_OK;
        case QBP_OPT_KERNEL:
            if (value < 0 || value > 3) return fail(QBP_E_INVALID, "kernel selector out of range");
            h->opt_kernel = (int)value; return QBP_OK;
        case QBP_OPT_EARLY_EXIT_FULL_WG:
            h->opt_early_exit_full_wg = value != 0; return QBP_OK;
        case QBP_OPT_NO_FIRST_STEP_TABLE:
            h->opt_no_r0_table = value != 0; return QBP_OK;
        case QBP_OPT_FORCED_TWO_BARRIERS:
            h->opt_forced_two_barriers = value != 0; return QBP_OK;
        case QBP_OPT_OSD_BIG:
            if (value < 0 || value > 3) return fail(QBP_E_INVALID, "OSD kernel selector out of range");
            h->opt_osd_big = (int)value;
            h->osd_ok = value == 0 && osd_one_wave(h);
            return QBP_OK;
        case QBP_OPT_GENERAL_NO_LDS_TABLES:
            h->opt_no_lds_tables = value != 0; return QBP_OK;
        case QBP_OPT_GENERAL_NO_R_SPLIT:
            h->opt_no_r_split = value != 0; return QBP_OK;
        case QBP_OPT_GENERAL_MEM:
            if (value < 0 || value > 2) return fail(QBP_E_INVALID, "memory mode out of range");
            h->opt_mem = (int)value; return QBP_OK;
        case QBP_OPT_MC_WEIGHT_CHUNK:
            if (value < 0 || value > (1 << 20)) return fail(QBP_E_INVALID, "trials per chunk out of [0, 2^20]");
            h->opt_weight_chunk = value; return QBP_OK;
        case QBP_OPT_LLR_HIST_CHUNK:
            if (value < 0) return fail(QBP_E_INVALID, "trials per launch must be >= 0");
            h->opt_llr_hist_chunk = value; return QBP_OK;
        case QBP_OPT_LAYERED_SLOTS:
            if (value < 0 || value > qbp::LAYERED_MAX_SLOTS) return fail(QBP_E_INVALID, "layered slots out of [0, %d]", qbp::LAYERED_MAX_SLOTS);
            h->opt_layered_slots = (int)value; return QBP_OK;
        case QBP_OPT_QUANT_SLOTS:
            if (value < 0 || value > qbp::QUANT_MAX_SLOTS) return fail(QBP_E_INVALID, "fixed-point slots out of [0, %d]", qbp::QUANT_MAX_SLOTS);
            h->opt_quant_slots = (int)value; return QBP_OK;
        case QBP_OPT_LAYERED_MEM:
        case QBP_OPT_RELAY_MEM:
        case QBP_OPT_GD_MEM:
        case QBP_OPT_LSD_MEM: {
            const int family = option == QBP_OPT_LAYERED_MEM ? qbp::MSG_MEM_LAYERED
                             : option == QBP_OPT_RELAY_MEM   ? qbp::MSG_MEM_RELAY
                             : option == QBP_OPT_GD_MEM      ? qbp::MSG_MEM_GD : qbp::MSG_MEM_LSD;
            static const char* const out_of_range[qbp::MSG_MEM_FAMILIES] = {       // (by qbp::MsgMemFamily)
                "Relay-BP memory mode out of range", "layered BP memory mode out of range",
                "BP guided decimation memory mode out of range", "localized statistics decoding memory mode out of range"};
            if (value < qbp::MSG_MEM_LDS || value > qbp::MSG_MEM_AUTO) return fail(QBP_E_INVALID, "%s", out_of_range[family]);
            h->opt_msg_mem[family] = (int)value; return QBP_OK;
        }
        case QBP_OPT_GENERAL_THREADS:
            if (value < 0 || value > 1024) return fail(QBP_E_INVALID, "threads per workgroup out of range");
            h->opt_threads = (int)value; return QBP_OK;
        default: return fail(QBP_E_INVALID, "unknown option %d", option);
    }
}
QBP_ABI_CATCH

int64_t qbp_get_info(qbp_handle* h, int32_t what)
try {
    if (!h) return -1;
    switch (what) {
        case QBP_INFO_M: return h->m;
        case QBP_INFO_N: return h->n;
        case QBP_INFO_EDGES: return h->E;
        case QBP_INFO_MAX_ROW_DEG: return h->max_row_deg;
        case QBP_INFO_MAX_COL_DEG: return h->max_col_deg;
        case QBP_INFO_KERNEL_KIND: {   // the kernel a decode call would use (small batch), see also ..._LAST
            const int kernel = bp_kernel(h, 1, 0, 0, false);
            return kernel > 0 ? kernel : h->opt_kernel;   // (the forced on-chip kernel, which that call refuses)
        }
        case QBP_INFO_LAST_KERNEL: return h->last_kernel;
        case QBP_INFO_ONE_BARRIER: return h->last_one_barrier;
        case QBP_INFO_THREADS: return h->last_threads;
        case QBP_INFO_LDS_BYTES: return h->last_lds;
        case QBP_INFO_GRID: return h->last_grid;
        case QBP_INFO_NUM_CU: return h->num_cu;
        default: return -1;
    }
}
catch (...) { return -1; }

int qbp_debug_math(qbp_handle* h, int32_t kind, const double* x, double* y, int64_t count)
try {
    if (!h || !x || !y || count < 0 || kind < 0 || kind > 5) return fail(QBP_E_INVALID, "bad arguments");
    if (count == 0) return QBP_OK;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    HIP_TRY(h->d_mathx.reserve((size_t)count));
    HIP_TRY(h->d_mathy.reserve((size_t)count));
    hipStream_t s = h->stream;
    HIP_TRY(hipMemcpyAsync(h->d_mathx.p, x, (size_t)count * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(qbp::launch_debug_math(kind, h->d_mathx.p, h->d_mathy.p, (long long)count, s));
    HIP_TRY(hipMemcpyAsync(y, h->d_mathy.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QBP_OK;
}
QBP_ABI_CATCH

// ---- sliding-window decoding (include/qbp.h, qbp_window_*; glue kernels: qbp_window.hpp) ---------------------------
// The partition of rule 1, host only: windows, their checks C_k and variables U_k, the commit flags, and the classes of
// identical local CSR (the first window of a class keeps it for qbp_create).
struct WindowPlan {
    int R = 0, K = 0;
    std::vector<int32_t> check_ptr, checks, var_ptr, vars, cls;      // cls[k] = -1: window k is skipped (rule 0)
    std::vector<uint8_t> commit;
    std::vector<std::vector<int32_t>> cls_row_ptr, cls_col_idx;
    std::vector<int> cls_n;
};

// Bounds of a plan: rounds need not be contiguous, so one large round number must not turn into hours of empty windows
// or tables beyond int32 (QBP_E_INVALID beyond these).
constexpr int WINDOW_MAX_ROUNDS = 1 << 20;
constexpr long long WINDOW_MAX_ENTRIES = (long long)1 << 28;      // sum of |C_k|, and of |U_k|

static int window_plan(const int32_t* row_ptr, const int32_t* col_idx, int m, int n, const int32_t* check_round, int W,
                       int F, WindowPlan& P)
{
    const int rc = check_csr(row_ptr, col_idx, m, n);
    if (rc) return rc;
    if (!check_round) return fail(QBP_E_INVALID, "check_round is null");
    if (W < 1) return fail(QBP_E_INVALID, "window size W = %d (need >= 1)", W);
    if (F < 1 || F > W) return fail(QBP_E_INVALID, "commit size F = %d outside [1, W = %d]", F, W);
    for (int c = 0; c < m; ++c) {
        if (check_round[c] < 0) return fail(QBP_E_INVALID, "check_round[%d] = %d is negative", c, check_round[c]);
        if (check_round[c] >= WINDOW_MAX_ROUNDS)
            return fail(QBP_E_INVALID, "check_round[%d] = %d: rounds must be below %d", c, check_round[c], WINDOW_MAX_ROUNDS);
        P.R = std::max(P.R, check_round[c] + 1);
    }
    std::vector<int32_t> var_round((size_t)n, INT32_MAX);
    for (int c = 0; c < m; ++c)
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e)
            var_round[col_idx[e]] = std::min(var_round[col_idx[e]], check_round[c]);
    for (int v = 0; v < n; ++v)
        if (var_round[v] == INT32_MAX) var_round[v] = 0;
    long long k_last = 0;
    while (k_last * F + W < P.R) ++k_last;
    P.K = (int)k_last + 1;
    // checks and variables sorted by round (ties by index): a window is a range of each, whatever R is
    std::vector<int32_t> by_check((size_t)m), by_var((size_t)n);
    for (int c = 0; c < m; ++c) by_check[c] = c;
    for (int v = 0; v < n; ++v) by_var[v] = v;
    std::stable_sort(by_check.begin(), by_check.end(), [&](int a, int b) { return check_round[a] < check_round[b]; });
    std::stable_sort(by_var.begin(), by_var.end(), [&](int a, int b) { return var_round[a] < var_round[b]; });
    auto range = [](const std::vector<int32_t>& by, const int32_t* round, long long lo, long long hi, std::vector<int32_t>& out) {
        auto first = std::lower_bound(by.begin(), by.end(), lo, [&](int a, long long x) { return round[a] < x; });
        auto last = std::lower_bound(first, by.end(), hi, [&](int a, long long x) { return round[a] < x; });
        out.assign(first, last);
        std::sort(out.begin(), out.end());
    };
    P.check_ptr.assign(1, 0);
    P.var_ptr.assign(1, 0);
    std::vector<int32_t> loc((size_t)n, -1), C, U;
    std::map<std::pair<std::vector<int32_t>, std::vector<int32_t>>, int> seen;   // (row_ptr + [n_k], col_idx) -> class
    for (int k = 0; k < P.K; ++k) {
        const long long lo = (long long)k * F, hi = std::min<long long>(lo + W, P.R);
        const long long commit_hi = k == P.K - 1 ? hi : lo + F;
        range(by_check, check_round, lo, hi, C);
        range(by_var, var_round.data(), lo, hi, U);
        if ((long long)P.checks.size() + (long long)C.size() > WINDOW_MAX_ENTRIES ||
            (long long)P.vars.size() + (long long)U.size() > WINDOW_MAX_ENTRIES)
            return fail(QBP_E_INVALID, "the windows hold more than 2^28 checks or variables in all (W = %d, F = %d)", W, F);
        P.checks.insert(P.checks.end(), C.begin(), C.end());
        P.check_ptr.push_back((int32_t)P.checks.size());
        for (size_t j = 0; j < U.size(); ++j) {
            P.vars.push_back(U[j]);
            P.commit.push_back(var_round[U[j]] < commit_hi ? 1 : 0);
        }
        P.var_ptr.push_back((int32_t)P.vars.size());
        if (C.empty() || U.empty()) { P.cls.push_back(-1); continue; }
        for (size_t j = 0; j < U.size(); ++j) loc[U[j]] = (int32_t)j;
        std::vector<int32_t> rp(1, 0), ci;
        for (int c : C) {
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e)
                if (loc[col_idx[e]] >= 0) ci.push_back(loc[col_idx[e]]);
            rp.push_back((int32_t)ci.size());
        }
        for (int v : U) loc[v] = -1;
        std::vector<int32_t> key_rp = rp;
        key_rp.push_back((int32_t)U.size());
        auto ins = seen.emplace(std::make_pair(std::move(key_rp), ci), (int)P.cls_n.size());
        if (ins.second) {
            P.cls_n.push_back((int)U.size());
            P.cls_row_ptr.push_back(std::move(rp));
            P.cls_col_idx.push_back(std::move(ci));
        }
        P.cls.push_back(ins.first->second);
    }
    return QBP_OK;
}

int qbp_window_plan(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, const int32_t* check_round,
                    int32_t W, int32_t F, int32_t sizes[3], int32_t* win_check_ptr, int32_t* win_checks,
                    int32_t* win_var_ptr, int32_t* win_vars, uint8_t* win_commit, int32_t* win_class)
try {
    if (!sizes) return fail(QBP_E_INVALID, "sizes is null");
    WindowPlan P;
    const int rc = window_plan(row_ptr, col_idx, m, n, check_round, W, F, P);
    if (rc) return rc;
    sizes[0] = P.K; sizes[1] = (int32_t)P.checks.size(); sizes[2] = (int32_t)P.vars.size();
    if (win_check_ptr) std::copy(P.check_ptr.begin(), P.check_ptr.end(), win_check_ptr);
    if (win_checks) std::copy(P.checks.begin(), P.checks.end(), win_checks);
    if (win_var_ptr) std::copy(P.var_ptr.begin(), P.var_ptr.end(), win_var_ptr);
    if (win_vars) std::copy(P.vars.begin(), P.vars.end(), win_vars);
    if (win_commit) std::copy(P.commit.begin(), P.commit.end(), win_commit);
    if (win_class) std::copy(P.cls.begin(), P.cls.end(), win_class);
    return QBP_OK;
}
QBP_ABI_CATCH

struct qbp_window {
    int device = 0, m = 0, n = 0;
    WindowPlan plan;
    std::vector<qbp_handle*> sub;           // one ordinary handle per window class
    // one window: its class handle, sizes, and where its tables start in the device arrays below
    struct Win { qbp_handle* h; int mk, nk, check_off, var_off, n_upd, upd_off, upd_ptr_off, ent_off, n_commit, commit_off; };
    std::vector<Win> win;
    int max_mk = 0, max_nk = 0;
    DevBuf<int32_t> d_checks, d_vars;                       // C_k and U_k, window after window
    DevBuf<int32_t> d_upd_check, d_upd_ptr, d_upd_local;    // the rows of H restricted to M_k (checks with an entry there)
    DevBuf<int32_t> d_commit_local, d_commit_var;           // M_k as positions in U_k and as columns of H
    DevBuf<int32_t> d_row_ptr, d_col_idx;                   // H itself (syndromes of the Monte-Carlo entries)
    // batch workspaces: the running syndrome, one window's inputs and outputs, the failure list and a count per window
    DevBuf<uint8_t> d_r, d_syn, d_hard, d_conv, d_sol;
    DevBuf<int32_t> d_it;
    DevBuf<double> d_llr, d_prior_w;
    DevBuf<long long> d_fail_list;
    DevBuf<unsigned long long> d_fail_count;
    // host-pointer entries and Monte-Carlo
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> d_in_syn, d_x, d_conv_out, d_err;
    DevBuf<double> d_in_prior, d_llr_out;
    DevBuf<int32_t> d_iters, d_fails;
    DevBuf<long long> d_counters;
    McInputs mc_in;
    long long opt_chunk = 0;
};

void qbp_window_destroy(qbp_window* w)
try {
    if (!w) return;
    DeviceScope on_device(w->device);
    for (qbp_handle* h : w->sub) qbp_destroy(h);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
}
catch (...) {
}

int qbp_window_create(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, const int32_t* check_round,
                      int32_t W, int32_t F, int32_t device, qbp_window** out)
try {
    if (!out) return fail(QBP_E_INVALID, "out is null");
    *out = nullptr;
    struct Guard {
        qbp_window* w;
        ~Guard() { if (w) qbp_window_destroy(w); }
    } guard{new qbp_window()};
    qbp_window* w = guard.w;
    WindowPlan& P = w->plan;
    int rc = window_plan(row_ptr, col_idx, m, n, check_round, W, F, P);
    if (rc) return rc;
    w->device = device; w->m = m; w->n = n;
    for (size_t c = 0; c < P.cls_n.size(); ++c) {
        qbp_handle* h = nullptr;
        rc = qbp_create(P.cls_row_ptr[c].data(), P.cls_col_idx[c].data(), (int32_t)P.cls_row_ptr[c].size() - 1, P.cls_n[c],
                        device, &h);
        if (rc) return rc;
        w->sub.push_back(h);
    }
    // the rows of H restricted to each commit set, and the commit sets themselves
    std::vector<int32_t> upd_check, upd_ptr, upd_local, commit_local, commit_var, loc((size_t)n, -1);
    for (int k = 0; k < P.K; ++k) {
        qbp_window::Win x{};
        x.h = P.cls[k] >= 0 ? w->sub[P.cls[k]] : nullptr;     // (null: a skipped window)
        x.check_off = P.check_ptr[k]; x.mk = P.check_ptr[k + 1] - x.check_off;
        x.var_off = P.var_ptr[k]; x.nk = P.var_ptr[k + 1] - x.var_off;
        x.upd_off = (int)upd_check.size(); x.upd_ptr_off = (int)upd_ptr.size(); x.ent_off = (int)upd_local.size();
        x.commit_off = (int)commit_local.size();
        for (int j = 0; j < x.nk; ++j)
            if (P.commit[x.var_off + j]) {
                loc[P.vars[x.var_off + j]] = j;
                commit_local.push_back(j);
                commit_var.push_back(P.vars[x.var_off + j]);
            }
        upd_ptr.push_back(0);
        // (a skipped window commits empty columns only, and a window that commits nothing updates nothing)
        for (int c = 0; x.h && (int)commit_local.size() > x.commit_off && c < m; ++c) {
            const size_t before = upd_local.size();
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e)
                if (loc[col_idx[e]] >= 0) upd_local.push_back(loc[col_idx[e]]);
            if (upd_local.size() == before) continue;
            upd_check.push_back(c);
            upd_ptr.push_back((int32_t)(upd_local.size() - x.ent_off));
        }
        x.n_upd = (int)upd_check.size() - x.upd_off;
        x.n_commit = (int)commit_local.size() - x.commit_off;
        for (int j = x.commit_off; j < (int)commit_var.size(); ++j) loc[commit_var[j]] = -1;
        w->max_mk = std::max(w->max_mk, x.mk);
        w->max_nk = std::max(w->max_nk, x.nk);
        w->win.push_back(x);
    }
    DeviceScope on_device(device);
    HIP_TRY(on_device.err);
    HIP_TRY(w->d_checks.upload(P.checks));
    HIP_TRY(w->d_vars.upload(P.vars));
    HIP_TRY(w->d_upd_check.upload(upd_check));
    HIP_TRY(w->d_upd_ptr.upload(upd_ptr));
    HIP_TRY(w->d_upd_local.upload(upd_local));
    HIP_TRY(w->d_commit_local.upload(commit_local));
    HIP_TRY(w->d_commit_var.upload(commit_var));
    HIP_TRY(w->d_row_ptr.upload(std::vector<int32_t>(row_ptr, row_ptr + m + 1)));
    HIP_TRY(w->d_col_idx.upload(std::vector<int32_t>(col_idx, col_idx + row_ptr[m])));
    HIP_TRY(w->d_fail_count.reserve((size_t)P.K));
    HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    guard.w = nullptr;
    *out = w;
    return QBP_OK;
}
QBP_ABI_CATCH

// Everything a window call refuses, host only and before any GPU work: the flags, and what a sub-handle would refuse.
static int window_check_call(qbp_window* w, int64_t B, int32_t max_iter, int32_t variant, uint32_t flags, int* method,
                             int* order)
{
    if (!w) return fail(QBP_E_INVALID, "null window decoder");
    if (flags & QBP_FLAG_LSD) return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_LSD is not available in a window call");
    if (flags & QBP_FLAG_QUANT) return fail(QBP_E_UNSUPPORTED, "QBP_FLAG_QUANT is not available in a window call");
    if (flags & ~(QBP_FLAG_FORCE_FULL | QBP_FLAG_OSD0 | OSD_ALL_BITS))
        return fail(QBP_E_INVALID, "flags 0x%x: a window call takes QBP_FLAG_FORCE_FULL and the OSD bits only", flags);
    for (qbp_handle* h : w->sub) {
        int rc = check_decode_args(h, B, max_iter, variant);
        if (rc) return rc;
        if ((rc = parse_osd_flags(h, flags & ~QBP_FLAG_FORCE_FULL, false, method, order)) != QBP_OK) return rc;
        if (bp_kernel(h, B, 0, 0, false) < 0) return fail(QBP_E_UNSUPPORTED, "a window's matrix does not fit the forced kernel");
    }
    return QBP_OK;
}

// One checked call on the stream (device pointers; any output may be null): the chain of launches of all windows.
static int window_run(qbp_window* w, const uint8_t* d_syndromes, const double* d_prior, int64_t B, int32_t max_iter,
                      int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags, int method, int order,
                      uint8_t* d_x, uint8_t* d_converged, int32_t* d_iters, double* d_llr, int32_t* d_fails, hipStream_t s,
                      bool gather_prior = true)
{
    const size_t b = (size_t)B, m = w->m;
    const bool osd = (flags & (QBP_FLAG_OSD0 | OSD_METHOD_BITS)) != 0;
    const int K = w->plan.K;
    HIP_TRY(w->d_r.reserve(b * m));
    HIP_TRY(w->d_syn.reserve(b * w->max_mk));
    HIP_TRY(w->d_hard.reserve(b * w->max_nk));
    HIP_TRY(w->d_llr.reserve(b * w->max_nk));
    HIP_TRY(w->d_conv.reserve(b));
    HIP_TRY(w->d_it.reserve(b));
    HIP_TRY(w->d_prior_w.reserve(w->plan.vars.size()));
    if (osd) {
        HIP_TRY(w->d_sol.reserve(b * w->max_nk));
        HIP_TRY(w->d_fail_list.reserve(b));
        HIP_TRY(hipMemsetAsync(w->d_fail_count.p, 0, (size_t)K * sizeof(unsigned long long), s));
    }
    HIP_TRY(hipMemcpyAsync(w->d_r.p, d_syndromes, b * m, hipMemcpyDeviceToDevice, s));
    if (d_iters) HIP_TRY(hipMemsetAsync(d_iters, 0, b * sizeof(int32_t), s));
    if (d_fails) HIP_TRY(hipMemsetAsync(d_fails, 0, b * sizeof(int32_t), s));
    // (the priors of all windows: once per call -- the Monte-Carlo entries pass false from their second chunk on)
    if (gather_prior)
        HIP_TRY(qbp::launch_window_gather_prior(d_prior, w->d_vars.p, (int)w->plan.vars.size(), w->d_prior_w.p, s));
    for (int k = 0; k < K; ++k) {
        const qbp_window::Win& x = w->win[k];
        if (!x.h) {
            // rule 0: nothing is decoded or counted; the variables of such a window (empty columns) get 0 and their prior
            if (x.n_commit && (d_x || d_llr)) {
                qbp::WindowCommit C{};
                C.B = B; C.m = w->m; C.n = w->n; C.nk = x.nk; C.llr = w->d_prior_w.p + x.var_off;
                C.n_commit = x.n_commit;
                C.commit_local = w->d_commit_local.p + x.commit_off; C.commit_var = w->d_commit_var.p + x.commit_off;
                C.x = d_x; C.llr_out = d_llr;
                HIP_TRY(qbp::launch_window_commit(C, false, s));
            }
            continue;
        }
        HIP_TRY(qbp::launch_window_gather(w->d_r.p, B, w->m, w->d_checks.p + x.check_off, x.mk, w->d_syn.p, s));
        int rc = qbp_decode_batch_device(x.h, w->d_syn.p, w->d_prior_w.p + x.var_off, B, max_iter, variant, alpha, damping,
                                         clip_llr, flags & QBP_FLAG_FORCE_FULL, w->d_hard.p, w->d_conv.p, w->d_it.p,
                                         w->d_llr.p, s);
        if (rc) return rc;
        if (osd) {
            // OSD on the failures only: their list and its device-side count feed the sub-handle's ordinary launch (a
            // window's syndrome need not lie in the column space of H_k: the redo pass follows the reference there)
            HIP_TRY(qbp::launch_window_fail_list(w->d_conv.p, B, w->d_fail_list.p, w->d_fail_count.p + k, s));
            qbp::OsdParams O{};
            O.count = B; O.count_ptr = reinterpret_cast<const long long*>(w->d_fail_count.p + k); O.list = w->d_fail_list.p;
            O.syndromes = w->d_syn.p; O.llr = w->d_llr.p; O.hard = w->d_hard.p; O.solution = w->d_sol.p;
            if ((rc = osd_launch(x.h, O, B, s, true, method, order)) != QBP_OK) return rc;
        }
        qbp::WindowCommit C{};
        C.B = B; C.m = w->m; C.n = w->n; C.nk = x.nk;
        C.hard = w->d_hard.p; C.sol = osd ? w->d_sol.p : nullptr; C.conv = w->d_conv.p; C.it = w->d_it.p; C.llr = w->d_llr.p;
        C.n_upd = x.n_upd; C.n_commit = x.n_commit;
        C.upd_check = w->d_upd_check.p + x.upd_off; C.upd_ptr = w->d_upd_ptr.p + x.upd_ptr_off;
        C.upd_local = w->d_upd_local.p + x.ent_off;
        C.commit_local = w->d_commit_local.p + x.commit_off; C.commit_var = w->d_commit_var.p + x.commit_off;
        C.r = w->d_r.p; C.x = d_x; C.llr_out = d_llr; C.iters = d_iters; C.fails = d_fails; C.converged = d_converged;
        HIP_TRY(qbp::launch_window_commit(C, false, s));
    }
    if (d_converged) {
        qbp::WindowCommit C{};
        C.B = B; C.m = w->m; C.r = w->d_r.p; C.converged = d_converged;
        HIP_TRY(qbp::launch_window_commit(C, true, s));
    }
    return QBP_OK;
}

int qbp_window_decode_batch_device(qbp_window* w, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                                   int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                                   uint32_t flags, uint8_t* d_correction, uint8_t* d_converged, int32_t* d_iters,
                                   double* d_llr, int32_t* d_window_fails, void* stream)
try {
    int method = 0, order = 0;
    const int rc = window_check_call(w, B, max_iter, variant, flags, &method, &order);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_prior) return fail(QBP_E_INVALID, "null input pointer");
    if (B > (int64_t)1 << 40) return fail(QBP_E_INVALID, "B too large");
    DeviceScope on_device(w->device);
    HIP_TRY(on_device.err);
    return window_run(w, d_syndromes, d_prior, B, max_iter, variant, alpha, damping, clip_llr, flags, method, order,
                      d_correction, d_converged, d_iters, d_llr, d_window_fails, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_window_decode_batch(qbp_window* w, const uint8_t* syndromes, const double* prior, int64_t B, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                            uint8_t* correction, uint8_t* converged, int32_t* iters, double* llr, int32_t* window_fails)
try {
    int method = 0, order = 0;
    int rc = window_check_call(w, B, max_iter, variant, flags, &method, &order);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!syndromes || !prior) return fail(QBP_E_INVALID, "null input pointer");
    if (B > (int64_t)1 << 40) return fail(QBP_E_INVALID, "B too large");
    if ((rc = check_prior(w->n, prior, false)) != QBP_OK) return rc;
    DeviceScope on_device(w->device);
    HIP_TRY(on_device.err);
    const size_t b = (size_t)B, m = w->m, n = w->n;
    HostStage st(w->stream);
    const uint8_t* d_syn = st.in(w->d_in_syn, syndromes, b * m);
    const double* d_prior = st.in(w->d_in_prior, prior, n);
    uint8_t* d_x = st.out(w->d_x, correction, b * n);
    uint8_t* d_conv = st.out(w->d_conv_out, converged, b);
    int32_t* d_iters = st.out(w->d_iters, iters, b);
    double* d_llr = st.out(w->d_llr_out, llr, b * n);
    int32_t* d_fails = st.out(w->d_fails, window_fails, b);
    if (st.failed()) return st.error();
    return st.finish(window_run(w, d_syn, d_prior, B, max_iter, variant, alpha, damping, clip_llr, flags, method, order, d_x,
                                d_conv, d_iters, d_llr, d_fails, w->stream));
}
QBP_ABI_CATCH

// One Monte-Carlo call of the window decoder (device prior and counters; Lx and probs host): `d_errors` the stored
// patterns of trials trial_begin.., or null to draw them.
struct WindowMcCall {
    const uint8_t* Lx; int32_t k, distance;
    const double* probs; int32_t draws; uint64_t seed;
    const uint8_t* d_errors;
    int64_t trial_begin, trial_end;
    const double* d_prior;
    int32_t max_iter, variant; double alpha, damping, clip_llr; uint32_t flags;
    int64_t* d_counters;
};

static int window_mc_check(qbp_window* w, const WindowMcCall& c, bool stored, int* method, int* order)
{
    if (!w) return fail(QBP_E_INVALID, "null window decoder");
    if (!c.d_prior || !c.d_counters) return fail(QBP_E_INVALID, "null pointer");
    if (c.trial_begin < 0) return fail(QBP_E_INVALID, "trial_begin must be >= 0");
    if (c.trial_end < c.trial_begin) return fail(QBP_E_INVALID, "trial_end before trial_begin");
    if (c.k < 0 || c.k > 64) return fail(QBP_E_INVALID, "k = %d logical operators (need 0..64)", c.k);
    if (c.k > 0 && !c.Lx) return fail(QBP_E_INVALID, "Lx is null");
    if (stored) {
        if (!c.d_errors) return fail(QBP_E_INVALID, "errors is null");
    } else {
        if (c.draws != 1 && c.draws != 2) return fail(QBP_E_INVALID, "draws must be 1 or 2 (got %d)", c.draws);
        if (!c.probs) return fail(QBP_E_INVALID, "probs is null");
        for (int v = 0; v < w->n; ++v)
            if (!(c.probs[v] >= 0.0 && c.probs[v] <= 1.0))
                return fail(QBP_E_INVALID, "probs[%d] = %g out of [0, 1]", v, c.probs[v]);
    }
    return window_check_call(w, c.trial_end - c.trial_begin, c.max_iter, c.variant, c.flags, method, order);
}

static long long window_chunk_trials(const qbp_window* w, int64_t T)
{
    const long long dflt = std::max<long long>(1, std::min<long long>(1 << 20, ((long long)1 << 28) / (long long)w->n));
    return std::min<long long>(w->opt_chunk > 0 ? w->opt_chunk : dflt, T);
}

// A checked call on the stream, chunk by chunk: [sample,] syndrome, the window chain, classification.
static int window_mc_run(qbp_window* w, const WindowMcCall& c, int method, int order, hipStream_t s)
{
    const int64_t T = c.trial_end - c.trial_begin;
    if (T == 0) return QBP_OK;
    const size_t n = w->n, m = w->m;
    int rc = w->mc_in.prepare_lx(n, c.Lx, c.k, s);
    if (rc == QBP_OK && !c.d_errors) rc = w->mc_in.prepare_thr(n, c.probs, s);
    if (rc) return rc;
    const long long chunk = window_chunk_trials(w, T);
    if (!c.d_errors) HIP_TRY(w->d_err.reserve((size_t)chunk * n));
    HIP_TRY(w->d_in_syn.reserve((size_t)chunk * m));
    HIP_TRY(w->d_x.reserve((size_t)chunk * n));
    HIP_TRY(w->d_conv_out.reserve((size_t)chunk));
    HIP_TRY(w->d_iters.reserve((size_t)chunk));
    HIP_TRY(w->d_fails.reserve((size_t)chunk));
    for (int64_t a = c.trial_begin; a < c.trial_end; a += chunk) {
        const long long t = std::min<long long>(chunk, c.trial_end - a);
        const uint8_t* err = c.d_errors ? c.d_errors + (size_t)(a - c.trial_begin) * n : w->d_err.p;
        if (!c.d_errors) HIP_TRY(qbp::launch_mc_sample_cols(w->d_err.p, w->n, t, a, c.draws, c.seed, w->mc_in.d_thr.p, s));
        HIP_TRY(qbp::launch_window_syndrome(err, t, w->m, w->n, w->d_row_ptr.p, w->d_col_idx.p, w->d_in_syn.p, s));
        rc = window_run(w, w->d_in_syn.p, c.d_prior, t, c.max_iter, c.variant, c.alpha, c.damping, c.clip_llr,
                                  c.flags, method, order, w->d_x.p, w->d_conv_out.p, w->d_iters.p, nullptr, w->d_fails.p, s,
                                  a == c.trial_begin);
        if (rc) return rc;
        HIP_TRY(qbp::launch_window_classify(err, w->d_x.p, w->d_conv_out.p, w->d_iters.p, w->d_fails.p, t, w->n,
                                            w->mc_in.d_lx_cols.p, c.distance / 2, reinterpret_cast<long long*>(c.d_counters), s));
    }
    return QBP_OK;
}

int qbp_window_mc_run_probs_device(qbp_window* w, const uint8_t* Lx_host, int32_t k, int32_t distance,
                                   const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                                   int64_t trial_end, const double* d_prior, int32_t max_iter, int32_t variant,
                                   double alpha, double damping, double clip_llr, uint32_t flags, int64_t* d_counters,
                                   void* stream)
try {
    const WindowMcCall c{Lx_host, k, distance, probs, draws, seed, nullptr, trial_begin, trial_end, d_prior,
                         max_iter, variant, alpha, damping, clip_llr, flags, d_counters};
    int method = 0, order = 0;
    const int rc = window_mc_check(w, c, false, &method, &order);
    if (rc) return rc;
    DeviceScope on_device(w->device);
    HIP_TRY(on_device.err);
    return window_mc_run(w, c, method, order, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

// The two host-array entries: the prior (and stored errors) uploaded, counters zeroed on the device, the launches, the
// result ADDED to the caller's counters (stored errors: SET).
static int window_mc_host(qbp_window* w, WindowMcCall c, const double* prior, const uint8_t* errors, int64_t* counters)
{
    const bool stored = errors != nullptr || c.probs == nullptr;
    c.d_prior = prior; c.d_counters = counters; c.d_errors = errors;
    int method = 0, order = 0;
    int rc = window_mc_check(w, c, stored, &method, &order);
    if (rc) return rc;
    if ((rc = check_prior(w->n, prior, false)) != QBP_OK) return rc;
    if (stored) std::fill(counters, counters + QBP_NUM_COUNTERS, (int64_t)0);
    const size_t T = (size_t)(c.trial_end - c.trial_begin), n = w->n;
    if (T == 0) return QBP_OK;
    DeviceScope on_device(w->device);
    HIP_TRY(on_device.err);
    HostStage st(w->stream);
    c.d_prior = st.in(w->d_in_prior, prior, n);
    long long* d_cnt = st.zeroed(w->d_counters, QBP_NUM_COUNTERS);
    st.add(counters, d_cnt, QBP_NUM_COUNTERS);
    c.d_counters = reinterpret_cast<int64_t*>(d_cnt);
    if (stored) c.d_errors = st.in(w->d_err, errors, T * n);
    if (st.failed()) return st.error();
    return st.finish(window_mc_run(w, c, method, order, w->stream));
}

int qbp_window_mc_run_probs(qbp_window* w, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                            int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* prior,
                            int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                            uint32_t flags, int64_t counters[QBP_NUM_COUNTERS])
try {
    if (!probs) return fail(QBP_E_INVALID, "probs is null");
    return window_mc_host(w, WindowMcCall{Lx, k, distance, probs, draws, seed, nullptr, trial_begin, trial_end, nullptr,
                                          max_iter, variant, alpha, damping, clip_llr, flags, nullptr},
                          prior, nullptr, counters);
}
QBP_ABI_CATCH

int qbp_window_mc_run_errors(qbp_window* w, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                             int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                             double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS])
try {
    if (T < 0) return fail(QBP_E_INVALID, "T must be >= 0");
    return window_mc_host(w, WindowMcCall{Lx, k, distance, nullptr, 1, 0, nullptr, 0, T, nullptr, max_iter, variant,
                                          alpha, damping, clip_llr, flags, nullptr},
                          prior, errors, counters);
}
QBP_ABI_CATCH

int64_t qbp_window_get_info(qbp_window* w, int32_t what, int32_t index)
try {
    if (!w) return -1;
    if (what == QBP_WINDOW_INFO_WINDOWS) return w->plan.K;
    if (what == QBP_WINDOW_INFO_CLASSES) return (int64_t)w->sub.size();
    if (what == QBP_WINDOW_INFO_ROUNDS) return w->plan.R;
    if (index < 0 || index >= (int32_t)w->sub.size()) return -1;
    return qbp_get_info(w->sub[index], what);
}
catch (...) { return -1; }

int qbp_window_set_option(qbp_window* w, int32_t option, int64_t value)
try {
    if (!w) return fail(QBP_E_INVALID, "null window decoder");
    if (option == QBP_OPT_MC_WEIGHT_CHUNK) {
        if (value < 0 || value > (1 << 20)) return fail(QBP_E_INVALID, "trials per chunk out of [0, 2^20]");
        w->opt_chunk = value;
        return QBP_OK;
    }
    for (qbp_handle* h : w->sub) {
        const int rc = qbp_set_option(h, option, value);
        if (rc) return rc;
    }
    return QBP_OK;
}
QBP_ABI_CATCH

// ---- BP with a prior per record (qbp_cond.hpp) -------------------------------------------------------------------
// Everything qbp_decode_batch_cond refuses apart from null pointers and NaN priors: host only, before any GPU work.
static int cond_check(qbp_handle* h, long long B, int max_iter, int variant, uint32_t flags)
{
    const int rc = check_decode_args(h, B, max_iter, variant);
    if (rc) return rc;
    if (flags & (QBP_FLAG_OSD0 | OSD_ALL_BITS)) return fail(QBP_E_INVALID, "flags 0x%x: an OSD bit in a BP call", flags);
    if (variant == QBP_DAMPED_SP)
        return fail(QBP_E_UNSUPPORTED, "BP with a prior per record runs QBP_SUM_PRODUCT or QBP_MIN_SUM, not QBP_DAMPED_SP");
    if (flags & (QBP_FLAG_PAIRWISE_COLSUM | QBP_FLAG_DENSE_F_COLSUM | QBP_FLAG_DENSE_F_COLSUM_ITER0 | QBP_FLAG_LAYERED |
                 QBP_FLAG_FAST_MATH | SECOND_BP_BITS | QBP_FLAG_QUANT))
        return fail(QBP_E_UNSUPPORTED, "flags 0x%x: BP with a prior per record has the flooding schedule, ascending column "
                                       "sums and numpy's functions only, and no second stage", flags);
    if (flags & ~(uint32_t)QBP_FLAG_FORCE_FULL) return fail(QBP_E_INVALID, "flags 0x%x: unknown bits", flags);
    const size_t lds = qbp::cond_lds_bytes(h->m, h->n, h->E, variant == QBP_SUM_PRODUCT);
    if (lds > (size_t)160 * 1024)
        return fail(QBP_E_UNSUPPORTED, "BP with a prior per record keeps the messages and two rows of n doubles in LDS: "
                                       "%d x %d with %d entries needs %zu B (limit 160 KiB)", h->m, h->n, h->E, lds);
    return QBP_OK;
}

static int cond_launch(qbp_handle* h, const RecordCall& c, const uint8_t* d_sel, const double* d_prior1, int max_iter,
                       int variant, double alpha, double clip_llr, hipStream_t s)
{
    constexpr int RC = qbp::GENERIC_MAX_ROW_CLASS, CC = qbp::GENERIC_MAX_COL_CLASS;
    const bool sp = variant == QBP_SUM_PRODUCT;
    const size_t lds = qbp::cond_lds_bytes(h->m, h->n, h->E, sp);
    const int threads = qbp::record_threads(h->rpad_off[RC + 1], h->cpad_off[CC + 1], qbp::COND_MAX_THREADS);
    qbp::CondParams P{};
    int grid = 0;
    // the wavefronts a CU holds at the kernel's registers, as bp_gd_kernel: min-sum 7 per SIMD, sum-product 5;
    // QBP_OPT_BLOCKS_PER_CU overrides
    const int rc = record_launch_setup(h, c, false, {"BP with a prior per record", lds, threads, sp ? 20 : 28, true}, s,
                                       P.tab, P.io, &grid);
    if (rc) return rc;
    HIP_TRY(h->d_prior1_sorted.reserve((size_t)h->n));
    HIP_TRY(qbp::launch_permute_prior(d_prior1, h->d_svar.p, h->d_prior1_sorted.p, h->n, s));
    P.sel = d_sel; P.prior1_sorted = h->d_prior1_sorted.p;
    P.max_iter = max_iter; P.alpha = alpha; P.clip_llr = clip_llr;
    HIP_TRY(qbp::launch_cond(variant, P, grid, threads, lds, s));
    return QBP_OK;
}

int qbp_decode_batch_cond_device(qbp_handle* h, const uint8_t* d_syndromes, const uint8_t* d_sel, const double* d_prior0,
                                 const double* d_prior1, int64_t B, int32_t max_iter, int32_t variant, double alpha,
                                 double clip_llr, uint32_t flags, uint8_t* d_hard, uint8_t* d_converged, int32_t* d_iters,
                                 double* d_llr, void* stream)
try {
    const int rc = cond_check(h, B, max_iter, variant, flags);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!d_syndromes || !d_sel || !d_prior0 || !d_prior1) return fail(QBP_E_INVALID, "null input pointer");
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    RecordCall c;
    c.prior = d_prior0; c.max_items = B; c.syndromes = d_syndromes;
    c.hard = d_hard; c.converged = d_converged; c.iters = d_iters; c.llr = d_llr;
    return cond_launch(h, c, d_sel, d_prior1, max_iter, variant, alpha, clip_llr, static_cast<hipStream_t>(stream));
}
QBP_ABI_CATCH

int qbp_decode_batch_cond(qbp_handle* h, const uint8_t* syndromes, const uint8_t* sel, const double* prior0,
                          const double* prior1, int64_t B, int32_t max_iter, int32_t variant, double alpha,
                          double clip_llr, uint32_t flags, uint8_t* hard, uint8_t* converged, int32_t* iters, double* llr)
try {
    int rc = cond_check(h, B, max_iter, variant, flags);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!syndromes || !sel || !prior0 || !prior1) return fail(QBP_E_INVALID, "null input pointer");
    if ((rc = check_prior(h->n, prior0, false)) != QBP_OK || (rc = check_prior(h->n, prior1, false)) != QBP_OK) return rc;
    DeviceScope on_device(h->device);
    HIP_TRY(on_device.err);
    const size_t m = h->m, n = h->n, b = (size_t)B;
    HostStage st(h->stream);
    const uint8_t* d_syn = st.in(h->d_syn, syndromes, b * m);
    const uint8_t* d_sel = st.in(h->d_cond_sel, sel, b * n);
    const double* d_p0 = st.in(h->d_prior, prior0, n);
    const double* d_p1 = st.in(h->d_cond_prior1, prior1, n);
    uint8_t* d_hard = st.out(h->d_hard, hard, b * n);
    uint8_t* d_conv = st.out(h->d_conv, converged, b);
    int32_t* d_iters = st.out(h->d_iters, iters, b);
    double* d_llr = st.out(h->d_llr, llr, b * n);
    if (st.failed()) return st.error();
    return st.finish(qbp_decode_batch_cond_device(h, d_syn, d_sel, d_p0, d_p1, B, max_iter, variant, alpha, clip_llr, flags,
                                                  d_hard, d_conv, d_iters, d_llr, h->stream));
}
QBP_ABI_CATCH

// ---- Two-stage decoding of a CSS code under Pauli noise (include/qbp.h, qbp_css_*) ---------------------------------
struct qbp_css {
    qbp_handle* ha = nullptr;       // borrowed
    qbp_handle* hb = nullptr;
    int device = 0, n = 0;
    hipStream_t stream = nullptr;
    // one chunk: errors, syndromes, a stage's BP outputs and OSD solutions, the corrections, the failure list
    DevBuf<uint8_t> d_ea, d_eb, d_syn_a, d_syn_b, d_hard, d_sol, d_conv_a, d_conv_b, d_xa, d_xb;
    DevBuf<int32_t> d_it_a, d_it_b;
    DevBuf<double> d_llr, d_prior_a, d_prior_b0, d_prior_b1;
    DevBuf<long long> d_fail_list, d_counters;
    DevBuf<unsigned long long> d_fail_count;    // [2]: one per stage
    McInputs in_a, in_b;                        // the logical operators of the sectors, by column
    long long opt_chunk = 0;
};

// One call of the chain: what every entry shares
struct CssCall {
    const double* prior_a; const double* prior_b0; const double* prior_b1;      // device
    int32_t max_iter, variant; double alpha, damping, clip_llr; uint32_t flags;
    int method, order;              // parse_osd_flags
};

// Everything a CSS call refuses apart from null pointers and NaN priors: host only, before any GPU work.
static int css_check(qbp_css* css, int64_t B, int32_t max_iter, int32_t variant, uint32_t flags, int* method, int* order)
{
    if (!css) return fail(QBP_E_INVALID, "null CSS decoder");
    if (flags & (QBP_FLAG_LAYERED | SECOND_BP_BITS | QBP_FLAG_QUANT))
        return fail(QBP_E_UNSUPPORTED, "flags 0x%x: Relay-BP, BP guided decimation, LSD, the layered schedule and "
                                       "fixed-point BP are not available as a stage of the CSS decoder", flags);
    int rc = cond_check(css->hb, B, max_iter, variant, flags & ~(QBP_FLAG_OSD0 | OSD_ALL_BITS));
    if (rc) return rc;
    // (what stage A's qbp_decode_batch_device would refuse: its argument check -- it has none for alpha, damping or the
    // clip -- and, below, its choice of kernel)
    if ((rc = check_decode_args(css->ha, B, max_iter, variant)) != QBP_OK) return rc;
    for (qbp_handle* h : {css->ha, css->hb}) {
        if ((rc = parse_osd_flags(h, flags & ~(uint32_t)QBP_FLAG_FORCE_FULL, true, method, order)) != QBP_OK) return rc;
        if (bp_kernel(h, B, 0, 0, false) < 0) return fail(QBP_E_UNSUPPORTED, "a sector's matrix does not fit the forced kernel");
    }
    return QBP_OK;
}

// One stage on B records (device pointers): BP through `decode` into hard / conv / it / llr; with OSD the solutions of
// the unconverged records, and x = solution there, hard elsewhere.  Without OSD, BP writes x itself.
extern "C++" {       // (a template: not in the C linkage of the entry points around it)
template <class Decode>
static int css_stage(qbp_css* css, qbp_handle* h, int stage, const uint8_t* d_syn, long long B, const CssCall& c,
                     uint8_t* d_x, uint8_t* d_conv, int32_t* d_it, hipStream_t s, bool redo, const Decode& decode)
{
    const bool osd = (c.flags & (QBP_FLAG_OSD0 | OSD_METHOD_BITS)) != 0;
    int rc = decode(osd ? css->d_hard.p : d_x, d_conv, d_it, osd ? css->d_llr.p : nullptr);
    if (rc || !osd) return rc;
    unsigned long long* const count = css->d_fail_count.p + stage;
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
    HIP_TRY(qbp::launch_window_fail_list(d_conv, B, css->d_fail_list.p, count, s));
    qbp::OsdParams O{};
    O.count = B; O.count_ptr = reinterpret_cast<const long long*>(count); O.list = css->d_fail_list.p;
    O.syndromes = d_syn; O.llr = css->d_llr.p; O.hard = css->d_hard.p; O.solution = css->d_sol.p;
    // (redo: a caller's syndrome need not lie in the column space of the matrix; a Monte-Carlo syndrome is H e)
    if ((rc = osd_launch(h, O, B, s, redo, c.method, c.order)) != QBP_OK) return rc;
    HIP_TRY(qbp::launch_css_select(css->d_hard.p, css->d_sol.p, d_conv, B, css->n, d_x, s));
    return QBP_OK;
}
}  // extern "C++"

static int css_reserve(qbp_css* css, size_t b, bool osd)
{
    const size_t n = css->n;
    HIP_TRY(css->d_xa.reserve(b * n));
    HIP_TRY(css->d_xb.reserve(b * n));
    HIP_TRY(css->d_conv_a.reserve(b));
    HIP_TRY(css->d_conv_b.reserve(b));
    HIP_TRY(css->d_it_a.reserve(b));
    HIP_TRY(css->d_it_b.reserve(b));
    if (osd) {
        HIP_TRY(css->d_hard.reserve(b * n));
        HIP_TRY(css->d_sol.reserve(b * n));
        HIP_TRY(css->d_llr.reserve(b * n));
        HIP_TRY(css->d_fail_list.reserve(b));
        HIP_TRY(css->d_fail_count.reserve(2));
    }
    return QBP_OK;
}

// Both stages on B records, buffers reserved: x_a, x_b, conv and iterations of both BP stages (device, none null).
// from_errors: the syndromes are H e (the Monte-Carlo entries), so OSD needs no redo pass.
static int css_run(qbp_css* css, const uint8_t* d_syn_a, const uint8_t* d_syn_b, long long B, const CssCall& c,
                   uint8_t* d_xa, uint8_t* d_xb, uint8_t* d_conv_a, uint8_t* d_conv_b, int32_t* d_it_a, int32_t* d_it_b,
                   bool from_errors, hipStream_t s)
{
    const uint32_t bp_flags = c.flags & QBP_FLAG_FORCE_FULL;
    int rc = css_stage(css, css->ha, 0, d_syn_a, B, c, d_xa, d_conv_a, d_it_a, s, !from_errors,
                       [&](uint8_t* hard, uint8_t* conv, int32_t* it, double* llr) {
                           return qbp_decode_batch_device(css->ha, d_syn_a, c.prior_a, B, c.max_iter, c.variant, c.alpha,
                                                          c.damping, c.clip_llr, bp_flags, hard, conv, it, llr, s);
                       });
    if (rc) return rc;
    return css_stage(css, css->hb, 1, d_syn_b, B, c, d_xb, d_conv_b, d_it_b, s, !from_errors,
                     [&](uint8_t* hard, uint8_t* conv, int32_t* it, double* llr) {
                         return qbp_decode_batch_cond_device(css->hb, d_syn_b, d_xa, c.prior_b0, c.prior_b1, B, c.max_iter,
                                                             c.variant, c.alpha, c.clip_llr, bp_flags, hard, conv, it, llr,
                                                             s);
                     });
}

void qbp_css_destroy(qbp_css* css)
try {
    if (!css) return;
    DeviceScope on_device(css->device);
    if (css->stream) (void)hipStreamDestroy(css->stream);
    delete css;
}
catch (...) {
}

int qbp_css_create(qbp_handle* ha, qbp_handle* hb, qbp_css** out)
try {
    if (!out) return fail(QBP_E_INVALID, "out is null");
    *out = nullptr;
    if (!ha || !hb) return fail(QBP_E_INVALID, "null handle");
    if (ha->device != hb->device)
        return fail(QBP_E_INVALID, "the two handles are on devices %d and %d", ha->device, hb->device);
    if (ha->n != hb->n) return fail(QBP_E_INVALID, "the two matrices have %d and %d columns", ha->n, hb->n);
    struct Guard {
        qbp_css* c;
        ~Guard() { if (c) qbp_css_destroy(c); }
    } guard{new qbp_css()};
    qbp_css* css = guard.c;
    css->ha = ha; css->hb = hb; css->device = ha->device; css->n = ha->n;
    DeviceScope on_device(css->device);
    HIP_TRY(on_device.err);
    HIP_TRY(hipStreamCreateWithFlags(&css->stream, hipStreamNonBlocking));
    guard.c = nullptr;
    *out = css;
    return QBP_OK;
}
QBP_ABI_CATCH

int qbp_css_set_option(qbp_css* css, int32_t option, int64_t value)
try {
    if (!css) return fail(QBP_E_INVALID, "null CSS decoder");
    if (option != QBP_OPT_MC_WEIGHT_CHUNK) return fail(QBP_E_INVALID, "unknown option %d", option);
    if (value < 0 || value > QBP_MC_OSD_MAX_TRIALS) return fail(QBP_E_INVALID, "trials per chunk out of [0, 2^20]");
    css->opt_chunk = value;
    return QBP_OK;
}
QBP_ABI_CATCH

// The sampler's cumulative thresholds (include/qbp.h): Z, X, Y
static int css_thresholds(double px, double py, double pz, unsigned thr[3])
{
    for (double p : {px, py, pz})
        if (!(p >= 0.0 && p <= 1.0)) return fail(QBP_E_INVALID, "Pauli probability %g out of [0, 1]", p);
    if (!((pz + px) + py <= 1.0)) return fail(QBP_E_INVALID, "px + py + pz = %g exceeds 1", (pz + px) + py);
    thr[0] = mc_threshold(pz); thr[1] = mc_threshold(pz + px); thr[2] = mc_threshold((pz + px) + py);
    return QBP_OK;
}

int qbp_css_sample_errors(qbp_css* css, double px, double py, double pz, uint64_t seed, int64_t trial_begin, int64_t T,
                          uint8_t* errors_a, uint8_t* errors_b)
try {
    if (!css) return fail(QBP_E_INVALID, "null CSS decoder");
    unsigned thr[3];
    const int rc = css_thresholds(px, py, pz, thr);
    if (rc) return rc;
    if (trial_begin < 0 || T < 0) return fail(QBP_E_INVALID, "trial_begin and T must be >= 0");
    if (T == 0) return QBP_OK;
    if (!errors_a || !errors_b) return fail(QBP_E_INVALID, "null output pointer");
    DeviceScope on_device(css->device);
    HIP_TRY(on_device.err);
    const size_t n = css->n;
    const long long chunk = std::min<long long>(T, std::max<long long>(1, ((long long)1 << 28) / (long long)n));
    HIP_TRY(css->d_ea.reserve((size_t)chunk * n));
    HIP_TRY(css->d_eb.reserve((size_t)chunk * n));
    for (int64_t a = 0; a < T; a += chunk) {
        const long long t = std::min<long long>(chunk, T - a);
        HIP_TRY(qbp::launch_css_sample_pauli(css->d_ea.p, css->d_eb.p, css->n, t, trial_begin + a, seed, thr[0], thr[1],
                                             thr[2], css->stream));
        HIP_TRY(hipMemcpyAsync(errors_a + (size_t)a * n, css->d_ea.p, (size_t)t * n, hipMemcpyDeviceToHost, css->stream));
        HIP_TRY(hipMemcpyAsync(errors_b + (size_t)a * n, css->d_eb.p, (size_t)t * n, hipMemcpyDeviceToHost, css->stream));
        HIP_TRY(hipStreamSynchronize(css->stream));
    }
    return QBP_OK;
}
QBP_ABI_CATCH

// The three priors of a host entry: none null, none NaN
static int css_check_priors(const qbp_css* css, const double* prior_a, const double* prior_b0, const double* prior_b1)
{
    if (!prior_a || !prior_b0 || !prior_b1) return fail(QBP_E_INVALID, "null prior");
    for (const double* p : {prior_a, prior_b0, prior_b1}) {
        const int rc = check_prior(css->n, p, false);
        if (rc) return rc;
    }
    return QBP_OK;
}

int qbp_css_decode_batch(qbp_css* css, const uint8_t* syn_a, const uint8_t* syn_b, int64_t B, const double* prior_a,
                         const double* prior_b0, const double* prior_b1, int32_t max_iter, int32_t variant, double alpha,
                         double damping, double clip_llr, uint32_t flags, uint8_t* x_a, uint8_t* x_b, uint8_t* conv_a,
                         uint8_t* conv_b)
try {
    CssCall c{nullptr, nullptr, nullptr, max_iter, variant, alpha, damping, clip_llr, flags, 0, 0};
    int rc = css_check(css, B, max_iter, variant, flags, &c.method, &c.order);
    if (rc) return rc;
    if (B == 0) return QBP_OK;
    if (!syn_a || !syn_b) return fail(QBP_E_INVALID, "null input pointer");
    if ((rc = css_check_priors(css, prior_a, prior_b0, prior_b1)) != QBP_OK) return rc;
    if (B > QBP_MC_OSD_MAX_TRIALS)
        return fail(QBP_E_UNSUPPORTED, "qbp_css_decode_batch takes at most %d records per call", QBP_MC_OSD_MAX_TRIALS);
    DeviceScope on_device(css->device);
    HIP_TRY(on_device.err);
    const size_t n = css->n, b = (size_t)B;
    const bool osd = (flags & (QBP_FLAG_OSD0 | OSD_METHOD_BITS)) != 0;
    if ((rc = css_reserve(css, b, osd)) != QBP_OK) return rc;
    HostStage st(css->stream);
    const uint8_t* d_sa = st.in(css->d_syn_a, syn_a, b * css->ha->m);
    const uint8_t* d_sb = st.in(css->d_syn_b, syn_b, b * css->hb->m);
    c.prior_a = st.in(css->d_prior_a, prior_a, n);
    c.prior_b0 = st.in(css->d_prior_b0, prior_b0, n);
    c.prior_b1 = st.in(css->d_prior_b1, prior_b1, n);
    // (x_a is stage B's input whether the caller wants it or not: the outputs are the chunk buffers)
    st.out(css->d_xa, x_a, b * n);
    st.out(css->d_xb, x_b, b * n);
    st.out(css->d_conv_a, conv_a, b);
    st.out(css->d_conv_b, conv_b, b);
    if (st.failed()) return st.error();
    return st.finish(css_run(css, d_sa, d_sb, B, c, css->d_xa.p, css->d_xb.p, css->d_conv_a.p, css->d_conv_b.p,
                             css->d_it_a.p, css->d_it_b.p, false, css->stream));
}
QBP_ABI_CATCH

// The Monte-Carlo entries after their checks: chunk by chunk [sample,] syndromes, the two stages, classification.
// d_ea / d_eb: the stored errors of all T trials (device), or null to draw them with thr.
static int css_mc_run(qbp_css* css, const CssCall& c, const uint8_t* d_ea, const uint8_t* d_eb, const unsigned* thr,
                      uint64_t seed, int64_t trial_begin, int64_t T, int32_t distance, long long* d_counters, hipStream_t s)
{
    const size_t n = css->n, ma = css->ha->m, mb = css->hb->m;
    const bool osd = (c.flags & (QBP_FLAG_OSD0 | OSD_METHOD_BITS)) != 0;
    const long long dflt = std::max<long long>(1, std::min<long long>(QBP_MC_OSD_MAX_TRIALS, ((long long)1 << 28) / (long long)n));
    const long long chunk = std::min<long long>(css->opt_chunk > 0 ? css->opt_chunk : dflt, T);
    int rc = css_reserve(css, (size_t)chunk, osd);
    if (rc) return rc;
    if (!d_ea) {
        HIP_TRY(css->d_ea.reserve((size_t)chunk * n));
        HIP_TRY(css->d_eb.reserve((size_t)chunk * n));
    }
    HIP_TRY(css->d_syn_a.reserve((size_t)chunk * ma));
    HIP_TRY(css->d_syn_b.reserve((size_t)chunk * mb));
    for (int64_t a = 0; a < T; a += chunk) {
        const long long t = std::min<long long>(chunk, T - a);
        const uint8_t* ea = d_ea ? d_ea + (size_t)a * n : css->d_ea.p;
        const uint8_t* eb = d_eb ? d_eb + (size_t)a * n : css->d_eb.p;
        if (!d_ea)
            HIP_TRY(qbp::launch_css_sample_pauli(css->d_ea.p, css->d_eb.p, css->n, t, trial_begin + a, seed, thr[0], thr[1],
                                                 thr[2], s));
        HIP_TRY(qbp::launch_window_syndrome(ea, t, (int)ma, css->n, css->ha->d_row_ptr.p, css->ha->d_col_idx.p,
                                            css->d_syn_a.p, s));
        HIP_TRY(qbp::launch_window_syndrome(eb, t, (int)mb, css->n, css->hb->d_row_ptr.p, css->hb->d_col_idx.p,
                                            css->d_syn_b.p, s));
        rc = css_run(css, css->d_syn_a.p, css->d_syn_b.p, t, c, css->d_xa.p, css->d_xb.p, css->d_conv_a.p, css->d_conv_b.p,
                     css->d_it_a.p, css->d_it_b.p, true, s);
        if (rc) return rc;
        qbp::CssClassify K{};
        K.T = t; K.n = css->n; K.ma = (int)ma; K.mb = (int)mb;
        K.e_a = ea; K.x_a = css->d_xa.p; K.e_b = eb; K.x_b = css->d_xb.p;
        K.conv_a = css->d_conv_a.p; K.conv_b = css->d_conv_b.p; K.it_a = css->d_it_a.p; K.it_b = css->d_it_b.p;
        K.row_ptr_a = css->ha->d_row_ptr.p; K.col_idx_a = css->ha->d_col_idx.p;
        K.row_ptr_b = css->hb->d_row_ptr.p; K.col_idx_b = css->hb->d_col_idx.p;
        K.l_a = css->in_a.d_lx_cols.p; K.l_b = css->in_b.d_lx_cols.p;
        K.half_distance = distance / 2; K.counters = d_counters;
        HIP_TRY(qbp::launch_css_classify(K, s));
    }
    return QBP_OK;
}

// Both Monte-Carlo host entries: errors_a null draws the errors.
static int css_mc_host(qbp_css* css, const uint8_t* La, int32_t ka, const uint8_t* Lb, int32_t kb, int32_t distance,
                       const uint8_t* errors_a, const uint8_t* errors_b, const unsigned* thr, uint64_t seed,
                       int64_t trial_begin, int64_t T, const double* prior_a, const double* prior_b0,
                       const double* prior_b1, CssCall c, int64_t* counters)
{
    int rc = css_check(css, T, c.max_iter, c.variant, c.flags, &c.method, &c.order);
    if (rc) return rc;
    if (!counters) return fail(QBP_E_INVALID, "counters is null");
    for (int32_t k : {ka, kb})
        if (k < 0 || k > 64) return fail(QBP_E_INVALID, "k = %d logical operators (need 0..64)", k);
    if ((ka > 0 && !La) || (kb > 0 && !Lb)) return fail(QBP_E_INVALID, "null logical operators");
    if ((rc = css_check_priors(css, prior_a, prior_b0, prior_b1)) != QBP_OK) return rc;
    const bool stored = thr == nullptr;
    if (stored && T > 0 && (!errors_a || !errors_b)) return fail(QBP_E_INVALID, "errors is null");
    if (stored) std::fill(counters, counters + 3 * QBP_NUM_COUNTERS, (int64_t)0);
    if (T == 0) return QBP_OK;
    DeviceScope on_device(css->device);
    HIP_TRY(on_device.err);
    const size_t n = css->n;
    hipStream_t s = css->stream;
    if ((rc = css->in_a.prepare_lx(n, La, ka, s)) != QBP_OK || (rc = css->in_b.prepare_lx(n, Lb, kb, s)) != QBP_OK) return rc;
    HostStage st(s);
    c.prior_a = st.in(css->d_prior_a, prior_a, n);
    c.prior_b0 = st.in(css->d_prior_b0, prior_b0, n);
    c.prior_b1 = st.in(css->d_prior_b1, prior_b1, n);
    long long* d_cnt = st.zeroed(css->d_counters, 3 * QBP_NUM_COUNTERS);
    st.add(counters, d_cnt, 3 * QBP_NUM_COUNTERS);
    const uint8_t* d_ea = stored ? st.in(css->d_ea, errors_a, (size_t)T * n) : nullptr;
    const uint8_t* d_eb = stored ? st.in(css->d_eb, errors_b, (size_t)T * n) : nullptr;
    if (st.failed()) return st.error();
    return st.finish(css_mc_run(css, c, d_ea, d_eb, thr, seed, trial_begin, T, distance, d_cnt, s));
}

int qbp_css_mc_run(qbp_css* css, const uint8_t* La, int32_t ka, const uint8_t* Lb, int32_t kb, int32_t distance,
                   double px, double py, double pz, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                   const double* prior_a, const double* prior_b0, const double* prior_b1, int32_t max_iter,
                   int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                   int64_t counters[3 * QBP_NUM_COUNTERS])
try {
    unsigned thr[3];
    const int rc = css_thresholds(px, py, pz, thr);
    if (rc) return rc;
    if (trial_begin < 0) return fail(QBP_E_INVALID, "trial_begin must be >= 0");
    if (trial_end < trial_begin) return fail(QBP_E_INVALID, "trial_end before trial_begin");
    return css_mc_host(css, La, ka, Lb, kb, distance, nullptr, nullptr, thr, seed, trial_begin, trial_end - trial_begin,
                       prior_a, prior_b0, prior_b1,
                       CssCall{nullptr, nullptr, nullptr, max_iter, variant, alpha, damping, clip_llr, flags, 0, 0}, counters);
}
QBP_ABI_CATCH

int qbp_css_mc_run_errors(qbp_css* css, const uint8_t* La, int32_t ka, const uint8_t* Lb, int32_t kb, int32_t distance,
                          const uint8_t* errors_a, const uint8_t* errors_b, int64_t T, const double* prior_a,
                          const double* prior_b0, const double* prior_b1, int32_t max_iter, int32_t variant, double alpha,
                          double damping, double clip_llr, uint32_t flags, int64_t counters[3 * QBP_NUM_COUNTERS])
try {
    if (T < 0) return fail(QBP_E_INVALID, "T must be >= 0");
    return css_mc_host(css, La, ka, Lb, kb, distance, errors_a, errors_b, nullptr, 0, 0, T, prior_a, prior_b0, prior_b1,
                       CssCall{nullptr, nullptr, nullptr, max_iter, variant, alpha, damping, clip_llr, flags, 0, 0}, counters);
}
QBP_ABI_CATCH


}  // extern "C"
