// BP with a prior chosen per record (include/qbp.h, qbp_decode_batch_cond), and the glue kernels of the two-stage
// decoder of a CSS code under Pauli noise (qbp_css_*).
//
// bp_cond_kernel is bp_gd_kernel's frame without the decimation and the arg-max: one workgroup per record, the per-record
// BP iteration of qbp_record_bp.hpp (the tables of the general-H kernel, the messages in place in LDS) with two workgroup
// barriers per iteration:
//   check step     min-sum: record_check_step_minsum; sum-product: record_check_step_sumproduct, the exact row on
//                  numpy's tanh / arctanh tables (as a function it costs this kernel 92 registers instead of 89 in its
//                  body: 5 wavefronts per SIMD either way);
//   -- barrier A --
//   variable step  record_variable_step with bias = W, the record's prior: V = colsum(R) + W (ascending check),
//                  Q = V - R in place, and the incremental syndrome test;
//   -- barrier B --
//   counter zero <=> H hard == s: the record is done.
// What is its own is the record start: the prior of the sorted variable x is one of two tables, chosen by the record's
// selector byte of that variable,
//   W[x] = (sel[rec * n + svar[x]] & 1) ? prior1_sorted[x] : prior0_sorted[x],     V = W,
// then a barrier -- the fill walks the variables thread by thread, record_prior_to_edges by weight class -- and Q = W on
// the edges.  With sel == 0 this is qbp_decode_batch on prior0, with sel == 1 on prior1, bit for bit.
// Min-sum is rework/decoding.py's rule at damping = 1: Q = clip(1.0 * (V - R) + 0.0 * Q_old).  The second term is a
// zero unless Q_old is infinite or NaN, and then the message is NaN from there on.  The slot of Q_old holds R by then,
// so a byte per edge remembers it (`stuck`: set at the record start from the prior on the edge, behind a barrier of
// its own because the first check step overwrites those slots, and by every update whose result is not finite).  Q_new itself is never -0.0 (V - R = -0.0 needs V = -0.0 and R = +0.0, and R is one of
// V's summands), so adding the zero changes no other bit.
// Per-record state, all in LDS: the E messages, V[n], W[n] (both in sorted-variable order), the syndrome and parity bits,
// min-sum: the stuck bytes; sum-product: numpy's function tables at LDS address 0.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_record_bp.hpp"

namespace qbp {

constexpr int COND_MAX_THREADS = 512;

struct CondParams {
    RecordTables tab;               // tab.prior_sorted: prior0 in sorted-variable order
    RecordIo io;                    // the batch half only
    const uint8_t* sel;             // [B][n] bit 0: the record takes prior1 for that variable (original variable order)
    const double* prior1_sorted;    // [n]
    int max_iter;
    double alpha, clip_llr;
};

// 32-bit words behind the doubles: the head (RecordLds: logical mask (2), error weight, difference flag, unsatisfied
// checks [2], next record, pad), syndrome bits [mw], parity bits [2][mw]; min-sum: a byte per edge behind them
constexpr int COND_HEAD_WORDS = 8;
__host__ __device__ inline size_t cond_lds_words(int m, int E, bool stuck)
{
    const size_t mw = ((size_t)m + 31) >> 5;
    return ((size_t)COND_HEAD_WORDS + 3 * mw + (stuck ? ((size_t)E + 3) >> 2 : 0) + 1) & ~(size_t)1;
}
// Dynamic LDS of one workgroup: (sum-product) the function tables, E messages, V and W [n] each, the words
__host__ __device__ inline size_t cond_lds_bytes(int m, int n, int E, bool tables)
{
    return (tables ? (size_t)NP_LDS_BYTES : 0) + (size_t)8 * ((size_t)E + 2 * (size_t)n) + 4 * cond_lds_words(m, E, !tables);
}

template <int VARIANT>
__global__ __launch_bounds__(COND_MAX_THREADS) void bp_cond_kernel(const CondParams P)
{
    static_assert(VARIANT == 0 || VARIANT == 2, "sum-product or min-sum");
    extern __shared__ __attribute__((aligned(16))) double cond_smem[];
    constexpr int TAB = VARIANT == 0 ? NP_LDS_DOUBLES : 0;      // (the function tables: RECORD_NP_TAB)
    constexpr int RC = GENERIC_MAX_ROW_CLASS;
    const RecordTables& G = P.tab;
    const RecordIo& io = P.io;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = G.m, n = G.n, E = G.E;
    double* const M = cond_smem + TAB;              // [E] messages, in place
    double* const V = M + E;                        // [n] posterior values, sorted-variable order
    double* const Wp = V + n;                       // [n] the record's prior, sorted-variable order
    unsigned* const words = reinterpret_cast<unsigned*>(Wp + n);
    const int mw = (m + 31) >> 5;
    const RecordLds S{M, V, reinterpret_cast<unsigned long long*>(words), reinterpret_cast<int*>(words + 2),
                      reinterpret_cast<int*>(words + 3), reinterpret_cast<int*>(words + 4), words + 6,
                      words + COND_HEAD_WORDS, words + COND_HEAD_WORDS + mw};
    uint8_t* const stuck = reinterpret_cast<uint8_t*>(S.par + 2 * mw);      // [E] min-sum only

    const int first_long = G.row_off[RC + 1], n_long = G.row_off[RC + 2] - first_long;
    const int lbase = G.row_base[RC + 1], n_ledges = E - lbase;
    double* const Lw = G.wsL + (size_t)blockIdx.x * 3 * (n_long > 0 ? n_long : 1);

    if constexpr (VARIANT == 0) np_tables_to_lds(cond_smem, tid, nt);   // (published by the record's first barrier)
    const long long count = record_count<false>(io, S);
    const bool dynamic = count > (long long)gridDim.x;

    for (long long item = blockIdx.x; item < count;) {
        const long long rec = record_load_syndrome<false>(G, io, S, item);
        // ---- the record's prior: W = V = prior1 where the selector has bit 0, else prior0 ---------------------------
        {
            const uint8_t* const sel = P.sel + rec * n;
            for (int x = tid; x < n; x += nt) {
                const double pv = (sel[G.svar[x]] & 1u) ? P.prior1_sorted[x] : G.prior_sorted[x];
                Wp[x] = pv; V[x] = pv;
            }
        }
        __syncthreads();      // (the edge write below takes its variables by weight class, not thread by thread)
        record_prior_to_edges(G, S, Wp);
        __syncthreads();
        const int syn_weight = S.unsat[0];    // unsatisfied checks of the all-zero candidate
        if constexpr (VARIANT == 2) {
            for (int o = tid; o < E; o += nt) {
                const double q = M[o];
                stuck[o] = (uint8_t)((q - q == 0.0) ? 0 : 1);
            }
            __syncthreads();      // (the check step overwrites M in place, its edges dealt to the threads by row class)
        }

        int total = 0;
        bool solved = false;
        for (int t = 0; t < P.max_iter && !solved; ++t) {
            // ================= check step ==========================================================================
            if constexpr (VARIANT == 2) {
                record_check_step_minsum(G, S, Lw, P.alpha);
            } else {
                record_check_step_sumproduct(G, S, Lw, P.alpha);
            }
            __syncthreads();                                          // ---- barrier A
            // ================= variable step + incremental syndrome test ==========================================
            const int p = total & 1;
            if constexpr (VARIANT == 2) {
                record_variable_step<true>(G, S, p, syn_weight, P.clip_llr, [&](int x) { return Wp[x]; },
                                           [&](int o, double q) {
                                               const double y = stuck[o] ? __longlong_as_double(0x7ff8000000000000ll) : q;
                                               if (!(y - y == 0.0)) stuck[o] = 1;
                                               return y;
                                           });
            } else {
                record_variable_step<false>(G, S, p, syn_weight, P.clip_llr, [&](int x) { return Wp[x]; });
            }
            __syncthreads();                                          // ---- barrier B
            ++total;
            solved = S.unsat[p] == 0;
        }
        // ---- outputs: the values of the last iteration executed --------------------------------------------------------
        for (int x = tid; x < n; x += nt) {
            const double val = V[x];
            const int v = G.svar[x];
            if (io.llr) io.llr[rec * n + v] = val;
            if (io.hard) io.hard[rec * n + v] = (uint8_t)(val < 0.0 ? 1 : 0);
        }
        if (tid == 0) {
            if (io.converged) io.converged[rec] = (uint8_t)(solved ? 1 : 0);
            if (io.iters) io.iters[rec] = total - 1;      // 0-based iteration of the first match, max_iter - 1 if none
        }
        item = record_next_item(G, S, dynamic);
    }
}

// ---- the glue kernels of qbp_css_*: memory-bound byte movers in the style of qbp_window.hpp ----------------------------
constexpr int CSS_THREADS = 256;
constexpr int CSS_MAX_GRID = 2048;        // blocks of a launch; the loops stride over the rest
constexpr unsigned CSS_PHILOX_WORD3 = 3u; // QBP_CSS_PHILOX_STREAM of include/qbp.h

struct CssClassify {
    long long T;
    int n, ma, mb;
    const uint8_t* e_a;             // [T][n] what the first sector's matrix detects, and its correction
    const uint8_t* x_a;
    const uint8_t* e_b;
    const uint8_t* x_b;
    const uint8_t* conv_a;          // [T] the BP stage's converged flags and iterations
    const uint8_t* conv_b;
    const int32_t* it_a;
    const int32_t* it_b;
    const int32_t* row_ptr_a;       // CSR of both matrices: a correction is valid when H (x ^ e) == 0
    const int32_t* col_idx_a;
    const int32_t* row_ptr_b;
    const int32_t* col_idx_b;
    const unsigned long long* l_a;  // per column, bit l: logical operator l of the sector has it
    const unsigned long long* l_b;
    int half_distance;
    long long* counters;            // [3][NUM_COUNTERS]
};

#ifdef QBP_COND_TU

// One Pauli per (trial, qubit): Philox4x32-10 on the counter (trial lo, trial hi, qubit / 4, 3), word qubit % 4 = u;
// u < t1: Z, u < t2: X, u < t3: Y, else none.  e_a = Z or Y, e_b = X or Y.  One lane per (trial, four qubits).
__global__ __launch_bounds__(CSS_THREADS) void css_sample_pauli_kernel(uint8_t* __restrict__ e_a, uint8_t* __restrict__ e_b,
                                                                        int n, long long T, long long trial_begin,
                                                                        unsigned long long seed, unsigned t1, unsigned t2,
                                                                        unsigned t3)
{
    const int n4 = (n + 3) >> 2;
    const long long total = T * (long long)n4, step = (long long)gridDim.x * CSS_THREADS;
    for (long long i = (long long)blockIdx.x * CSS_THREADS + threadIdx.x; i < total; i += step) {
        const long long t = i / n4;
        const int g = (int)(i - t * n4);
        const unsigned long long trial = (unsigned long long)(trial_begin + t);
        unsigned c[4] = {(unsigned)trial, (unsigned)(trial >> 32), (unsigned)g, CSS_PHILOX_WORD3};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * g + k;
            if (q < n) {
                const unsigned u = c[k];
                const bool z = u < t1, x = !z && u < t2, y = !z && !x && u < t3;
                e_a[t * n + q] = (uint8_t)(z || y ? 1 : 0);
                e_b[t * n + q] = (uint8_t)(x || y ? 1 : 0);
            }
        }
    }
}

// x [T][n] = sol where the record's BP did not converge, else hard (bit 0 of each).
__global__ __launch_bounds__(CSS_THREADS) void css_select_kernel(const uint8_t* __restrict__ hard,
                                                                  const uint8_t* __restrict__ sol,
                                                                  const uint8_t* __restrict__ conv, long long T, int n,
                                                                  uint8_t* __restrict__ x)
{
    const long long total = T * (long long)n, step = (long long)gridDim.x * CSS_THREADS;
    for (long long i = (long long)blockIdx.x * CSS_THREADS + threadIdx.x; i < total; i += step)
        x[i] = (conv[i / n] ? hard[i] : sol[i]) & 1u;
}

// One sector of one trial, by one wavefront: logical mask, error weight, difference flag and validity of x against e.
struct CssSector {
    unsigned long long lm;
    int ew, df, bad;
};
__device__ __forceinline__ CssSector css_sector(const uint8_t* e, const uint8_t* d, int n, int m,
                                                const int32_t* row_ptr, const int32_t* col_idx,
                                                const unsigned long long* l_cols, int lane)
{
    CssSector s{0ull, 0, 0, 0};
    for (int v = lane; v < n; v += 64) {
        const unsigned eb = e[v] & 1u, res = (d[v] ^ eb) & 1u;
        s.ew += (int)eb;
        s.df |= (int)res;
        if (res) s.lm ^= l_cols[v];
    }
    for (int c = lane; c < m; c += 64) {
        unsigned acc = 0;
        for (int k = row_ptr[c]; k < row_ptr[c + 1]; ++k) acc ^= d[col_idx[k]] ^ e[col_idx[k]];
        s.bad |= (int)(acc & 1u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s.lm ^= __shfl_xor(s.lm, o, 64);
        s.ew += __shfl_xor(s.ew, o, 64);
        s.df |= __shfl_xor(s.df, o, 64);
        s.bad |= __shfl_xor(s.bad, o, 64);
    }
    return s;
}

// Classification of T trials decoded in both sectors, one wavefront per trial.  Rows 0 and 1: mc_count_trial on the
// sector, with window_classify_kernel's two additions (a correction OSD made valid counts for degenerateErrors; [10]
// counts the corrections that miss their syndrome).  Row 2, the trial as a whole: [0] trials, [1] a logical error in
// either sector, [6] either BP unconverged, [8] the [1] among the [6], [9] both corrections equal to the errors,
// [10] either correction misses its syndrome.  Summed per workgroup in LDS, one atomic per counter and workgroup.
__global__ __launch_bounds__(CSS_THREADS) void css_classify_kernel(const CssClassify P)
{
    __shared__ unsigned long long block_cnt[3 * NUM_COUNTERS];
    if (threadIdx.x < 3 * NUM_COUNTERS) block_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (CSS_THREADS / 64);
    for (long long t = (long long)blockIdx.x * (CSS_THREADS / 64) + (threadIdx.x >> 6); t < P.T; t += waves) {
        const CssSector a = css_sector(P.e_a + t * P.n, P.x_a + t * P.n, P.n, P.ma, P.row_ptr_a, P.col_idx_a, P.l_a, lane);
        const CssSector b = css_sector(P.e_b + t * P.n, P.x_b + t * P.n, P.n, P.mb, P.row_ptr_b, P.col_idx_b, P.l_b, lane);
        if (lane == 0) {
            int cnt[3][NUM_COUNTERS];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int i = 0; i < NUM_COUNTERS; ++i) cnt[r][i] = 0;
            const int conv_a = P.conv_a[t] != 0, conv_b = P.conv_b[t] != 0;
            mc_count_trial(cnt[0], a.lm, a.ew, a.df, conv_a, P.it_a[t], P.half_distance);
            if (!conv_a && !a.bad && a.lm == 0ull && a.df) cnt[0][5] += 1;
            if (a.bad) cnt[0][10] += 1;
            mc_count_trial(cnt[1], b.lm, b.ew, b.df, conv_b, P.it_b[t], P.half_distance);
            if (!conv_b && !b.bad && b.lm == 0ull && b.df) cnt[1][5] += 1;
            if (b.bad) cnt[1][10] += 1;
            const bool logical = (a.lm | b.lm) != 0ull, unconv = !conv_a || !conv_b;
            cnt[2][0] = 1;
            if (logical) cnt[2][1] = 1;
            if (unconv) cnt[2][6] = 1;
            if (logical && unconv) cnt[2][8] = 1;
            if (!a.df && !b.df) cnt[2][9] = 1;
            if (a.bad || b.bad) cnt[2][10] = 1;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int i = 0; i < NUM_COUNTERS; ++i)
                    if (cnt[r][i]) atomicAdd(&block_cnt[r * NUM_COUNTERS + i], (unsigned long long)cnt[r][i]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * NUM_COUNTERS && block_cnt[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(P.counters) + threadIdx.x, block_cnt[threadIdx.x]);
}

#endif  // QBP_COND_TU

}  // namespace qbp
