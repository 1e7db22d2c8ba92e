// BP guided decimation (BPGD): rounds of flooding BP; a round that ends without a solution freezes the most reliable
// variable by overwriting its prior with +-decim_llr, and the next round continues on the same messages (include/qbp.h,
// qbp_gd_decode_batch, states the rules; tests/gd_oracle.py is the numpy statement the kernel is compared with bit
// for bit).
//
// The shape is bp_relay_kernel's (qbp_relay.hpp): one workgroup per record on the tables of the general-H kernel
// (class-blocked, transposed message layout; srow / epos / vpos / vrow / svar), two workgroup barriers per iteration:
//   check step     one thread per check of weight <= 8 (check_row of qbp_check.hpp: min-sum, or the exact sum-product row
//                  on numpy's tanh / arctanh tables), rows beyond that in passes (one message per edge, the sequential
//                  product / minimum search per check), on ONE array of E messages updated in place;
//   -- barrier A --
//   variable step  one thread per variable: V = colsum(R) + W (ascending check; W is the working prior), Q = V - R in
//                  place (min-sum: clipped), and the incremental syndrome test of the general-H kernel;
//   -- barrier B --
//   counter zero <=> H hard == s: the record is done.
// After the T iterations of a round without a solution, one block-wide arg-max chooses the variable to decimate: the key
// is (|V| as its bit pattern, then the lowest ORIGINAL variable index) over the variables that have a check, are not
// decimated yet and whose V is not NaN.  Every thread takes the best of its own variables, a wavefront reduces with
// cross-lane shuffles, lane 0 of each writes three LDS words, and after one barrier every thread reads the (at most 8)
// wavefront results: no thread scans the variables alone.  The kernel walks the variables in the sorted order svar, so
// the index of the key is svar[x], not x: on the symmetric codes with uniform priors exact ties in |V| are the rule.
// Per-record state, all in LDS: the E messages, V[n], W[n] (both in sorted-variable order), the decimated map (n bits),
// the syndrome and parity bits, and for sum-product numpy's function tables at LDS address 0.
// Two builds: RECORDS = false decodes B syndromes to outputs; RECORDS = true reads the failure records of a Monte-Carlo
// launch (count and list in device memory, fail_syn, fail_err), decodes them and classifies the result into the
// counters, as the Relay-BP and OSD record kernels do.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_check.hpp"
#include "qbp_generic.hpp"
#include "qbp_mc.hpp"

namespace qbp {

constexpr int GD_MAX_THREADS = 512;
constexpr int GD_MAX_WAVES = GD_MAX_THREADS / 64;

struct GdParams {
    int m, n, E;
    // ---- tables of the general-H kernel (GenericParams has the layout) --------------------------------------------
    const int32_t* srow;
    const int32_t* srow_e0;
    const int32_t* srow_deg;
    const int32_t* epos;
    const int32_t* long_edge_row;
    const int32_t* svar;
    const int32_t* vpos;
    const int32_t* vrow;
    const int32_t* lcol_ptr;
    int row_off[GENERIC_MAX_ROW_CLASS + 3];
    int row_base[GENERIC_MAX_ROW_CLASS + 2];
    int rpad_off[GENERIC_MAX_ROW_CLASS + 2];
    int col_off[GENERIC_MAX_COL_CLASS + 3];
    int col_base[GENERIC_MAX_COL_CLASS + 2];
    int cpad_off[GENERIC_MAX_COL_CLASS + 2];
    const double* prior_sorted;     // [n] prior of the sorted variable x
    double* wsL;                    // [grid][3 * number of long checks] (min-sum: sprod, min1, min2; sum-product: prod)
    unsigned* work_counter;         // zeroed before launch: index - grid of the next record
    // ---- the configuration (qbp_gd_configure) -----------------------------------------------------------------------
    int iters_per_round, max_rounds;
    double decim_llr, alpha, clip_llr;
    // ---- batch build: syndromes in, outputs out (any output may be null) ----------------------------------------
    const uint8_t* syndromes;       // [B][m]
    long long B;
    uint8_t* hard;                  // [B][n]
    uint8_t* converged;             // [B]
    int32_t* iters;                 // [B] iterations executed, all rounds
    double* llr;                    // [B][n]
    int32_t* rounds;                // [B] variables decimated
    // ---- records build: the failure records of a Monte-Carlo launch --------------------------------------------------
    const unsigned long long* fail_count;   // number of records (device)
    const long long* fail_list;     // record index of item i
    const uint8_t* fail_syn;        // [*][m]
    const uint8_t* fail_err;        // [*][n]
    const unsigned long long* lx_cols;
    int half_distance;
    long long* counters;
};

// 32-bit words behind the doubles: logical mask (2), error weight, difference flag, unsatisfied checks [2], next
// record, pad; the arg-max results of the wavefronts (|V| bits [W] as 64-bit, variable [W], sorted position [W]);
// syndrome bits [mw], parity bits [2][mw], decimated map [nw]
constexpr int GD_HEAD_WORDS = 8 + 4 * GD_MAX_WAVES;
__host__ __device__ inline size_t gd_lds_words(int m, int n)
{
    const size_t mw = ((size_t)m + 31) >> 5, nw = ((size_t)n + 31) >> 5;
    return ((size_t)GD_HEAD_WORDS + 3 * mw + nw + 1) & ~(size_t)1;
}
// Dynamic LDS of one workgroup: (sum-product) the function tables, E messages, V and W [n] each, the words
__host__ __device__ inline size_t gd_lds_bytes(int m, int n, int E, bool tables)
{
    return (tables ? (size_t)NP_LDS_BYTES : 0) + (size_t)8 * ((size_t)E + 2 * (size_t)n) + 4 * gd_lds_words(m, n);
}

// Threads of a workgroup: the larger of the two steps' padded work in equal passes of at most GD_MAX_THREADS
// ([[144,12,12]]: 192, [[288,12,18]]: 320)
__host__ inline int gd_threads(int check_items, int var_items)
{
    int work = check_items > var_items ? check_items : var_items;
    if (work < 64) work = 64;
    const int passes = (work + GD_MAX_THREADS - 1) / GD_MAX_THREADS;
    return (((work + passes - 1) / passes) + 63) / 64 * 64;
}

// The arg-max key: larger |V| bits first, then the lower variable index.  (0, INT_MAX) is "no candidate": every
// candidate beats it.
struct GdKey {
    unsigned long long bits;
    int var, pos;
};
__device__ __forceinline__ bool gd_better(const GdKey& a, const GdKey& b)
{
    return a.bits > b.bits || (a.bits == b.bits && a.var < b.var);
}

template <int VARIANT, bool RECORDS>
__global__ __launch_bounds__(GD_MAX_THREADS) void bp_gd_kernel(const GdParams P)
{
    static_assert(VARIANT == 0 || VARIANT == 2, "sum-product or min-sum");
    extern __shared__ __attribute__((aligned(16))) double gd_smem[];
    constexpr NpT np_tab = 0u;          // the tables of tanh / arctanh sit at LDS address 0 (sum-product)
    constexpr int TAB = VARIANT == 0 ? NP_LDS_DOUBLES : 0;
    constexpr int RC = GENERIC_MAX_ROW_CLASS, CC = GENERIC_MAX_COL_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = P.m, n = P.n, E = P.E;
    double* const M = gd_smem + TAB;                // [E] messages, in place
    double* const V = M + E;                        // [n] posterior values, sorted-variable order
    double* const Wp = V + n;                       // [n] working prior, sorted-variable order
    unsigned* const words = reinterpret_cast<unsigned*>(Wp + n);
    const int mw = (m + 31) >> 5, nw = (n + 31) >> 5;
    unsigned long long* const mc_lmask = reinterpret_cast<unsigned long long*>(words);
    int* const mc_weight = reinterpret_cast<int*>(words + 2);
    int* const mc_diff = reinterpret_cast<int*>(words + 3);
    int* const unsat = reinterpret_cast<int*>(words + 4);           // [2] set bits of par, by iteration parity
    unsigned* const next_item = words + 6;
    unsigned long long* const am_bits = reinterpret_cast<unsigned long long*>(words + 8);      // [GD_MAX_WAVES]
    int* const am_var = reinterpret_cast<int*>(words + 8 + 2 * GD_MAX_WAVES);                  // [GD_MAX_WAVES]
    int* const am_pos = am_var + GD_MAX_WAVES;                                                 // [GD_MAX_WAVES]
    unsigned* const synw = words + GD_HEAD_WORDS;   // [mw] syndrome bits, sorted check order
    unsigned* const par = synw + mw;                // [2][mw] parity of H hard ^ s
    unsigned* const decw = par + 2 * mw;            // [nw] decimated variables, by sorted position

    const int first_long = P.row_off[RC + 1], n_long = P.row_off[RC + 2] - first_long;
    const int lbase = P.row_base[RC + 1], n_ledges = E - lbase;
    const int first_lcol = P.col_off[CC + 1], n_lcol = P.col_off[CC + 2] - first_lcol;
    const double clip = P.clip_llr;
    const int T = P.iters_per_round;
    double* const Lw = P.wsL + (size_t)blockIdx.x * 3 * (n_long > 0 ? n_long : 1);

    if constexpr (VARIANT == 0) np_tables_to_lds(gd_smem, tid, nt);     // (published by the record's first barrier)
    if constexpr (RECORDS) {
        if (tid == 0) { *mc_lmask = 0ull; *mc_weight = 0; *mc_diff = 0; }
    }
    long long count = P.B;
    if constexpr (RECORDS) count = (long long)*P.fail_count;
    const bool dynamic = count > (long long)gridDim.x;

    // new variable->check message of one edge: V - R, clipped in min-sum; no damping term
    auto q_of = [&](double val, double r) {
        const double q = val - r;
        if constexpr (VARIANT == 2) {
            const double y = q < -clip ? -clip : q;
            return y > clip ? clip : y;
        } else {
            return q;
        }
    };

    for (long long item = blockIdx.x; item < count;) {
        const long long rec = RECORDS ? P.fail_list[item] : item;
        const uint8_t* const syn = RECORDS ? P.fail_syn + rec * m : P.syndromes + rec * m;
        if (tid == 0) unsat[0] = 0;
        __syncthreads();      // (the previous record's last readers of LDS are done)
        // ---- syndrome bits in sorted check order; parity buffer 0 := syndrome ------------------------------------
        {
            int cnt = 0;
            for (int w0 = tid - lane; w0 < m; w0 += nt) {           // w0 is wave-uniform
                const int w = w0 + lane;
                const unsigned bit = w < m ? (syn[P.srow[w]] & 1u) : 0u;
                const unsigned long long mask = __ballot(bit != 0);
                if (lane == 0) {
                    const int wi = w0 >> 5;
                    synw[wi] = (unsigned)mask; par[wi] = (unsigned)mask;
                    if (wi + 1 < mw) { synw[wi + 1] = (unsigned)(mask >> 32); par[wi + 1] = (unsigned)(mask >> 32); }
                    cnt += __builtin_popcountll(mask);
                }
            }
            if (lane == 0 && cnt) atomicAdd(&unsat[0], cnt);
        }
        // ---- rule 1: W = V = prior, Q = prior on the edges, nothing decimated ----------------------------------------
        for (int i = tid; i < nw; i += nt) decw[i] = 0u;
        for (int x = tid; x < n; x += nt) {
            const double pv = P.prior_sorted[x];
            Wp[x] = pv; V[x] = pv;
        }
        for (int x = tid + P.col_off[1]; x < first_lcol; x += nt) {
            int D, cnt, o;
            if (x < P.col_off[2])      { D = 1; cnt = P.col_off[2] - P.col_off[1]; o = P.col_base[1] + (x - P.col_off[1]); }
            else if (x < P.col_off[3]) { D = 2; cnt = P.col_off[3] - P.col_off[2]; o = P.col_base[2] + (x - P.col_off[2]); }
            else if (x < P.col_off[4]) { D = 3; cnt = P.col_off[4] - P.col_off[3]; o = P.col_base[3] + (x - P.col_off[3]); }
            else                       { D = 4; cnt = P.col_off[5] - P.col_off[4]; o = P.col_base[4] + (x - P.col_off[4]); }
            const double pv = P.prior_sorted[x];
            for (int j = 0; j < D; ++j) M[P.vpos[o + (size_t)j * cnt]] = pv;
        }
        for (int i = tid; i < n_lcol; i += nt) {
            const double pv = P.prior_sorted[first_lcol + i];
            for (int k = P.lcol_ptr[i]; k < P.lcol_ptr[i + 1]; ++k) M[P.vpos[k]] = pv;
        }
        __syncthreads();
        const int syn_weight = unsat[0];      // unsatisfied checks of the all-zero candidate

        int total = 0, rounds = 0;
        bool solved = false;
        for (;;) {
            // ===================== one round: T iterations (rule 2) ===================================================
            for (int t = 0; t < T && !solved; ++t) {
                // ================= check step (rule 2.1) ==========================================================
                for (int wp0 = tid - lane; wp0 < P.rpad_off[RC + 1]; wp0 += nt) {
                    // one wavefront = 64 consecutive work items of ONE weight class (scalar class search)
                    const int wpu = __builtin_amdgcn_readfirstlane(wp0);
                    int D = 1;
#pragma unroll
                    for (int k = 2; k <= RC; ++k) D += wpu >= P.rpad_off[k] ? 1 : 0;
                    int lane_ = lane;       // (opaque: keeps the per-class address arithmetic inside the loop)
                    asm volatile("" : "+v"(lane_));
#define QBP_GD_ROW_CLASS(DD)                                                                       \
                    case DD: {                                                                     \
                        const int cnt = P.row_off[DD + 1] - P.row_off[DD];                         \
                        const int i = wpu - P.rpad_off[DD] + lane_;                                \
                        if (i < cnt) {                                                             \
                            const int w = P.row_off[DD] + i;                                       \
                            const unsigned sbit = (synw[w >> 5] >> (w & 31)) & 1u;                 \
                            const int base = P.row_base[DD] + i;                                   \
                            double q[DD];                                                          \
                            _Pragma("unroll") for (int j = 0; j < DD; ++j) q[j] = M[base + j * cnt];   \
                            auto put = [&](int j, double v) { M[base + j * cnt] = v; };            \
                            check_row<VARIANT, DD, true>(q, sbit, P.alpha, true, np_tab, put);     \
                        }                                                                          \
                    } break;
                    switch (D) {
                        QBP_GD_ROW_CLASS(1) QBP_GD_ROW_CLASS(2) QBP_GD_ROW_CLASS(3) QBP_GD_ROW_CLASS(4)
                        QBP_GD_ROW_CLASS(5) QBP_GD_ROW_CLASS(6) QBP_GD_ROW_CLASS(7) QBP_GD_ROW_CLASS(8)
                        default: break;
                    }
#undef QBP_GD_ROW_CLASS
                }
                // ---- checks of weight > 8: the per-edge work one thread per edge, the sequential part (np.prod in
                //      ascending column order / the minimum search) one thread per check
                if (n_long > 0) {                                           // uniform
                    if constexpr (VARIANT == 0) {
                        for (int k = tid; k < n_ledges; k += nt) M[lbase + k] = tanh_half_msg<VARIANT>(M[lbase + k], np_tab);
                        __syncthreads();
                    }
                    for (int i = tid; i < n_long; i += nt) {
                        const int deg = P.srow_deg[first_long + i];
                        const int p0 = P.epos[P.srow_e0[first_long + i]];   // entries contiguous from here
                        if constexpr (VARIANT == 2) {
                            const MinSumRow row = minsum_row([&](int j) { return M[p0 + j]; }, deg);
                            Lw[3 * i] = row.sprod; Lw[3 * i + 1] = row.min1; Lw[3 * i + 2] = row.min2;
                        } else {
                            double prod = M[p0];
                            for (int j = 1; j < deg; ++j) prod = prod * M[p0 + j];
                            Lw[3 * i] = prod;
                        }
                    }
                    __syncthreads();
                    for (int k = tid; k < n_ledges; k += nt) {
                        const int i = P.long_edge_row[k];
                        const int w = first_long + i;
                        const unsigned sbit = (synw[w >> 5] >> (w & 31)) & 1u;
                        if constexpr (VARIANT == 2) {
                            M[lbase + k] = minsum_message(M[lbase + k], MinSumRow{Lw[3 * i], Lw[3 * i + 1], Lw[3 * i + 2]},
                                                          sbit, P.alpha);
                        } else {
                            M[lbase + k] = sp_message<VARIANT>(Lw[3 * i], M[lbase + k], sbit, np_tab);
                        }
                    }
                }
                __syncthreads();                                          // ---- barrier A
                // ================= variable step (rules 2.2 - 2.4) + incremental syndrome test (2.5) ================
                const int p = total & 1;
                unsigned* const pbuf = par + p * mw;
                {   // the other buffer becomes the syndrome again (its last readers passed barrier A)
                    unsigned* const obuf = par + (p ^ 1) * mw;
                    for (int i = tid; i < mw; i += nt) obuf[i] = synw[i];
                    if (tid == 0) unsat[p ^ 1] = syn_weight;
                }
                int delta = 0;
                auto flip = [&](int cw) {             // the check at sorted position cw changes parity
                    const unsigned bit = 1u << (cw & 31);
                    const unsigned old = atomicXor(&pbuf[cw >> 5], bit);
                    delta += (old & bit) ? -1 : 1;
                };
                for (int x = tid; x < P.col_off[1]; x += nt) V[x] = 0.0 + Wp[x];     // no check: an empty column sum
                for (int xp0 = tid - lane; xp0 < P.cpad_off[CC + 1]; xp0 += nt) {
                    const int xpu = __builtin_amdgcn_readfirstlane(xp0);
                    int D = 1;
#pragma unroll
                    for (int k = 2; k <= CC; ++k) D += xpu >= P.cpad_off[k] ? 1 : 0;
                    int lane_ = lane;
                    asm volatile("" : "+v"(lane_));
#define QBP_GD_COL_CLASS(DD)                                                                       \
                    case DD: {                                                                     \
                        const int cnt = P.col_off[DD + 1] - P.col_off[DD];                         \
                        const int i = xpu - P.cpad_off[DD] + lane_;                                \
                        if (i < cnt) {                                                             \
                            const int base = P.col_base[DD] + i;                                   \
                            const int x = P.col_off[DD] + i;                                       \
                            int o[DD];                                                             \
                            double r[DD];                                                          \
                            _Pragma("unroll") for (int j = 0; j < DD; ++j) o[j] = P.vpos[base + j * cnt];  \
                            _Pragma("unroll") for (int j = 0; j < DD; ++j) r[j] = M[o[j]];         \
                            double s = r[0];                                                       \
                            _Pragma("unroll") for (int j = 1; j < DD; ++j) s = s + r[j];           \
                            const double val = s + Wp[x];                                          \
                            V[x] = val;                                                            \
                            if (val < 0.0) {                                                       \
                                _Pragma("unroll") for (int j = 0; j < DD; ++j) flip(P.vrow[base + j * cnt]); \
                            }                                                                      \
                            _Pragma("unroll") for (int j = 0; j < DD; ++j) M[o[j]] = q_of(val, r[j]);  \
                        }                                                                          \
                    } break;
                    switch (D) {
                        QBP_GD_COL_CLASS(1) QBP_GD_COL_CLASS(2) QBP_GD_COL_CLASS(3) QBP_GD_COL_CLASS(4)
                        default: break;
                    }
#undef QBP_GD_COL_CLASS
                }
                for (int i = tid; i < n_lcol; i += nt) {
                    const int k0 = P.lcol_ptr[i], k1 = P.lcol_ptr[i + 1];
                    const int x = first_lcol + i;
                    double s = 0.0;
                    for (int k = k0; k < k1; ++k) {
                        const double r = M[P.vpos[k]];
                        s = (k == k0) ? r : s + r;                    // ascending check order
                    }
                    const double val = s + Wp[x];
                    V[x] = val;
                    if (val < 0.0)
                        for (int k = k0; k < k1; ++k) flip(P.vrow[k]);
                    for (int k = k0; k < k1; ++k) {
                        const int o = P.vpos[k];
                        M[o] = q_of(val, M[o]);
                    }
                }
                if (delta) atomicAdd(&unsat[p], delta);
                __syncthreads();                                          // ---- barrier B
                ++total;
                solved = unsat[p] == 0;
            }
            if (solved || rounds == P.max_rounds) break;                  // rule 3 (uniform)
            // ===================== the variable to decimate: block-wide arg-max ========================================
            GdKey best{0ull, 0x7fffffff, 0};
            for (int x = tid + P.col_off[1]; x < n; x += nt) {            // (variables before col_off[1] have no check)
                const double val = V[x];
                if (val != val || ((decw[x >> 5] >> (x & 31)) & 1u)) continue;
                const GdKey k{(unsigned long long)__double_as_longlong(val) & 0x7fffffffffffffffull, P.svar[x], x};
                if (gd_better(k, best)) best = k;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                GdKey o;
                o.bits = (unsigned long long)__shfl_xor((long long)best.bits, off, 64);
                o.var = __shfl_xor(best.var, off, 64);
                o.pos = __shfl_xor(best.pos, off, 64);
                if (gd_better(o, best)) best = o;
            }
            if (lane == 0) { am_bits[tid >> 6] = best.bits; am_var[tid >> 6] = best.var; am_pos[tid >> 6] = best.pos; }
            __syncthreads();
            best = GdKey{am_bits[0], am_var[0], am_pos[0]};
            for (int w = 1; w < (nt >> 6); ++w) {
                const GdKey o{am_bits[w], am_var[w], am_pos[w]};
                if (gd_better(o, best)) best = o;
            }
            if (best.var == 0x7fffffff) break;                            // no candidate left (uniform)
            if (tid == 0) {
                // (W and the map are read next after barrier A of the coming iteration; V is written after it)
                Wp[best.pos] = V[best.pos] < 0.0 ? -P.decim_llr : P.decim_llr;
                decw[best.pos >> 5] |= 1u << (best.pos & 31);
            }
            ++rounds;
        }
        // ---- rule 4: the last iteration executed -----------------------------------------------------------------------
        if constexpr (RECORDS) {
            // classification of the result (paperResults_GPU.py:127-144), as the OSD record kernels do it: the
            // first stage has counted the trial, its iterations and its not_converged
            const uint8_t* const err = P.fail_err + rec * n;
            unsigned long long lm = 0ull;
            int ew = 0, df = 0;
            for (int x = tid; x < n; x += nt) {
                const int v = P.svar[x];
                const unsigned e = err[v] & 1u;
                const unsigned res = (V[x] < 0.0 ? 1u : 0u) ^ e;
                ew += (int)e;
                df |= (int)res;
                if (res) lm ^= P.lx_cols[v];
            }
            if (lm) atomicXor(mc_lmask, lm);
            if (ew) atomicAdd(mc_weight, ew);
            if (df) atomicOr(mc_diff, 1);
            __syncthreads();
            if (tid == 0) {
                int row[NUM_COUNTERS];
#pragma unroll
                for (int i = 0; i < NUM_COUNTERS; ++i) row[i] = 0;
                mc_count_trial(row, *mc_lmask, *mc_weight, *mc_diff, solved ? 1 : 0, 0, P.half_distance);
                *mc_lmask = 0ull; *mc_weight = 0; *mc_diff = 0;
                auto add = [&](int i) { atomicAdd(reinterpret_cast<unsigned long long*>(P.counters + i), 1ull); };
                if (row[5]) add(5);
                if (row[1]) { add(1); add(row[3] ? 3 : 4); add(8); }     // (every record is a trial BP left unconverged)
                if (row[9]) add(9);
                if (!solved) add(10);                                    // no solution: the output misses the syndrome
            }
        } else {
            for (int x = tid; x < n; x += nt) {
                const double val = V[x];
                const int v = P.svar[x];
                if (P.llr) P.llr[rec * n + v] = val;
                if (P.hard) P.hard[rec * n + v] = (uint8_t)(val < 0.0 ? 1 : 0);
            }
            if (tid == 0) {
                if (P.converged) P.converged[rec] = (uint8_t)(solved ? 1 : 0);
                if (P.iters) P.iters[rec] = total;
                if (P.rounds) P.rounds[rec] = rounds;
            }
        }
        if (tid == 0) *next_item = dynamic ? atomicAdd(P.work_counter, 1u) : 0x7fffffffu;
        __syncthreads();
        item = (long long)gridDim.x + (long long)*next_item;      // (next write: after the barriers of the next record)
    }
}

}  // namespace qbp
