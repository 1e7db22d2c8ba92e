// Relay-BP: min-sum with a disordered memory term, run as a chain of legs (include/qbp.h, qbp_relay_decode_batch,
// states the rules; tests/relay_oracle.py is the numpy statement the kernel is compared with bit for bit).
//
// One workgroup per record on the tables of the general-H kernel (qbp_generic.hpp: class-blocked, transposed message
// layout; srow / epos / vpos / vrow / svar), two workgroup barriers per iteration:
//   check step     one thread per check of weight <= 8 (check_row of qbp_check.hpp), rows beyond that in two passes
//                  (minsum_row per check, minsum_message per edge), on ONE array of E messages updated in place: a slot
//                  holds the variable->check message before the step and the check->variable message after it;
//   -- barrier A --
//   variable step  one thread per variable: bias = (1 - gamma) prior + gamma V, V = colsum(R) + bias (ascending check),
//                  Q = clip(V - R) in place, and the incremental syndrome test of the general-H kernel (parity bits in
//                  LDS, a counter of unsatisfied checks);
//   -- barrier B --
//   counter zero <=> H hard == s: a solution.  One thread adds up its weight in column order (as osd_order_kernel adds
//   its costs); if it is the lightest so far the workgroup writes it straight to the record's output row.
// Everything a record touches per iteration is in LDS: the E messages, V[n], the prior and the current leg's gamma row
// (both in sorted-variable order; gamma is reloaded at each leg start), the syndrome and parity bits.  Min-sum needs no
// tanh / arctanh tables.  A record of [[144,12,12]] takes 7 KB, so the workgroup is kept small (relay_threads) and
// several are resident per CU: records run hundreds of iterations of a few dozen instructions each, and what hides
// the LDS and barrier latency of one is the other workgroups of the CU.
// Two builds: RECORDS = false decodes B syndromes to outputs; RECORDS = true reads the failure records of a
// Monte-Carlo launch (count and list in device memory, fail_syn, fail_err), decodes them and classifies the result
// into the counters, as the OSD record kernels do.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_check.hpp"
#include "qbp_generic.hpp"
#include "qbp_mc.hpp"

namespace qbp {

struct RelayParams {
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
    const int32_t* vinv;            // [n] sorted position of variable v (the inverse of svar)
    const double* prior;            // [n] the caller's prior
    const double* prior_sorted;     // [n] prior of the sorted variable x
    double* wsL;                    // [grid][3 * number of long checks] (sprod, min1, min2)
    unsigned* work_counter;         // zeroed before launch: index - grid of the next record
    // ---- the configuration (qbp_relay_configure) -------------------------------------------------------------------
    const double* gammas_sorted;    // [L][n] memory strengths, sorted-variable order
    const int32_t* leg_iters;       // [L]
    int L, stop_after;
    double alpha, clip_llr;
    // ---- batch build: syndromes in, outputs out (any output may be null) ----------------------------------------
    const uint8_t* syndromes;       // [B][m]
    long long B;
    uint8_t* hard;                  // [B][n]
    uint8_t* converged;             // [B]
    int32_t* iters;                 // [B] iterations executed, all legs
    double* llr;                    // [B][n]
    int32_t* legs;                  // [B] legs entered
    int32_t* solutions;             // [B] solutions found
    // ---- records build: the failure records of a Monte-Carlo launch --------------------------------------------------
    const unsigned long long* fail_count;   // number of records (device)
    const long long* fail_list;     // record index of item i
    const uint8_t* fail_syn;        // [*][m]
    const uint8_t* fail_err;        // [*][n]
    const unsigned long long* lx_cols;
    int half_distance;
    long long* counters;
};

// 32-bit words behind the doubles: logical mask (2), error weight, difference flag, unsatisfied checks [2], "write this
// solution" flag, next record, syndrome bits [mw], parity bits [2][mw]
__host__ __device__ inline size_t relay_lds_words(int m)
{
    const size_t mw = ((size_t)m + 31) >> 5;
    return (8 + 3 * mw + 1) & ~(size_t)1;
}
// Dynamic LDS of one workgroup: E messages, V, prior and gamma [n] each, the words, and (records build) the hard
// decision of the best solution, a byte per variable
__host__ __device__ inline size_t relay_lds_bytes(int m, int n, int E, bool records)
{
    return (size_t)8 * ((size_t)E + 3 * (size_t)n) + 4 * relay_lds_words(m) + (records ? (((size_t)n + 7) & ~(size_t)7) : 0);
}

// Threads of a workgroup: the larger of the two steps' padded work in one pass, at most 1024 ([[144,12,12]]: 192,
// [[288,12,18]]: 320 -- nine and five workgroups in the 28 wavefronts a CU holds at the kernel's registers).
__host__ inline int relay_threads(int check_items, int var_items)
{
    int work = check_items > var_items ? check_items : var_items;
    if (work < 64) work = 64;
    const int passes = (work + 1023) / 1024;
    return (((work + passes - 1) / passes) + 63) / 64 * 64;
}

template <bool RECORDS>
__global__ __launch_bounds__(1024) void bp_relay_kernel(const RelayParams P)
{
    extern __shared__ __attribute__((aligned(16))) double relay_smem[];
    constexpr NpT np_tab = 0u;          // (min-sum reads no table)
    constexpr int RC = GENERIC_MAX_ROW_CLASS, CC = GENERIC_MAX_COL_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = P.m, n = P.n, E = P.E;
    double* const M = relay_smem;                   // [E] messages, in place
    double* const V = M + E;                        // [n] posterior values, sorted-variable order
    double* const prior_t = V + n;                  // [n]
    double* const gam = prior_t + n;                // [n] the current leg's memory strengths
    unsigned* const words = reinterpret_cast<unsigned*>(gam + n);
    const int mw = (m + 31) >> 5;
    unsigned long long* const mc_lmask = reinterpret_cast<unsigned long long*>(words);
    int* const mc_weight = reinterpret_cast<int*>(words + 2);
    int* const mc_diff = reinterpret_cast<int*>(words + 3);
    int* const unsat = reinterpret_cast<int*>(words + 4);           // [2] set bits of par, by iteration parity
    unsigned* const better = words + 6;
    unsigned* const next_item = words + 7;
    unsigned* const synw = words + 8;               // [mw] syndrome bits, sorted check order
    unsigned* const par = synw + mw;                // [2][mw] parity of H hard ^ s
    uint8_t* const best_hard = reinterpret_cast<uint8_t*>(words + relay_lds_words(m));   // [n] (records build)

    const int first_long = P.row_off[RC + 1], n_long = P.row_off[RC + 2] - first_long;
    const int lbase = P.row_base[RC + 1], n_ledges = E - lbase;
    const int first_lcol = P.col_off[CC + 1], n_lcol = P.col_off[CC + 2] - first_lcol;
    const double clip = P.clip_llr;
    double* const Lw = P.wsL + (size_t)blockIdx.x * 3 * (n_long > 0 ? n_long : 1);

    for (int x = tid; x < n; x += nt) prior_t[x] = P.prior_sorted[x];
    if constexpr (RECORDS) {
        if (tid == 0) { *mc_lmask = 0ull; *mc_weight = 0; *mc_diff = 0; }
    }
    long long count = P.B;
    if constexpr (RECORDS) count = (long long)*P.fail_count;
    const bool dynamic = count > (long long)gridDim.x;

    // new variable->check message of one edge: clip(V - R), no damping term
    auto q_of = [&](double val, double r) {
        const double q = val - r;
        const double y = q < -clip ? -clip : q;
        return y > clip ? clip : y;
    };

    for (long long item = blockIdx.x; item < count;) {
        const long long rec = RECORDS ? P.fail_list[item] : item;
        const uint8_t* const syn = RECORDS ? P.fail_syn + rec * m : P.syndromes + rec * m;
        if (tid == 0) unsat[0] = 0;
        __syncthreads();      // (also: the prior is in LDS; the previous record's last readers of LDS are done)
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
        // ---- rule 1: Q = prior on the edges, V = prior ---------------------------------------------------------------
        for (int x = tid; x < n; x += nt) V[x] = prior_t[x];
        for (int x = tid + P.col_off[1]; x < first_lcol; x += nt) {
            int D, cnt, o;
            if (x < P.col_off[2])      { D = 1; cnt = P.col_off[2] - P.col_off[1]; o = P.col_base[1] + (x - P.col_off[1]); }
            else if (x < P.col_off[3]) { D = 2; cnt = P.col_off[3] - P.col_off[2]; o = P.col_base[2] + (x - P.col_off[2]); }
            else if (x < P.col_off[4]) { D = 3; cnt = P.col_off[4] - P.col_off[3]; o = P.col_base[3] + (x - P.col_off[3]); }
            else                       { D = 4; cnt = P.col_off[5] - P.col_off[4]; o = P.col_base[4] + (x - P.col_off[4]); }
            const double pv = prior_t[x];
            for (int j = 0; j < D; ++j) M[P.vpos[o + (size_t)j * cnt]] = pv;
        }
        for (int i = tid; i < n_lcol; i += nt) {
            const double pv = prior_t[first_lcol + i];
            for (int k = P.lcol_ptr[i]; k < P.lcol_ptr[i + 1]; ++k) M[P.vpos[k]] = pv;
        }
        __syncthreads();
        const int syn_weight = unsat[0];      // unsatisfied checks of the all-zero candidate

        int found = 0, total = 0, legs = 0;
        double best_w = 0.0;                  // (thread 0)
        for (int leg = 0; leg < P.L; ++leg) {
            ++legs;
            // (the last readers of gam passed barrier B of the previous leg; barrier A publishes the new row)
            for (int x = tid; x < n; x += nt) gam[x] = P.gammas_sorted[(size_t)leg * n + x];
            const int T = P.leg_iters[leg];
            bool solved = false;
            for (int t = 0; t < T && !solved; ++t) {
                // ================= check step (rule 2a) ==========================================================
                for (int wp0 = tid - lane; wp0 < P.rpad_off[RC + 1]; wp0 += nt) {
                    // one wavefront = 64 consecutive work items of ONE weight class (scalar class search)
                    const int wpu = __builtin_amdgcn_readfirstlane(wp0);
                    int D = 1;
#pragma unroll
                    for (int k = 2; k <= RC; ++k) D += wpu >= P.rpad_off[k] ? 1 : 0;
                    int lane_ = lane;       // (opaque: keeps the per-class address arithmetic inside the loop)
                    asm volatile("" : "+v"(lane_));
#define QBP_RELAY_ROW_CLASS(DD)                                                                    \
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
                            check_row<2, DD, true>(q, sbit, P.alpha, true, np_tab, put);           \
                        }                                                                          \
                    } break;
                    switch (D) {
                        QBP_RELAY_ROW_CLASS(1) QBP_RELAY_ROW_CLASS(2) QBP_RELAY_ROW_CLASS(3) QBP_RELAY_ROW_CLASS(4)
                        QBP_RELAY_ROW_CLASS(5) QBP_RELAY_ROW_CLASS(6) QBP_RELAY_ROW_CLASS(7) QBP_RELAY_ROW_CLASS(8)
                        default: break;
                    }
#undef QBP_RELAY_ROW_CLASS
                }
                // ---- checks of weight > 8: the minimum search one thread per check, the messages one per edge
                if (n_long > 0) {                                           // uniform
                    for (int i = tid; i < n_long; i += nt) {
                        const int deg = P.srow_deg[first_long + i];
                        const int p0 = P.epos[P.srow_e0[first_long + i]];   // entries contiguous from here
                        const MinSumRow row = minsum_row([&](int j) { return M[p0 + j]; }, deg);
                        Lw[3 * i] = row.sprod; Lw[3 * i + 1] = row.min1; Lw[3 * i + 2] = row.min2;
                    }
                    __syncthreads();
                    for (int k = tid; k < n_ledges; k += nt) {
                        const int i = P.long_edge_row[k];
                        const int w = first_long + i;
                        const unsigned sbit = (synw[w >> 5] >> (w & 31)) & 1u;
                        M[lbase + k] = minsum_message(M[lbase + k], MinSumRow{Lw[3 * i], Lw[3 * i + 1], Lw[3 * i + 2]},
                                                      sbit, P.alpha);
                    }
                }
                __syncthreads();                                          // ---- barrier A
                // ================= variable step (rules 2b - 2e) + incremental syndrome test =====================
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
                // bias of the sorted variable x (rule 2b: every operation rounded on its own)
                auto bias_of = [&](int x) {
                    const double g = gam[x];
                    return (1.0 - g) * prior_t[x] + g * V[x];
                };
                for (int x = tid; x < P.col_off[1]; x += nt) V[x] = 0.0 + bias_of(x);     // no check: an empty column sum
                for (int xp0 = tid - lane; xp0 < P.cpad_off[CC + 1]; xp0 += nt) {
                    const int xpu = __builtin_amdgcn_readfirstlane(xp0);
                    int D = 1;
#pragma unroll
                    for (int k = 2; k <= CC; ++k) D += xpu >= P.cpad_off[k] ? 1 : 0;
                    int lane_ = lane;
                    asm volatile("" : "+v"(lane_));
#define QBP_RELAY_COL_CLASS(DD)                                                                    \
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
                            const double val = s + bias_of(x);                                     \
                            V[x] = val;                                                            \
                            if (val < 0.0) {                                                       \
                                _Pragma("unroll") for (int j = 0; j < DD; ++j) flip(P.vrow[base + j * cnt]); \
                            }                                                                      \
                            _Pragma("unroll") for (int j = 0; j < DD; ++j) M[o[j]] = q_of(val, r[j]);  \
                        }                                                                          \
                    } break;
                    switch (D) {
                        QBP_RELAY_COL_CLASS(1) QBP_RELAY_COL_CLASS(2) QBP_RELAY_COL_CLASS(3) QBP_RELAY_COL_CLASS(4)
                        default: break;
                    }
#undef QBP_RELAY_COL_CLASS
                }
                for (int i = tid; i < n_lcol; i += nt) {
                    const int k0 = P.lcol_ptr[i], k1 = P.lcol_ptr[i + 1];
                    const int x = first_lcol + i;
                    double s = 0.0;
                    for (int k = k0; k < k1; ++k) {
                        const double r = M[P.vpos[k]];
                        s = (k == k0) ? r : s + r;                    // ascending check order
                    }
                    const double val = s + bias_of(x);
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
                if (unsat[p] != 0) continue;
                // ================= a solution (rule 2f) ==========================================================
                solved = true;
                if (tid == 0) {
                    // weight: the priors of the flipped variables, added in ascending v from +0.0
                    double w = 0.0;
                    for (int v = 0; v < n; ++v)
                        if (V[P.vinv[v]] < 0.0) w += P.prior[v];
                    const bool take = found == 0 || w < best_w;
                    if (take) best_w = w;
                    *better = take ? 1u : 0u;
                }
                ++found;
                __syncthreads();
                if (*better) {
                    // the lightest so far: straight to the record's output row
                    for (int x = tid; x < n; x += nt) {
                        const double val = V[x];
                        const uint8_t hd = val < 0.0 ? 1 : 0;
                        if constexpr (RECORDS) {
                            best_hard[x] = hd;
                        } else {
                            const int v = P.svar[x];
                            if (P.llr) P.llr[rec * n + v] = val;
                            if (P.hard) P.hard[rec * n + v] = hd;
                        }
                    }
                }
            }
            if (found >= P.stop_after) break;             // rule 3
        }
        if (found == 0) {
            // no solution: the last iteration executed
            for (int x = tid; x < n; x += nt) {
                const double val = V[x];
                const uint8_t hd = val < 0.0 ? 1 : 0;
                if constexpr (RECORDS) {
                    best_hard[x] = hd;
                } else {
                    const int v = P.svar[x];
                    if (P.llr) P.llr[rec * n + v] = val;
                    if (P.hard) P.hard[rec * n + v] = hd;
                }
            }
        }
        if constexpr (RECORDS) {
            // classification of the result (paperResults_GPU.py:127-144), as the OSD record kernels do it: the
            // first stage has counted the trial, its iterations and its not_converged
            __syncthreads();
            const uint8_t* const err = P.fail_err + rec * n;
            unsigned long long lm = 0ull;
            int ew = 0, df = 0;
            for (int x = tid; x < n; x += nt) {
                const int v = P.svar[x];
                const unsigned e = err[v] & 1u;
                const unsigned res = (unsigned)best_hard[x] ^ e;
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
                mc_count_trial(row, *mc_lmask, *mc_weight, *mc_diff, found > 0 ? 1 : 0, 0, P.half_distance);
                *mc_lmask = 0ull; *mc_weight = 0; *mc_diff = 0;
                auto add = [&](int i) { atomicAdd(reinterpret_cast<unsigned long long*>(P.counters + i), 1ull); };
                if (row[5]) add(5);
                if (row[1]) { add(1); add(row[3] ? 3 : 4); add(8); }     // (every record is a trial BP left unconverged)
                if (row[9]) add(9);
                if (found == 0) add(10);                                 // no solution: the output misses the syndrome
            }
        } else if (tid == 0) {
            if (P.converged) P.converged[rec] = (uint8_t)(found > 0 ? 1 : 0);
            if (P.iters) P.iters[rec] = total;
            if (P.legs) P.legs[rec] = legs;
            if (P.solutions) P.solutions[rec] = found;
        }
        if (tid == 0) *next_item = dynamic ? atomicAdd(P.work_counter, 1u) : 0x7fffffffu;
        __syncthreads();
        item = (long long)gridDim.x + (long long)*next_item;      // (next write: after the barriers of the next record)
    }
}

}  // namespace qbp
