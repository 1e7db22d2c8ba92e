// Fixed-point min-sum BP: messages of q bits, saturating integer arithmetic (include/qbp.h, qbp_quant_configure, states
// the rules; tests/quant_oracle.py is the numpy statement the kernel is compared with bit for bit).  Integer sums are
// exact in any order, so there is no association to pin: the only doubles are the quantisation of the prior (rule 1,
// once per workgroup) and the conversion (double)V of the llr output.
//
// One workgroup decodes S records at once ("slots"), as bp_layered_kernel does.  Per slot in LDS: one message per edge
// in CSR order -- int8 for q <= 8, int16 above; it holds Q (variable->check) before the check step and R
// (check->variable) after it --, the posterior V[n] as int32, the syndrome bits and a few words of bookkeeping; shared
// by the workgroup: the quantised prior P[n] as int32.  The CSR and CSC arrays of the general-H tables (row_ptr,
// col_idx, col_ptr, col_edge) are read from global memory: the same few KB for every workgroup.
//   check step     a work item is (slot, check): one pass over the row's Q for the two smallest magnitudes, the place
//                  of the smallest and the sign parity, a second pass writes R over Q (the row belongs to the item);
//   -- barrier --
//   variable step  a work item is (slot, variable): V = P + the column's R, then Q = clamp(V - R) over R;
//   -- barrier --
//   syndrome test  by row gather of V < 0: a work item is (slot, check);
//   -- barrier --
//   slot turnover  a slot whose record has converged or run out of iterations writes its outputs (or classifies its
//                  trial) and takes the next record from a global counter: early exit is per record, and nothing a
//                  record computes depends on S, the grid or its neighbours.
// Two builds: MC = false decodes B syndromes to outputs; MC = true reads stored errors [T][n], forms the syndromes,
// decodes and classifies with mc_count_trial, or leaves the failure records the second stages read (llr = (double)V).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_mc.hpp"

namespace qbp {

constexpr int QUANT_THREADS = 256;
constexpr int QUANT_MAX_SLOTS = 32;
constexpr unsigned QUANT_FORCE_FULL = 1u;          // QBP_FLAG_FORCE_FULL

struct QuantParams {
    int m, n, E, S;
    const int32_t* row_ptr;         // [m + 1] CSR
    const int32_t* col_idx;         // [E]
    const int32_t* col_ptr;         // [n + 1] CSC
    const int32_t* col_edge;        // [E] the CSR position of every entry, column after column
    const double* prior;            // [n]
    unsigned* work_counter;         // zeroed before launch: index - grid * S of the next record
    int max_iter;
    unsigned flags;                 // QUANT_FORCE_FULL (batch build only)
    int M;                          // 2^(bits - 1) - 1
    double scale;
    int alpha_num, alpha_shift, beta;
    long long B;                    // records (batch build) or trials (Monte-Carlo build)
    // ---- batch build: syndromes in, outputs out (any output may be null) ----------------------------------------
    const uint8_t* syndromes;       // [B][m]
    uint8_t* hard;                  // [B][n]
    uint8_t* converged;             // [B]
    int32_t* iters;                 // [B]
    int32_t* posterior_q;           // [B][n]
    double* llr;                    // [B][n]
    // ---- Monte-Carlo build ------------------------------------------------------------------------------------------
    const uint8_t* errors_in;       // [B][n]
    const unsigned long long* lx_cols;
    int half_distance;
    long long* counters;
    long long* fail_list;           // null = classify the BP output directly
    unsigned long long* fail_count;
    uint8_t *fail_syn, *fail_hard, *fail_err;
    double* fail_llr;
};

// 32-bit words behind the messages.  Workgroup: [0] "a slot is active", [2 .. 25] the 12 counters (64 bit).  Per slot:
// record index (2), logical mask (2), iteration, unsatisfied flag, state bits, error weight, difference flag, pad,
// then the syndrome bits [mw].
constexpr int QUANT_WG_WORDS = 32;
constexpr int QUANT_SLOT_HEAD = 10;
__host__ __device__ inline size_t quant_slot_words(int m)
{
    return ((size_t)QUANT_SLOT_HEAD + (((size_t)m + 31) >> 5) + 1) & ~(size_t)1;
}
// 32-bit words of one slot's messages (`wide`: int16, else int8)
__host__ __device__ inline size_t quant_msg_words(int E, bool wide)
{
    return ((size_t)E * (wide ? 2 : 1) + 3) >> 2;
}
// 32-bit words of P[n] and of every slot's V[n] and messages, rounded up to even: the words behind them hold 64-bit
// cells (record index, logical mask, counters) that take LDS atomics, which need their 8-byte alignment
__host__ __device__ inline size_t quant_state_words(int n, int E, int S, bool wide)
{
    return ((size_t)n + (size_t)S * ((size_t)n + quant_msg_words(E, wide)) + 1) & ~(size_t)1;
}
// Dynamic LDS of one workgroup with S slots: P[n], then per slot V[n] and the messages, then the words
__host__ __device__ inline size_t quant_lds_bytes(int m, int n, int E, int S, bool wide)
{
    return 4 * (quant_state_words(n, E, S, wide) + (size_t)QUANT_WG_WORDS + (size_t)S * quant_slot_words(m));
}

enum : unsigned { QUANT_ACTIVE = 1u, QUANT_FRESH = 2u, QUANT_FROZEN = 4u };

// Rule 1: 0 for a NaN, else clamp(rint(prior * scale), -M, M) -- one multiply, round half to even, +-inf clamp
__device__ __forceinline__ int quant_prior(double prior, double scale, int M)
{
    const double x = prior * scale;
    if (x != x) return 0;
    const double r = __builtin_rint(x);
    if (r >= (double)M) return M;
    if (r <= -(double)M) return -M;
    return (int)r;
}

template <typename MsgT, bool MC>
__global__ __launch_bounds__(QUANT_THREADS) void bp_quant_kernel(const QuantParams P)
{
    extern __shared__ __attribute__((aligned(16))) int quant_smem[];
    constexpr bool WIDE = sizeof(MsgT) == 2;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = P.m, n = P.n, E = P.E, S = P.S;
    const int mwords = (int)quant_msg_words(E, WIDE);
    const int stride = n + mwords;                          // words of a slot: V, then the messages
    const int mw = (m + 31) >> 5;
    const int sw = (int)quant_slot_words(m);
    int* const prior_q = quant_smem;                        // [n]
    int* const slots = prior_q + n;                         // [S][n + mwords]
    auto s_V = [&](int s) { return slots + (size_t)s * stride; };
    auto s_msg = [&](int s) { return reinterpret_cast<MsgT*>(slots + (size_t)s * stride + n); };
    unsigned* const words = reinterpret_cast<unsigned*>(quant_smem + quant_state_words(n, E, S, WIDE));   // (8-byte aligned)
    unsigned long long* const cnt = reinterpret_cast<unsigned long long*>(words + 2);      // [12]
    unsigned* const sl = words + QUANT_WG_WORDS;            // [S][sw]
    auto s_rec = [&](int s) { return reinterpret_cast<long long*>(sl + s * sw); };
    auto s_lmask = [&](int s) { return reinterpret_cast<unsigned long long*>(sl + s * sw + 2); };
    auto s_it = [&](int s) { return reinterpret_cast<int*>(sl + s * sw + 4); };
    auto s_unsat = [&](int s) { return sl + s * sw + 5; };
    auto s_state = [&](int s) { return sl + s * sw + 6; };
    auto s_weight = [&](int s) { return reinterpret_cast<int*>(sl + s * sw + 7); };
    auto s_diff = [&](int s) { return reinterpret_cast<int*>(sl + s * sw + 8); };
    auto s_syn = [&](int s) { return sl + s * sw + QUANT_SLOT_HEAD; };

    const int M = P.M, anum = P.alpha_num, ashift = P.alpha_shift, beta = P.beta;
    const long long count = P.B;
    const bool force = !MC && (P.flags & QUANT_FORCE_FULL) != 0;
    const int last_it = P.max_iter - 1;

    for (int v = tid; v < n; v += nt) prior_q[v] = quant_prior(P.prior[v], P.scale, M);
    if (tid < QUANT_WG_WORDS) words[tid] = 0u;
    if (tid < S) {
        const long long rec = (long long)blockIdx.x * S + tid;
        const bool have = rec < count;
        *s_rec(tid) = have ? rec : -1;
        *s_lmask(tid) = 0ull;
        *s_it(tid) = 0; *s_unsat(tid) = 0u; *s_weight(tid) = 0; *s_diff(tid) = 0;
        *s_state(tid) = have ? (QUANT_ACTIVE | QUANT_FRESH) : 0u;
    }
    __syncthreads();
    if ((long long)blockIdx.x * S >= count) return;         // (uniform: no record for this workgroup)

    for (;;) {
        // ================= fresh slots: Q = P on every edge, the syndrome bits ======================================
        for (int s = 0; s < S; ++s) {
            if (!(*s_state(s) & QUANT_FRESH)) continue;     // uniform
            MsgT* const msg = s_msg(s);
            for (int e = tid; e < E; e += nt) msg[e] = (MsgT)prior_q[P.col_idx[e]];
            const long long rec = *s_rec(s);
            unsigned* const synw = s_syn(s);
            for (int c0 = tid - lane; c0 < m; c0 += nt) {   // c0 is wave-uniform
                const int c = c0 + lane;
                unsigned bit = 0u;
                if (c < m) {
                    if constexpr (MC) {
                        const uint8_t* const err = P.errors_in + rec * n;
                        for (int e = P.row_ptr[c]; e < P.row_ptr[c + 1]; ++e) bit ^= err[P.col_idx[e]] & 1u;
                    } else {
                        bit = P.syndromes[rec * m + c] & 1u;
                    }
                }
                const unsigned long long mask = __ballot(bit != 0u);
                if (lane == 0) {
                    const int wi = c0 >> 5;
                    synw[wi] = (unsigned)mask;
                    if (wi + 1 < mw) synw[wi + 1] = (unsigned)(mask >> 32);
                }
            }
        }
        __syncthreads();
        if (tid < S) *s_state(tid) &= ~QUANT_FRESH;         // (read again only after the next barrier)

        // ================= check step: R over Q, row by row ==========================================================
        for (int i = tid; i < S * m; i += nt) {
            const int s = i / m, c = i - s * m;
            if (!(*s_state(s) & QUANT_ACTIVE)) continue;
            const int e0 = P.row_ptr[c], e1 = P.row_ptr[c + 1];
            MsgT* const msg = s_msg(s);
            // the two smallest magnitudes (M if the row has no such entry), the first place of the smallest, the parity
            // of the negative entries
            int min1 = M, min2 = M, at = -1;
            unsigned par = (s_syn(s)[c >> 5] >> (c & 31)) & 1u;
            for (int e = e0; e < e1; ++e) {
                const int q = msg[e];
                const int a = q < 0 ? -q : q;
                par ^= q < 0 ? 1u : 0u;
                if (a < min1) { min2 = min1; min1 = a; at = e; }
                else if (a < min2) min2 = a;
            }
            int r1 = ((min1 * anum) >> ashift) - beta;      // mag' of every entry but `at`
            int r2 = ((min2 * anum) >> ashift) - beta;      // mag' of `at`
            r1 = r1 < 0 ? 0 : r1;
            r2 = r2 < 0 ? 0 : r2;
            for (int e = e0; e < e1; ++e) {
                const int q = msg[e];
                const unsigned neg = par ^ (q < 0 ? 1u : 0u);
                const int mag = e == at ? r2 : r1;
                msg[e] = (MsgT)(neg ? -mag : mag);
            }
        }
        __syncthreads();

        // ================= variable step: V = P + the column's R, Q = clamp(V - R) over R ===========================
        for (int i = tid; i < S * n; i += nt) {
            const int s = i / n, v = i - s * n;
            if (!(*s_state(s) & QUANT_ACTIVE)) continue;
            const int k0 = P.col_ptr[v], k1 = P.col_ptr[v + 1];
            MsgT* const msg = s_msg(s);
            int sum = prior_q[v];
            for (int k = k0; k < k1; ++k) sum += msg[P.col_edge[k]];
            s_V(s)[v] = sum;
            for (int k = k0; k < k1; ++k) {
                const int e = P.col_edge[k];
                int q = sum - msg[e];
                q = q > M ? M : q;
                q = q < -M ? -M : q;
                msg[e] = (MsgT)q;
            }
        }
        __syncthreads();

        // ================= syndrome test: H (V < 0) == s, by row gather ==========================================
        for (int i = tid; i < S * m; i += nt) {
            const int s = i / m, c = i - s * m;
            if (!(*s_state(s) & QUANT_ACTIVE)) continue;
            const int* const V = s_V(s);
            unsigned par = (s_syn(s)[c >> 5] >> (c & 31)) & 1u;
            for (int e = P.row_ptr[c]; e < P.row_ptr[c + 1]; ++e) par ^= V[P.col_idx[e]] < 0 ? 1u : 0u;
            if (par) *s_unsat(s) = 1u;                      // (every writer stores the same value)
        }
        if (tid == 0) words[0] = 0u;
        __syncthreads();

        // ================= slot turnover, part 1 (all threads): the outputs of the slots that emit ================
        for (int s = 0; s < S; ++s) {
            const unsigned st = *s_state(s);
            if (!(st & QUANT_ACTIVE) || (st & QUANT_FROZEN)) continue;          // uniform
            const bool solved = *s_unsat(s) == 0u;
            if (!solved && *s_it(s) < last_it) continue;
            const long long rec = *s_rec(s);
            const int* const V = s_V(s);
            if constexpr (MC) {
                const bool to_osd = P.fail_list != nullptr && !solved;
                const uint8_t* const err = P.errors_in + rec * n;
                unsigned long long lm = 0ull;
                int ew = 0, df = 0;
                for (int v = tid; v < n; v += nt) {
                    const int val = V[v];
                    const unsigned hd = val < 0 ? 1u : 0u;
                    const unsigned e = err[v] & 1u;
                    if (to_osd) {
                        P.fail_llr[rec * n + v] = (double)val;
                        P.fail_hard[rec * n + v] = (uint8_t)hd;
                        P.fail_err[rec * n + v] = (uint8_t)e;
                    } else {
                        const unsigned res = hd ^ e;
                        ew += (int)e;
                        df |= (int)res;
                        if (res) lm ^= P.lx_cols[v];
                    }
                }
                if (to_osd) {
                    for (int c = tid; c < m; c += nt) P.fail_syn[rec * m + c] = (uint8_t)((s_syn(s)[c >> 5] >> (c & 31)) & 1u);
                } else {
                    if (lm) atomicXor(s_lmask(s), lm);
                    if (ew) atomicAdd(s_weight(s), ew);
                    if (df) atomicOr(s_diff(s), 1);
                }
            } else {
                for (int v = tid; v < n; v += nt) {
                    const int val = V[v];
                    if (P.posterior_q) P.posterior_q[rec * n + v] = val;
                    if (P.llr) P.llr[rec * n + v] = (double)val;
                    if (P.hard) P.hard[rec * n + v] = (uint8_t)(val < 0 ? 1 : 0);
                }
            }
        }
        __syncthreads();

        // ================= slot turnover, part 2 (one thread per slot): flags, counters, the next record ==========
        if (tid < S) {
            const int s = tid;
            const unsigned st = *s_state(s);
            if (st & QUANT_ACTIVE) {
                const bool solved = *s_unsat(s) == 0u;
                const int it = *s_it(s);
                const bool last = it >= last_it;
                const bool frozen = (st & QUANT_FROZEN) != 0u;
                const long long rec = *s_rec(s);
                if (!frozen && (solved || last)) {
                    if constexpr (MC) {
                        if (P.fail_list != nullptr && !solved) {
                            P.fail_list[atomicAdd(P.fail_count, 1ull)] = rec;
                            atomicAdd(cnt + 0, 1ull); atomicAdd(cnt + 6, 1ull);       // BP bookkeeping only
                            atomicAdd(cnt + 7, (unsigned long long)it);
                        } else {
                            int row[NUM_COUNTERS];
#pragma unroll
                            for (int i = 0; i < NUM_COUNTERS; ++i) row[i] = 0;
                            mc_count_trial(row, *s_lmask(s), *s_weight(s), *s_diff(s), solved ? 1 : 0, it, P.half_distance);
                            *s_lmask(s) = 0ull; *s_weight(s) = 0; *s_diff(s) = 0;
#pragma unroll
                            for (int i = 0; i < NUM_COUNTERS; ++i)
                                if (row[i]) atomicAdd(cnt + i, (unsigned long long)row[i]);
                        }
                    } else {
                        if (P.converged) P.converged[rec] = (uint8_t)(solved ? 1 : 0);
                        if (P.iters) P.iters[rec] = it;
                    }
                }
                *s_unsat(s) = 0u;
                if (last || (solved && !force)) {
                    // the record is done: the next one, if any
                    const long long next = (long long)gridDim.x * S + (long long)atomicAdd(P.work_counter, 1u);
                    const bool have = next < count;
                    *s_rec(s) = have ? next : -1;
                    *s_it(s) = 0;
                    *s_state(s) = have ? (QUANT_ACTIVE | QUANT_FRESH) : 0u;
                    if (have) words[0] = 1u;
                } else {
                    *s_it(s) = it + 1;
                    if (solved) *s_state(s) = st | QUANT_FROZEN;         // (forced: outputs stay those of this iteration)
                    words[0] = 1u;
                }
            }
        }
        __syncthreads();
        if (!words[0]) break;                               // uniform
    }
    if constexpr (MC) {
        if (tid < NUM_COUNTERS && cnt[tid])
            atomicAdd(reinterpret_cast<unsigned long long*>(P.counters + tid), cnt[tid]);
    }
}

}  // namespace qbp
