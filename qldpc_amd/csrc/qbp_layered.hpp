// Layered (check-serial) BP: the checks are visited one after another in a fixed order, and each sees the posteriors
// its predecessors of the same iteration just updated (include/qbp.h, qbp_layered_configure, states the rules;
// tests/layered_oracle.py is the numpy statement the kernel is compared with bit for bit).
//
// What runs is the level form of that statement: the level of a check is 1 + the largest level of the checks that
// share a variable with it and come earlier in the order.  Checks of one level share no variable, every ordered pair
// of conflicting checks keeps its order, so level after level -- all checks of a level at once -- computes the
// sequential statement bit for bit (qbp_layered_plan builds the levels on the host).
//
// One workgroup decodes S records at once ("slots").  Per slot in LDS: one check->variable message R per edge (CSR
// order), the posterior V[n], the syndrome bits and a few words of bookkeeping; shared by the workgroup: the prior and,
// for sum-product, numpy's function tables at LDS address 0.  The level tables and the CSR arrays are read from
// global memory (they are the same few KB for every workgroup and stay in L2 / the scalar cache).
//   level step     a work item is (slot, check of the level), items padded to whole wavefronts per level: gather
//                  d = V - R, run check_row (rows of weight <= 8, in registers) and write R = r, V = d + r back; rows
//                  beyond 8 take a two-pass loop in the same thread (minsum_row / sp_message), recomputing d;
//   -- one barrier per level --
//   syndrome test  once per iteration, by row gather: a work item is (slot, check);
//   -- barrier --
//   slot turnover  a slot whose record has converged or run out of iterations writes its outputs (or classifies its
//                  trial) and takes the next record from a global counter: early exit is per record, and nothing a
//                  record computes depends on S, the grid or its neighbours.
// Two builds: MC = false decodes B syndromes to outputs; MC = true reads stored errors [T][n], forms the syndromes,
// decodes and classifies with mc_count_trial, or leaves the failure records the OSD and Relay record kernels read.
//
// Two memory layouts (QBP_OPT_LAYERED_MEM).  LARGE = false: everything above in LDS.  LARGE = true, for matrices whose
// single-slot state passes 160 KiB: the R of slot s in the workgroup's slice of a global workspace,
// wsR[blockIdx.x][S][E] in CSR order, the prior read in place when a slot turns fresh; V[S][n], the syndrome bits, the
// slot words and the tables stay in LDS.  The item -> (slot, check) mapping of a level is the same in every iteration,
// so a row's messages are read and written by one and the same thread for the whole launch: no other thread ever
// touches them, and nothing orders global memory between threads.  A fresh slot's slice is not zeroed; its first
// iteration reads R as +0.0 instead (V - (+0.0): the same bits), so the previous record's messages are never seen.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_check.hpp"
#include "qbp_mc.hpp"

namespace qbp {

constexpr int LAYERED_THREADS = 256;
constexpr int LAYERED_MAX_SLOTS = 32;
constexpr unsigned LAYERED_FORCE_FULL = 1u;        // QBP_FLAG_FORCE_FULL

struct LayeredParams {
    int m, n, E, n_levels, S;
    const int32_t* row_ptr;         // [m + 1] CSR
    const int32_t* col_idx;         // [E]
    const int32_t* order;           // [m] the checks, level after level
    const int32_t* level_ptr;       // [n_levels + 1] into order
    const double* prior;            // [n]
    unsigned* work_counter;         // zeroed before launch: index - grid * S of the next record
    int max_iter;
    unsigned flags;                 // LAYERED_FORCE_FULL (batch build only)
    double alpha, clip_llr;
    long long B;                    // records (batch build) or trials (Monte-Carlo build)
    // ---- batch build: syndromes in, outputs out (any output may be null) ----------------------------------------
    const uint8_t* syndromes;       // [B][m]
    uint8_t* hard;                  // [B][n]
    uint8_t* converged;             // [B]
    int32_t* iters;                 // [B]
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
    // ---- large build ------------------------------------------------------------------------------------------------
    double* wsR;                    // [grid][S][E] messages (null in the LDS build)
};

// 32-bit words behind the doubles.  Workgroup: [0] "a slot is active", [2 .. 25] the 12 counters (64 bit).  Per slot:
// record index (2), logical mask (2), iteration, unsatisfied flag, state bits, error weight, difference flag, pad,
// then the syndrome bits [mw].
constexpr int LAYERED_WG_WORDS = 32;
constexpr int LAYERED_SLOT_HEAD = 10;
__host__ __device__ inline size_t layered_slot_words(int m)
{
    return ((size_t)LAYERED_SLOT_HEAD + (((size_t)m + 31) >> 5) + 1) & ~(size_t)1;
}
// Dynamic LDS of one workgroup with S slots (tables: sum-product only)
__host__ __device__ inline size_t layered_lds_bytes(int m, int n, int E, int S, bool tables)
{
    return (tables ? (size_t)NP_LDS_BYTES : 0) + 8 * ((size_t)n + (size_t)S * ((size_t)E + (size_t)n)) +
           4 * ((size_t)LAYERED_WG_WORDS + (size_t)S * layered_slot_words(m));
}

// The large build: V[S][n] and the words; R in the workspace, no copy of the prior
__host__ __device__ inline size_t layered_large_lds_bytes(int m, int n, int S, bool tables)
{
    return (tables ? (size_t)NP_LDS_BYTES : 0) + 8 * (size_t)S * (size_t)n +
           4 * ((size_t)LAYERED_WG_WORDS + (size_t)S * layered_slot_words(m));
}

enum : unsigned { LAYERED_ACTIVE = 1u, LAYERED_FRESH = 2u, LAYERED_FROZEN = 4u };

template <int VARIANT, bool MC, bool LARGE>
__global__ __launch_bounds__(LAYERED_THREADS) void bp_layered_kernel(const LayeredParams P)
{
    static_assert(VARIANT == 0 || VARIANT == 2, "sum-product or min-sum");
    extern __shared__ __attribute__((aligned(16))) double layered_smem[];
    constexpr NpT np_tab = 0u;          // the tables of tanh / arctanh sit at LDS address 0 (sum-product)
    constexpr int TAB = VARIANT == 0 ? NP_LDS_DOUBLES : 0;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = P.m, n = P.n, E = P.E, S = P.S;
    const int stride = LARGE ? n : E + n;                   // doubles of a slot in LDS
    const int mw = (m + 31) >> 5;
    const int sw = (int)layered_slot_words(m);
    double* const prior_l = layered_smem + TAB;            // [n] (LDS build only)
    double* const slots = prior_l + (LARGE ? 0 : n);        // [S][E + n]: R, then V; large build [S][n]: V
    // the messages and the posterior of slot s
    auto s_R = [&](int s) {
        if constexpr (LARGE) return P.wsR + ((size_t)blockIdx.x * S + s) * (size_t)E;
        else return slots + (size_t)s * stride;
    };
    auto s_V = [&](int s) { return slots + (size_t)s * stride + (LARGE ? 0 : E); };
    unsigned* const words = reinterpret_cast<unsigned*>(slots + (size_t)S * stride);
    unsigned long long* const cnt = reinterpret_cast<unsigned long long*>(words + 2);      // [12]
    unsigned* const sl = words + LAYERED_WG_WORDS;          // [S][sw]
    auto s_rec = [&](int s) { return reinterpret_cast<long long*>(sl + s * sw); };
    auto s_lmask = [&](int s) { return reinterpret_cast<unsigned long long*>(sl + s * sw + 2); };
    auto s_it = [&](int s) { return reinterpret_cast<int*>(sl + s * sw + 4); };
    auto s_unsat = [&](int s) { return sl + s * sw + 5; };
    auto s_state = [&](int s) { return sl + s * sw + 6; };
    auto s_weight = [&](int s) { return reinterpret_cast<int*>(sl + s * sw + 7); };
    auto s_diff = [&](int s) { return reinterpret_cast<int*>(sl + s * sw + 8); };
    auto s_syn = [&](int s) { return sl + s * sw + LAYERED_SLOT_HEAD; };

    const double clip = P.clip_llr;
    const long long count = P.B;
    const bool force = !MC && (P.flags & LAYERED_FORCE_FULL) != 0;
    const int last_it = P.max_iter - 1;

    if constexpr (VARIANT == 0) np_tables_to_lds(layered_smem, tid, nt);
    if constexpr (!LARGE)
        for (int x = tid; x < n; x += nt) prior_l[x] = P.prior[x];
    if (tid < LAYERED_WG_WORDS) words[tid] = 0u;
    if (tid < S) {
        const long long rec = (long long)blockIdx.x * S + tid;
        const bool have = rec < count;
        *s_rec(tid) = have ? rec : -1;
        *s_lmask(tid) = 0ull;
        *s_it(tid) = 0; *s_unsat(tid) = 0u; *s_weight(tid) = 0; *s_diff(tid) = 0;
        *s_state(tid) = have ? (LAYERED_ACTIVE | LAYERED_FRESH) : 0u;
    }
    __syncthreads();
    if ((long long)blockIdx.x * S >= count) return;         // (uniform: no record for this workgroup)

    // np.clip of a variable->check message (min-sum): a NaN stays a NaN
    auto clipq = [&](double q) {
        const double y = q < -clip ? -clip : q;
        return y > clip ? clip : y;
    };

    for (;;) {
        // ================= fresh slots: R = +0.0 (large build: read as +0.0 in iteration 0), V = prior, the syndrome
        // bits =========================================================================================================
        for (int s = 0; s < S; ++s) {
            if (!(*s_state(s) & LAYERED_FRESH)) continue;   // uniform
            if constexpr (LARGE) {
                double* const V = s_V(s);
                for (int k = tid; k < n; k += nt) V[k] = P.prior[k];
            } else {
                double* const R = s_R(s);
                for (int k = tid; k < stride; k += nt) R[k] = k < E ? 0.0 : prior_l[k - E];
            }
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
        if (tid < S) *s_state(tid) &= ~LAYERED_FRESH;       // (read again only after the next barrier)

        // ================= one iteration: level after level ========================================================
        for (int l = 0; l < P.n_levels; ++l) {
            const int lp = P.level_ptr[l], cl = P.level_ptr[l + 1] - lp;
            const int items = S * cl;
            for (int i = tid; i < items; i += nt) {
                const int s = i / cl, k = i - s * cl;
                if (!(*s_state(s) & LAYERED_ACTIVE)) continue;
                const int c = P.order[lp + k];
                const int e0 = P.row_ptr[c], deg = P.row_ptr[c + 1] - e0;
                double* const R = s_R(s) + e0;                  // the row's messages
                double* const V = s_V(s);
                // (large build: in iteration 0 the slice still holds the previous record's messages)
                const bool first = LARGE && *s_it(s) == 0;
                auto rd = [&](int j) {
                    if constexpr (LARGE) return first ? 0.0 : R[j];
                    else return R[j];
                };
                const int32_t* const col = P.col_idx + e0;
                const unsigned sbit = (s_syn(s)[c >> 5] >> (c & 31)) & 1u;
#define QBP_LAYERED_ROW(DD)                                                                        \
                case DD: {                                                                         \
                    int vv[DD];                                                                    \
                    double d[DD], q[DD];                                                           \
                    _Pragma("unroll") for (int j = 0; j < DD; ++j) vv[j] = col[j];                 \
                    _Pragma("unroll") for (int j = 0; j < DD; ++j) d[j] = V[vv[j]] - rd(j);        \
                    _Pragma("unroll") for (int j = 0; j < DD; ++j) q[j] = VARIANT == 2 ? clipq(d[j]) : d[j]; \
                    auto put = [&](int j, double r) { R[j] = r; V[vv[j]] = d[j] + r; };            \
                    check_row<VARIANT, DD, true>(q, sbit, P.alpha, true, np_tab, put);             \
                } break;
                switch (deg) {
                    case 0: break;
                    QBP_LAYERED_ROW(1) QBP_LAYERED_ROW(2) QBP_LAYERED_ROW(3) QBP_LAYERED_ROW(4)
                    QBP_LAYERED_ROW(5) QBP_LAYERED_ROW(6) QBP_LAYERED_ROW(7) QBP_LAYERED_ROW(8)
                    default: {
                        // rows beyond 8: two passes in this thread, d recomputed (the row's variables are distinct,
                        // and message j is overwritten only after its own d was read)
                        if constexpr (VARIANT == 2) {
                            const MinSumRow row = minsum_row([&](int j) { return clipq(V[col[j]] - rd(j)); }, deg);
                            for (int j = 0; j < deg; ++j) {
                                const int v = col[j];
                                const double dj = V[v] - rd(j);
                                const double r = minsum_message(clipq(dj), row, sbit, P.alpha);
                                R[j] = r; V[v] = dj + r;
                            }
                        } else {
                            double prod = 0.0;
                            for (int j = 0; j < deg; ++j) {
                                const double t = tanh_half_msg<VARIANT>(V[col[j]] - rd(j), np_tab);
                                prod = (j == 0) ? t : prod * t;
                            }
                            for (int j = 0; j < deg; ++j) {
                                const int v = col[j];
                                const double dj = V[v] - rd(j);
                                const double r = sp_message<VARIANT>(prod, tanh_half_msg<VARIANT>(dj, np_tab), sbit, np_tab);
                                R[j] = r; V[v] = dj + r;
                            }
                        }
                    } break;
                }
#undef QBP_LAYERED_ROW
            }
            __syncthreads();
        }

        // ================= syndrome test: H (V < 0) == s, by row gather ==========================================
        for (int i = tid; i < S * m; i += nt) {
            const int s = i / m, c = i - s * m;
            if (!(*s_state(s) & LAYERED_ACTIVE)) continue;
            const double* const V = s_V(s);
            unsigned par = (s_syn(s)[c >> 5] >> (c & 31)) & 1u;
            for (int e = P.row_ptr[c]; e < P.row_ptr[c + 1]; ++e) par ^= V[P.col_idx[e]] < 0.0 ? 1u : 0u;
            if (par) *s_unsat(s) = 1u;                      // (every writer stores the same value)
        }
        if (tid == 0) words[0] = 0u;
        __syncthreads();

        // ================= slot turnover, part 1 (all threads): the outputs of the slots that emit ================
        for (int s = 0; s < S; ++s) {
            const unsigned st = *s_state(s);
            if (!(st & LAYERED_ACTIVE) || (st & LAYERED_FROZEN)) continue;      // uniform
            const bool solved = *s_unsat(s) == 0u;
            if (!solved && *s_it(s) < last_it) continue;
            const long long rec = *s_rec(s);
            const double* const V = s_V(s);
            if constexpr (MC) {
                const bool to_osd = P.fail_list != nullptr && !solved;
                const uint8_t* const err = P.errors_in + rec * n;
                unsigned long long lm = 0ull;
                int ew = 0, df = 0;
                for (int v = tid; v < n; v += nt) {
                    const double val = V[v];
                    const unsigned hd = val < 0.0 ? 1u : 0u;
                    const unsigned e = err[v] & 1u;
                    if (to_osd) {
                        P.fail_llr[rec * n + v] = val;
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
                    const double val = V[v];
                    if (P.llr) P.llr[rec * n + v] = val;
                    if (P.hard) P.hard[rec * n + v] = (uint8_t)(val < 0.0 ? 1 : 0);
                }
            }
        }
        __syncthreads();

        // ================= slot turnover, part 2 (one thread per slot): flags, counters, the next record ==========
        if (tid < S) {
            const int s = tid;
            const unsigned st = *s_state(s);
            if (st & LAYERED_ACTIVE) {
                const bool solved = *s_unsat(s) == 0u;
                const int it = *s_it(s);
                const bool last = it >= last_it;
                const bool frozen = (st & LAYERED_FROZEN) != 0u;
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
                    *s_state(s) = have ? (LAYERED_ACTIVE | LAYERED_FRESH) : 0u;
                    if (have) words[0] = 1u;
                } else {
                    *s_it(s) = it + 1;
                    if (solved) *s_state(s) = st | LAYERED_FROZEN;       // (forced: outputs stay those of this iteration)
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
