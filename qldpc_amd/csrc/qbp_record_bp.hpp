// The per-record BP iteration with the messages in LDS, stated once for bp_relay_kernel (qbp_relay.hpp),
// bp_gd_kernel (qbp_gd.hpp) and bp_cond_kernel (qbp_cond.hpp).
//
// The kernels run one workgroup per record on the tables of the general-H kernel (qbp_generic.hpp: class-blocked,
// transposed message layout; srow / epos / vpos / vrow / svar), on ONE array of E messages updated in place -- a slot
// holds the variable->check message before the check step and the check->variable message after it -- with two
// workgroup barriers per iteration, which stay in the kernels' own loops:
//   record_check_step_minsum  one thread per check of weight <= 8 (check_row of qbp_check.hpp), rows beyond that in passes;
//   record_check_step_sumproduct  the same for the exact sum-product row (bp_cond_kernel);
//   -- barrier A --
//   record_variable_step   one thread per variable: V = colsum(R) + bias (ascending check), Q = V - R in place, and the
//                          incremental syndrome test of the general-H kernel (parity bits in LDS, a counter of
//                          unsatisfied checks);
//   -- barrier B --
//   counter zero <=> H hard == s.
// Around the iteration: the parameter blocks the kernels embed (RecordTables, RecordIo), the record prologue
// (record_load_syndrome, record_prior_to_edges), the classification of a Monte-Carlo failure record (record_classify),
// the hand-out of the next record (record_next_item) and the workgroup size (record_threads).
// What a kernel keeps for itself: its LDS carve-up (it fills a RecordLds), its loop around the iteration (legs, rounds),
// the bias of the variable step and its batch outputs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_check.hpp"
#include "qbp_generic.hpp"
#include "qbp_mc.hpp"

namespace qbp {

// The tables of the general-H kernel (GenericParams has the layout), and what every launch on them needs
struct RecordTables {
    int m, n, E;
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
};

// Where the records come from and where the results go
struct RecordIo {
    // ---- batch build: syndromes in, outputs out (any output may be null) ----------------------------------------
    const uint8_t* syndromes;       // [B][m]
    long long B;
    uint8_t* hard;                  // [B][n]
    uint8_t* converged;             // [B]
    int32_t* iters;                 // [B] iterations executed
    double* llr;                    // [B][n]
    // ---- records build: the failure records of a Monte-Carlo launch --------------------------------------------------
    const unsigned long long* fail_count;   // number of records (device)
    const long long* fail_list;     // record index of item i
    const uint8_t* fail_syn;        // [*][m]
    const uint8_t* fail_err;        // [*][n]
    const unsigned long long* lx_cols;
    int half_distance;
    long long* counters;
};

// The LDS of one workgroup that the shared steps read and write (each kernel carves it: relay_lds_words, gd_lds_words)
struct RecordLds {
    double* M;                      // [E] messages, in place
    double* V;                      // [n] posterior values, sorted-variable order
    unsigned long long* mc_lmask;   // records build: logical mask, error weight, difference flag of the current record
    int* mc_weight;
    int* mc_diff;
    int* unsat;                     // [2] set bits of par, by iteration parity
    unsigned* next_item;
    unsigned* synw;                 // [mw] syndrome bits, sorted check order
    unsigned* par;                  // [2][mw] parity of H hard ^ s
};

// The tables of tanh / arctanh sit at LDS address 0 (sum-product); min-sum reads no table
constexpr NpT RECORD_NP_TAB = 0u;

// Threads of a workgroup: the larger of the two steps' padded work in equal passes of at most max_threads
// ([[144,12,12]]: 192, [[288,12,18]]: 320)
__host__ inline int record_threads(int check_items, int var_items, int max_threads)
{
    int work = check_items > var_items ? check_items : var_items;
    if (work < 64) work = 64;
    const int passes = (work + max_threads - 1) / max_threads;
    return (((work + passes - 1) / passes) + 63) / 64 * 64;
}

// Kernel start: the classification words, and the number of records of the launch
template <bool RECORDS>
__device__ __forceinline__ long long record_count(const RecordIo& io, const RecordLds& S)
{
    if constexpr (RECORDS) {
        if (threadIdx.x == 0) { *S.mc_lmask = 0ull; *S.mc_weight = 0; *S.mc_diff = 0; }
        return (long long)*io.fail_count;
    } else {
        return io.B;
    }
}

// Record start: syndrome bits in sorted check order, parity buffer 0 := syndrome, unsat[0] := its weight (published by
// the caller's next barrier).  Returns the record's index.
template <bool RECORDS>
__device__ __forceinline__ long long record_load_syndrome(const RecordTables& G, const RecordIo& io, const RecordLds& S,
                                                          long long item)
{
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = G.m, mw = (m + 31) >> 5;
    const long long rec = RECORDS ? io.fail_list[item] : item;
    const uint8_t* const syn = RECORDS ? io.fail_syn + rec * m : io.syndromes + rec * m;
    if (tid == 0) S.unsat[0] = 0;
    __syncthreads();      // (also: what the kernel put in LDS before its record loop; the previous record's last readers
                          //  of LDS are done)
    int cnt = 0;
    for (int w0 = tid - lane; w0 < m; w0 += nt) {           // w0 is wave-uniform
        const int w = w0 + lane;
        const unsigned bit = w < m ? (syn[G.srow[w]] & 1u) : 0u;
        const unsigned long long mask = __ballot(bit != 0);
        if (lane == 0) {
            const int wi = w0 >> 5;
            S.synw[wi] = (unsigned)mask; S.par[wi] = (unsigned)mask;
            if (wi + 1 < mw) { S.synw[wi + 1] = (unsigned)(mask >> 32); S.par[wi + 1] = (unsigned)(mask >> 32); }
            cnt += __builtin_popcountll(mask);
        }
    }
    if (lane == 0 && cnt) atomicAdd(&S.unsat[0], cnt);
    return rec;
}

// Rule 1 of both decoders: Q = prior on the edges.  prior[x]: the prior of the sorted variable x.  (The class search
// is generic_col_class of qbp_generic.hpp on these tables, written in place: through reference outputs it costs the
// kernels two registers.)
__device__ __forceinline__ void record_prior_to_edges(const RecordTables& G, const RecordLds& S, const double* prior)
{
    constexpr int CC = GENERIC_MAX_COL_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int first_lcol = G.col_off[CC + 1], n_lcol = G.col_off[CC + 2] - first_lcol;
    for (int x = tid + G.col_off[1]; x < first_lcol; x += nt) {
        int D, cnt, o;
        if (x < G.col_off[2])      { D = 1; cnt = G.col_off[2] - G.col_off[1]; o = G.col_base[1] + (x - G.col_off[1]); }
        else if (x < G.col_off[3]) { D = 2; cnt = G.col_off[3] - G.col_off[2]; o = G.col_base[2] + (x - G.col_off[2]); }
        else if (x < G.col_off[4]) { D = 3; cnt = G.col_off[4] - G.col_off[3]; o = G.col_base[3] + (x - G.col_off[3]); }
        else                       { D = 4; cnt = G.col_off[5] - G.col_off[4]; o = G.col_base[4] + (x - G.col_off[4]); }
        const double pv = prior[x];
        for (int j = 0; j < D; ++j) S.M[G.vpos[o + (size_t)j * cnt]] = pv;
    }
    for (int i = tid; i < n_lcol; i += nt) {
        const double pv = prior[first_lcol + i];
        for (int k = G.lcol_ptr[i]; k < G.lcol_ptr[i + 1]; ++k) S.M[G.vpos[k]] = pv;
    }
}

// ---- check step, min-sum: M := the check->variable messages -----------------------------------------------------------
// Lw: the workgroup's slice of wsL.  The caller's barrier A publishes the messages.  (The sum-product rows of
// bp_gd_kernel are the one statement of the iteration that stays in its kernel: qbp_gd.hpp says why.)
#define QBP_RECORD_ROW_CLASS(DD)                                                               \
        case DD: {                                                                             \
            const int cnt = G.row_off[DD + 1] - G.row_off[DD];                                 \
            const int i = wpu - G.rpad_off[DD] + lane_;                                        \
            if (i < cnt) {                                                                     \
                const int w = G.row_off[DD] + i;                                               \
                const unsigned sbit = (S.synw[w >> 5] >> (w & 31)) & 1u;                       \
                const int base = G.row_base[DD] + i;                                           \
                double q[DD];                                                                  \
                _Pragma("unroll") for (int j = 0; j < DD; ++j) q[j] = M[base + j * cnt];       \
                auto put = [&](int j, double v) { M[base + j * cnt] = v; };                    \
                check_row<VARIANT, DD, true>(q, sbit, alpha, true, RECORD_NP_TAB, put);        \
            }                                                                                  \
        } break;

// The checks of weight <= 8 of either rule (VARIANT 2: min-sum, 0: the exact sum-product row on numpy's tables)
template <int VARIANT>
__device__ __forceinline__ void record_check_rows(const RecordTables& G, const RecordLds& S, double alpha)
{
    constexpr int RC = GENERIC_MAX_ROW_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    double* const M = S.M;
    for (int wp0 = tid - lane; wp0 < G.rpad_off[RC + 1]; wp0 += nt) {
        // one wavefront = 64 consecutive work items of ONE weight class (scalar class search)
        const int wpu = __builtin_amdgcn_readfirstlane(wp0);
        int D = 1;
#pragma unroll
        for (int k = 2; k <= RC; ++k) D += wpu >= G.rpad_off[k] ? 1 : 0;
        int lane_ = lane;       // (opaque: keeps the per-class address arithmetic inside the loop)
        asm volatile("" : "+v"(lane_));
        switch (D) {
            QBP_RECORD_ROW_CLASS(1) QBP_RECORD_ROW_CLASS(2) QBP_RECORD_ROW_CLASS(3) QBP_RECORD_ROW_CLASS(4)
            QBP_RECORD_ROW_CLASS(5) QBP_RECORD_ROW_CLASS(6) QBP_RECORD_ROW_CLASS(7) QBP_RECORD_ROW_CLASS(8)
            default: break;
        }
    }
}
#undef QBP_RECORD_ROW_CLASS

__device__ __forceinline__ void record_check_step_minsum(const RecordTables& G, const RecordLds& S, double* Lw, double alpha)
{
    constexpr int RC = GENERIC_MAX_ROW_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x;
    double* const M = S.M;
    const int first_long = G.row_off[RC + 1], n_long = G.row_off[RC + 2] - first_long;
    const int lbase = G.row_base[RC + 1], n_ledges = G.E - lbase;
    record_check_rows<2>(G, S, alpha);
    // ---- checks of weight > 8: the minimum search one thread per check, the messages one per edge
    if (n_long > 0) {                                           // uniform
        for (int i = tid; i < n_long; i += nt) {
            const int deg = G.srow_deg[first_long + i];
            const int p0 = G.epos[G.srow_e0[first_long + i]];   // entries contiguous from here
            const MinSumRow row = minsum_row([&](int j) { return M[p0 + j]; }, deg);
            Lw[3 * i] = row.sprod; Lw[3 * i + 1] = row.min1; Lw[3 * i + 2] = row.min2;
        }
        __syncthreads();
        for (int k = tid; k < n_ledges; k += nt) {
            const int i = G.long_edge_row[k];
            const int w = first_long + i;
            const unsigned sbit = (S.synw[w >> 5] >> (w & 31)) & 1u;
            M[lbase + k] = minsum_message(M[lbase + k], MinSumRow{Lw[3 * i], Lw[3 * i + 1], Lw[3 * i + 2]}, sbit, alpha);
        }
    }
}

// ---- check step, sum-product: the same on numpy's tanh / arctanh tables (bp_cond_kernel; bp_gd_kernel states these rows
// in its own body: qbp_gd.hpp says why)
__device__ __forceinline__ void record_check_step_sumproduct(const RecordTables& G, const RecordLds& S, double* Lw,
                                                             double alpha)
{
    constexpr int RC = GENERIC_MAX_ROW_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x;
    double* const M = S.M;
    const int first_long = G.row_off[RC + 1], n_long = G.row_off[RC + 2] - first_long;
    const int lbase = G.row_base[RC + 1], n_ledges = G.E - lbase;
    record_check_rows<0>(G, S, alpha);
    // ---- checks of weight > 8: the per-edge work one thread per edge, the sequential part (np.prod in ascending column
    //      order) one thread per check
    if (n_long > 0) {                                           // uniform
        for (int k = tid; k < n_ledges; k += nt) M[lbase + k] = tanh_half_msg<0>(M[lbase + k], RECORD_NP_TAB);
        __syncthreads();
        for (int i = tid; i < n_long; i += nt) {
            const int deg = G.srow_deg[first_long + i];
            const int p0 = G.epos[G.srow_e0[first_long + i]];   // entries contiguous from here
            double prod = M[p0];
            for (int j = 1; j < deg; ++j) prod = prod * M[p0 + j];
            Lw[3 * i] = prod;
        }
        __syncthreads();
        for (int k = tid; k < n_ledges; k += nt) {
            const int i = G.long_edge_row[k];
            const int w = first_long + i;
            const unsigned sbit = (S.synw[w >> 5] >> (w & 31)) & 1u;
            M[lbase + k] = sp_message<0>(Lw[3 * i], M[lbase + k], sbit, RECORD_NP_TAB);
        }
    }
}

// ---- variable step + incremental syndrome test ----------------------------------------------------------------------
// Runs after barrier A.  V[x] = colsum(R) + bias_of(x), added in ascending check order; the new variable->check message
// of an edge is V - R (CLIP: clipped to +-clip), no damping term.  p = the iteration's parity: a variable whose hard
// decision is 1 flips its checks in parity buffer p, which was the syndrome, and unsat[p] follows; buffer p ^ 1 becomes
// the syndrome again for the next iteration.  After the caller's barrier B, unsat[p] == 0 <=> H hard == s.
#define QBP_RECORD_COL_CLASS(DD)                                                               \
        case DD: {                                                                             \
            const int cnt = G.col_off[DD + 1] - G.col_off[DD];                                 \
            const int i = xpu - G.cpad_off[DD] + lane_;                                        \
            if (i < cnt) {                                                                     \
                const int base = G.col_base[DD] + i;                                           \
                const int x = G.col_off[DD] + i;                                               \
                int o[DD];                                                                     \
                double r[DD];                                                                  \
                _Pragma("unroll") for (int j = 0; j < DD; ++j) o[j] = G.vpos[base + j * cnt];  \
                _Pragma("unroll") for (int j = 0; j < DD; ++j) r[j] = M[o[j]];                 \
                double s = r[0];                                                               \
                _Pragma("unroll") for (int j = 1; j < DD; ++j) s = s + r[j];                   \
                const double val = s + bias_of(x);                                             \
                V[x] = val;                                                                    \
                if (val < 0.0) {                                                               \
                    _Pragma("unroll") for (int j = 0; j < DD; ++j) flip(G.vrow[base + j * cnt]);   \
                }                                                                              \
                _Pragma("unroll") for (int j = 0; j < DD; ++j) M[o[j]] = q_of(val, r[j], o[j]); \
            }                                                                                  \
        } break;

// edge_rule (bp_cond_kernel's min-sum): edge_rule(o, q) is stored in slot o instead of q; the other kernels pass none.
struct RecordNoEdgeRule {};
template <bool CLIP, typename Bias, typename EdgeRule = RecordNoEdgeRule>
__device__ __forceinline__ void record_variable_step(const RecordTables& G, const RecordLds& S, int p, int syn_weight,
                                                     double clip, const Bias& bias_of,
                                                     const EdgeRule& edge_rule = EdgeRule{})
{
    constexpr bool EDGE_RULE = !__is_same(EdgeRule, RecordNoEdgeRule);
    constexpr int CC = GENERIC_MAX_COL_CLASS;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int mw = (G.m + 31) >> 5;
    double* const M = S.M;
    double* const V = S.V;
    const int first_lcol = G.col_off[CC + 1], n_lcol = G.col_off[CC + 2] - first_lcol;
    unsigned* const pbuf = S.par + p * mw;
    {   // the other buffer becomes the syndrome again (its last readers passed barrier A)
        unsigned* const obuf = S.par + (p ^ 1) * mw;
        for (int i = tid; i < mw; i += nt) obuf[i] = S.synw[i];
        if (tid == 0) S.unsat[p ^ 1] = syn_weight;
    }
    int delta = 0;
    auto flip = [&](int cw) {             // the check at sorted position cw changes parity
        const unsigned bit = 1u << (cw & 31);
        const unsigned old = atomicXor(&pbuf[cw >> 5], bit);
        delta += (old & bit) ? -1 : 1;
    };
    auto q_of = [&](double val, double r, int o) {
        double q = val - r;
        if constexpr (CLIP) {
            const double y = q < -clip ? -clip : q;
            q = y > clip ? clip : y;
        }
        if constexpr (EDGE_RULE) return (double)edge_rule(o, q); else return q;
    };
    for (int x = tid; x < G.col_off[1]; x += nt) V[x] = 0.0 + bias_of(x);     // no check: an empty column sum
    for (int xp0 = tid - lane; xp0 < G.cpad_off[CC + 1]; xp0 += nt) {
        const int xpu = __builtin_amdgcn_readfirstlane(xp0);
        int D = 1;
#pragma unroll
        for (int k = 2; k <= CC; ++k) D += xpu >= G.cpad_off[k] ? 1 : 0;
        int lane_ = lane;
        asm volatile("" : "+v"(lane_));
        switch (D) {
            QBP_RECORD_COL_CLASS(1) QBP_RECORD_COL_CLASS(2) QBP_RECORD_COL_CLASS(3) QBP_RECORD_COL_CLASS(4)
            default: break;
        }
    }
    for (int i = tid; i < n_lcol; i += nt) {
        const int k0 = G.lcol_ptr[i], k1 = G.lcol_ptr[i + 1];
        const int x = first_lcol + i;
        double s = 0.0;
        for (int k = k0; k < k1; ++k) {
            const double r = M[G.vpos[k]];
            s = (k == k0) ? r : s + r;                    // ascending check order
        }
        const double val = s + bias_of(x);
        V[x] = val;
        if (val < 0.0)
            for (int k = k0; k < k1; ++k) flip(G.vrow[k]);
        for (int k = k0; k < k1; ++k) {
            const int o = G.vpos[k];
            M[o] = q_of(val, M[o], o);
        }
    }
    if (delta) atomicAdd(&S.unsat[p], delta);
}
#undef QBP_RECORD_COL_CLASS

// ---- records build: classification of the result (paperResults_GPU.py:127-144), as the OSD record kernels do it: the
// first stage has counted the trial, its iterations and its not_converged.  hard_of(x): the hard decision (0u / 1u) of
// the sorted variable x; solved: it reproduces the syndrome.
template <typename Hard>
__device__ __forceinline__ void record_classify(const RecordTables& G, const RecordIo& io, const RecordLds& S,
                                                long long rec, bool solved, const Hard& hard_of)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = G.n;
    const uint8_t* const err = io.fail_err + rec * n;
    unsigned long long lm = 0ull;
    int ew = 0, df = 0;
    for (int x = tid; x < n; x += nt) {
        const int v = G.svar[x];
        const unsigned e = err[v] & 1u;
        const unsigned res = hard_of(x) ^ e;
        ew += (int)e;
        df |= (int)res;
        if (res) lm ^= io.lx_cols[v];
    }
    if (lm) atomicXor(S.mc_lmask, lm);
    if (ew) atomicAdd(S.mc_weight, ew);
    if (df) atomicOr(S.mc_diff, 1);
    __syncthreads();
    if (tid == 0) {
        int row[NUM_COUNTERS];
#pragma unroll
        for (int i = 0; i < NUM_COUNTERS; ++i) row[i] = 0;
        mc_count_trial(row, *S.mc_lmask, *S.mc_weight, *S.mc_diff, solved ? 1 : 0, 0, io.half_distance);
        *S.mc_lmask = 0ull; *S.mc_weight = 0; *S.mc_diff = 0;
        auto add = [&](int i) { atomicAdd(reinterpret_cast<unsigned long long*>(io.counters + i), 1ull); };
        if (row[5]) add(5);
        if (row[1]) { add(1); add(row[3] ? 3 : 4); add(8); }     // (every record is a trial BP left unconverged)
        if (row[9]) add(9);
        if (!solved) add(10);                                    // no solution: the output misses the syndrome
    }
}

// Record end: the workgroup's next item (`dynamic`: more records than workgroups, handed out through work_counter)
__device__ __forceinline__ long long record_next_item(const RecordTables& G, const RecordLds& S, bool dynamic)
{
    if (threadIdx.x == 0) *S.next_item = dynamic ? atomicAdd(G.work_counter, 1u) : 0x7fffffffu;
    __syncthreads();
    return (long long)gridDim.x + (long long)*S.next_item;      // (next write: after the barriers of the next record)
}

}  // namespace qbp
