// BP guided decimation (BPGD): rounds of flooding BP; a round that ends without a solution freezes the most reliable
// variable by overwriting its prior with +-decim_llr, and the next round continues on the same messages (include/qbp.h,
// qbp_gd_decode_batch, states the rules; tests/gd_oracle.py is the numpy statement the kernel is compared with bit
// for bit).
//
// One workgroup per record, the per-record BP iteration of qbp_record_bp.hpp (the tables of the general-H kernel, the
// messages in place in LDS) with two workgroup barriers per iteration:
//   check step     min-sum: record_check_step_minsum; sum-product: the exact row on numpy's tanh / arctanh tables,
//                  the one block stated in this file (its registers: see the kernel);
//   -- barrier A --
//   variable step  record_variable_step with bias = W, the working prior: V = colsum(R) + W (ascending check),
//                  Q = V - R in place (min-sum: clipped), and the incremental syndrome test;
//   -- barrier B --
//   counter zero <=> H hard == s: the record is done.
// This file has what is BPGD's own: the LDS carve-up, the round loop, the arg-max and the decimation, and the batch
// outputs.  The parameter blocks, the record prologue, the two steps, the classification of the records build and the
// hand-out of the next record are qbp_record_bp.hpp's, shared with bp_relay_kernel.
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
// Two memory layouts of each (QBP_OPT_GD_MEM): LARGE = false is the above; LARGE = true is the same statement for
// matrices whose E messages do not fit -- space-time and detector-error-model matrices.  Its messages are the
// workgroup's slice of a global workspace wsM[grid][E], as in bp_relay_kernel<RECORDS, true> (qbp_relay.hpp says what
// orders a store before the barrier with a load after it); the shared steps reach them through RecordLds::M and are
// called unchanged, the sum-product rows of this file go through the same pointer, and both barriers stay where they
// are.  W[n] is not stored: a decimated variable holds exactly +-decim_llr and every other its prior, so a second n-bit
// map (the sign) beside the decimated map states W, and the prior is read where the launch permuted it (prior_sorted).
// In LDS stay the tables, V[n] (the arg-max reads it), the words and the two maps: 8 n bytes + the words, 65 288 B for
// 2592 x 7776 (68 360 B with the tables).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_record_bp.hpp"

namespace qbp {

constexpr int GD_MAX_THREADS = 512;
constexpr int GD_MAX_WAVES = GD_MAX_THREADS / 64;

struct GdParams {
    RecordTables tab;
    RecordIo io;
    // ---- the configuration (qbp_gd_configure) -----------------------------------------------------------------------
    int iters_per_round, max_rounds;
    double decim_llr, alpha, clip_llr;
    // ---- batch build: the output beyond RecordIo's (may be null) ------------------------------------------------------
    int32_t* rounds;                // [B] variables decimated
    // ---- LARGE build -----------------------------------------------------------------------------------------------------
    double* wsM;                    // [grid][E] the messages of the workgroups' current records
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

// The same of the LARGE build: a second map [nw], the signs of the decimated variables
__host__ __device__ inline size_t gd_large_lds_words(int m, int n)
{
    const size_t mw = ((size_t)m + 31) >> 5, nw = ((size_t)n + 31) >> 5;
    return ((size_t)GD_HEAD_WORDS + 3 * mw + 2 * nw + 1) & ~(size_t)1;
}
// Dynamic LDS of one workgroup of the LARGE build: (sum-product) the function tables, V [n], the words
__host__ __device__ inline size_t gd_large_lds_bytes(int m, int n, bool tables)
{
    return (tables ? (size_t)NP_LDS_BYTES : 0) + (size_t)8 * (size_t)n + 4 * gd_large_lds_words(m, n);
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

// LARGE: the messages in the workgroup's slice of P.wsM, the working prior from the two maps and prior_sorted.
template <int VARIANT, bool RECORDS, bool LARGE = false>
__global__ __launch_bounds__(GD_MAX_THREADS) void bp_gd_kernel(const GdParams P)
{
    static_assert(VARIANT == 0 || VARIANT == 2, "sum-product or min-sum");
    extern __shared__ __attribute__((aligned(16))) double gd_smem[];
    constexpr int TAB = VARIANT == 0 ? NP_LDS_DOUBLES : 0;      // (the function tables: RECORD_NP_TAB)
    constexpr int RC = GENERIC_MAX_ROW_CLASS;
    const RecordTables& G = P.tab;
    const RecordIo& io = P.io;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int m = G.m, n = G.n, E = G.E;
    // [E] messages, in place
    double* const M = LARGE ? P.wsM + (size_t)blockIdx.x * (size_t)E : gd_smem + TAB;
    double* const V = LARGE ? gd_smem + TAB : M + E;    // [n] posterior values, sorted-variable order
    double* const Wp = V + n;                       // [n] working prior, sorted-variable order (not LARGE)
    unsigned* const words = reinterpret_cast<unsigned*>(LARGE ? V + n : Wp + n);
    const int mw = (m + 31) >> 5, nw = (n + 31) >> 5;
    unsigned long long* const am_bits = reinterpret_cast<unsigned long long*>(words + 8);      // [GD_MAX_WAVES]
    int* const am_var = reinterpret_cast<int*>(words + 8 + 2 * GD_MAX_WAVES);                  // [GD_MAX_WAVES]
    int* const am_pos = am_var + GD_MAX_WAVES;                                                 // [GD_MAX_WAVES]
    const RecordLds S{M, V, reinterpret_cast<unsigned long long*>(words), reinterpret_cast<int*>(words + 2),
                      reinterpret_cast<int*>(words + 3), reinterpret_cast<int*>(words + 4), words + 6,
                      words + GD_HEAD_WORDS, words + GD_HEAD_WORDS + mw};
    unsigned* const decw = S.par + 2 * mw;          // [nw] decimated variables, by sorted position
    unsigned* const sgnw = decw + nw;               // [nw] LARGE: those decimated to -decim_llr

    const int first_long = G.row_off[RC + 1], n_long = G.row_off[RC + 2] - first_long;
    const int lbase = G.row_base[RC + 1], n_ledges = E - lbase;
    const int T = P.iters_per_round;
    double* const Lw = G.wsL + (size_t)blockIdx.x * 3 * (n_long > 0 ? n_long : 1);

    if constexpr (VARIANT == 0) np_tables_to_lds(gd_smem, tid, nt);     // (published by the record's first barrier)
    const long long count = record_count<RECORDS>(io, S);
    const bool dynamic = count > (long long)gridDim.x;

    for (long long item = blockIdx.x; item < count;) {
        const long long rec = record_load_syndrome<RECORDS>(G, io, S, item);
        // ---- rule 1: W = V = prior, Q = prior on the edges, nothing decimated ----------------------------------------
        if constexpr (LARGE) {
            for (int i = tid; i < 2 * nw; i += nt) decw[i] = 0u;      // (both maps)
            for (int x = tid; x < n; x += nt) V[x] = G.prior_sorted[x];
        } else {
            for (int i = tid; i < nw; i += nt) decw[i] = 0u;
            for (int x = tid; x < n; x += nt) {
                const double pv = G.prior_sorted[x];
                Wp[x] = pv; V[x] = pv;
            }
        }
        record_prior_to_edges(G, S, G.prior_sorted);
        __syncthreads();
        const int syn_weight = S.unsat[0];    // unsatisfied checks of the all-zero candidate

        int total = 0, rounds = 0;
        bool solved = false;
        for (;;) {
            // ===================== one round: T iterations (rule 2) ===================================================
            for (int t = 0; t < T && !solved; ++t) {
                // ================= check step (rule 2.1) ==========================================================
                if constexpr (VARIANT == 2) {
                    record_check_step_minsum(G, S, Lw, P.alpha);
                } else {
                    // The sum-product rows stay here, on the kernel's own M: stated in a function of qbp_record_bp.hpp the
                    // same text needs 101 registers instead of 96, which is 4 wavefronts per SIMD instead of the 5 the
                    // host's grid counts on (gd_launch).
                    for (int wp0 = tid - lane; wp0 < G.rpad_off[RC + 1]; wp0 += nt) {
                        // one wavefront = 64 consecutive work items of ONE weight class (scalar class search)
                        const int wpu = __builtin_amdgcn_readfirstlane(wp0);
                        int D = 1;
#pragma unroll
                        for (int k = 2; k <= RC; ++k) D += wpu >= G.rpad_off[k] ? 1 : 0;
                        int lane_ = lane;       // (opaque: keeps the per-class address arithmetic inside the loop)
                        asm volatile("" : "+v"(lane_));
#define QBP_GD_SP_ROW_CLASS(DD)                                                                        \
                        case DD: {                                                                     \
                            const int cnt = G.row_off[DD + 1] - G.row_off[DD];                         \
                            const int i = wpu - G.rpad_off[DD] + lane_;                                \
                            if (i < cnt) {                                                             \
                                const int w = G.row_off[DD] + i;                                       \
                                const unsigned sbit = (S.synw[w >> 5] >> (w & 31)) & 1u;               \
                                const int base = G.row_base[DD] + i;                                   \
                                double q[DD];                                                          \
                                _Pragma("unroll") for (int j = 0; j < DD; ++j) q[j] = M[base + j * cnt];   \
                                auto put = [&](int j, double v) { M[base + j * cnt] = v; };            \
                                check_row<0, DD, true>(q, sbit, P.alpha, true, RECORD_NP_TAB, put); \
                            }                                                                          \
                        } break;
                        switch (D) {
                            QBP_GD_SP_ROW_CLASS(1) QBP_GD_SP_ROW_CLASS(2) QBP_GD_SP_ROW_CLASS(3) QBP_GD_SP_ROW_CLASS(4)
                            QBP_GD_SP_ROW_CLASS(5) QBP_GD_SP_ROW_CLASS(6) QBP_GD_SP_ROW_CLASS(7) QBP_GD_SP_ROW_CLASS(8)
                            default: break;
                        }
#undef QBP_GD_SP_ROW_CLASS
                    }
                    // ---- checks of weight > 8: the per-edge work one thread per edge, the sequential part (np.prod in
                    //      ascending column order) one thread per check
                    if (n_long > 0) {                                           // uniform
                        for (int k = tid; k < n_ledges; k += nt)
                            M[lbase + k] = tanh_half_msg<VARIANT>(M[lbase + k], RECORD_NP_TAB);
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
                            M[lbase + k] = sp_message<VARIANT>(Lw[3 * i], M[lbase + k], sbit, RECORD_NP_TAB);
                        }
                    }
                }
                __syncthreads();                                          // ---- barrier A
                // ================= variable step (rules 2.2 - 2.4) + incremental syndrome test (2.5) ================
                const int p = total & 1;
                if constexpr (LARGE) {
                    // W of the sorted variable x: +-decim_llr where decimated, else its prior (every value W[x] held)
                    record_variable_step<VARIANT == 2>(G, S, p, syn_weight, P.clip_llr, [&](int x) {
                        const unsigned bit = 1u << (x & 31);
                        if (decw[x >> 5] & bit) return (sgnw[x >> 5] & bit) ? -P.decim_llr : P.decim_llr;
                        return G.prior_sorted[x];
                    });
                } else {
                    record_variable_step<VARIANT == 2>(G, S, p, syn_weight, P.clip_llr, [&](int x) { return Wp[x]; });
                }
                __syncthreads();                                          // ---- barrier B
                ++total;
                solved = S.unsat[p] == 0;
            }
            if (solved || rounds == P.max_rounds) break;                  // rule 3 (uniform)
            // ===================== the variable to decimate: block-wide arg-max ========================================
            GdKey best{0ull, 0x7fffffff, 0};
            for (int x = tid + G.col_off[1]; x < n; x += nt) {            // (variables before col_off[1] have no check)
                const double val = V[x];
                if (val != val || ((decw[x >> 5] >> (x & 31)) & 1u)) continue;
                const GdKey k{(unsigned long long)__double_as_longlong(val) & 0x7fffffffffffffffull, G.svar[x], x};
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
                if constexpr (LARGE) {
                    if (V[best.pos] < 0.0) sgnw[best.pos >> 5] |= 1u << (best.pos & 31);
                } else {
                    Wp[best.pos] = V[best.pos] < 0.0 ? -P.decim_llr : P.decim_llr;
                }
                decw[best.pos >> 5] |= 1u << (best.pos & 31);
            }
            ++rounds;
        }
        // ---- rule 4: the last iteration executed -----------------------------------------------------------------------
        if constexpr (RECORDS) {
            record_classify(G, io, S, rec, solved, [&](int x) { return V[x] < 0.0 ? 1u : 0u; });
        } else {
            for (int x = tid; x < n; x += nt) {
                const double val = V[x];
                const int v = G.svar[x];
                if (io.llr) io.llr[rec * n + v] = val;
                if (io.hard) io.hard[rec * n + v] = (uint8_t)(val < 0.0 ? 1 : 0);
            }
            if (tid == 0) {
                if (io.converged) io.converged[rec] = (uint8_t)(solved ? 1 : 0);
                if (io.iters) io.iters[rec] = total;
                if (P.rounds) P.rounds[rec] = rounds;
            }
        }
        item = record_next_item(G, S, dynamic);
    }
}

}  // namespace qbp
