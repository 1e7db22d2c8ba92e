// Relay-BP: min-sum with a disordered memory term, run as a chain of legs (include/qbp.h, qbp_relay_decode_batch,
// states the rules; tests/relay_oracle.py is the numpy statement the kernel is compared with bit for bit).
//
// One workgroup per record, the per-record BP iteration of qbp_record_bp.hpp (the tables of the general-H kernel, the
// messages in place in LDS) with two workgroup barriers per iteration:
//   check step     record_check_step_minsum;
//   -- barrier A --
//   variable step  record_variable_step with bias = (1 - gamma) prior + gamma V: V = colsum(R) + bias (ascending check),
//                  Q = clip(V - R) in place, and the incremental syndrome test;
//   -- barrier B --
//   counter zero <=> H hard == s: a solution.  One thread adds up its weight in column order (as osd_order_kernel adds
//   its costs); if it is the lightest so far the workgroup writes it straight to the record's output row.
// This file has what is Relay's own: the LDS carve-up, the leg loop, the bias, the solution bookkeeping (best_hard) and
// the batch outputs.  The parameter blocks, the record prologue, the two steps, the classification of the records build
// and the hand-out of the next record are qbp_record_bp.hpp's, shared with bp_gd_kernel.
// Everything a record touches per iteration is in LDS: the E messages, V[n], the prior and the current leg's gamma row
// (both in sorted-variable order; gamma is reloaded at each leg start), the syndrome and parity bits.  Min-sum needs no
// tanh / arctanh tables.  A record of [[144,12,12]] takes 7 KB, so the workgroup is kept small (record_threads) and
// several are resident per CU: records run hundreds of iterations of a few dozen instructions each, and what hides
// the LDS and barrier latency of one is the other workgroups of the CU.
// Two builds: RECORDS = false decodes B syndromes to outputs; RECORDS = true reads the failure records of a
// Monte-Carlo launch (count and list in device memory, fail_syn, fail_err), decodes them and classifies the result
// into the counters, as the OSD record kernels do.
// Two memory layouts of each (QBP_OPT_RELAY_MEM): LARGE = false is the above; LARGE = true is the same
// statement for matrices whose E messages do not fit -- space-time and detector-error-model matrices.  Its messages are
// the workgroup's slice of a global workspace wsM[grid][E], which stays in L2 / Infinity Cache as the general-H kernel's
// does (qbp_generic.hpp); the prior is read where the launch permuted it (prior_sorted) and the gamma row where the
// configuration put it, so neither is copied.  In LDS stay V[n] (the bias reads the previous V[x], the same thread writes
// the new one), the words, the syndrome and parity bits and best_hard: 8 n bytes + the words, 69 KiB for 2592 x 7776 in
// the records build.
// The shared steps reach the messages through RecordLds::M, a plain pointer, and are called unchanged; both barriers
// stay where they are.  A message is written by one wavefront and read by another of the same workgroup across a
// barrier: __syncthreads() is a workgroup-scope release, the barrier and a workgroup-scope acquire.  On gfx950 outside
// threadgroup-split mode the compiler emits s_waitcnt lgkmcnt(0) and NO vmcnt(0) for that release: the wavefronts of a
// workgroup share their CU's vector L1, which is write-through and keeps their memory operations in issue order, so a
// store issued before the barrier is ordered before a load issued after it (DESIGN.md section 3b has what the ISA shows;
// wsL of the LDS build and the general-H kernel's workspace rely on the same).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_record_bp.hpp"

namespace qbp {

constexpr int RELAY_MAX_THREADS = 1024;     // ([[144,12,12]]: 192 threads, [[288,12,18]]: 320 -- nine and five
                                            //  workgroups in the 28 wavefronts a CU holds at the kernel's registers)

struct RelayParams {
    RecordTables tab;
    RecordIo io;
    const int32_t* vinv;            // [n] sorted position of variable v (the inverse of svar)
    const double* prior;            // [n] the caller's prior
    // ---- the configuration (qbp_relay_configure) -------------------------------------------------------------------
    const double* gammas_sorted;    // [L][n] memory strengths, sorted-variable order
    const int32_t* leg_iters;       // [L]
    int L, stop_after;
    double alpha, clip_llr;
    // ---- batch build: the outputs beyond RecordIo's (either may be null) -----------------------------------------------
    int32_t* legs;                  // [B] legs entered
    int32_t* solutions;             // [B] solutions found
    // ---- LARGE build -----------------------------------------------------------------------------------------------------
    double* wsM;                    // [grid][E] the messages of the workgroups' current records
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

// Dynamic LDS of one workgroup of the LARGE build: V, the words, and (records build) best_hard
__host__ __device__ inline size_t relay_large_lds_bytes(int m, int n, bool records)
{
    return (size_t)8 * (size_t)n + 4 * relay_lds_words(m) + (records ? (((size_t)n + 7) & ~(size_t)7) : 0);
}

// LARGE: the messages in the workgroup's slice of P.wsM, prior and gammas read in place.
template <bool RECORDS, bool LARGE = false>
__global__ __launch_bounds__(RELAY_MAX_THREADS) void bp_relay_kernel(const RelayParams P)
{
    extern __shared__ __attribute__((aligned(16))) double relay_smem[];
    constexpr int RC = GENERIC_MAX_ROW_CLASS;
    const RecordTables& G = P.tab;
    const RecordIo& io = P.io;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int m = G.m, n = G.n, E = G.E;
    // [E] messages, in place
    double* const M = LARGE ? P.wsM + (size_t)blockIdx.x * (size_t)E : relay_smem;
    double* const V = LARGE ? relay_smem : M + E;   // [n] posterior values, sorted-variable order
    double* const prior_lds = V + n;                // [n] (not LARGE)
    double* const gam_lds = prior_lds + n;          // [n] the current leg's memory strengths (not LARGE)
    const double* const prior_t = LARGE ? G.prior_sorted : prior_lds;
    const double* gam = gam_lds;                    // (LARGE: the leg's row of P.gammas_sorted)
    unsigned* const words = reinterpret_cast<unsigned*>(LARGE ? V + n : gam_lds + n);
    const int mw = (m + 31) >> 5;
    unsigned* const better = words + 6;
    const RecordLds S{M, V, reinterpret_cast<unsigned long long*>(words), reinterpret_cast<int*>(words + 2),
                      reinterpret_cast<int*>(words + 3), reinterpret_cast<int*>(words + 4), words + 7, words + 8,
                      words + 8 + mw};
    uint8_t* const best_hard = reinterpret_cast<uint8_t*>(words + relay_lds_words(m));   // [n] (records build)

    const int n_long = G.row_off[RC + 2] - G.row_off[RC + 1];
    double* const Lw = G.wsL + (size_t)blockIdx.x * 3 * (n_long > 0 ? n_long : 1);

    if constexpr (!LARGE)
        for (int x = tid; x < n; x += nt) prior_lds[x] = G.prior_sorted[x];   // (published by the record's first barrier)
    const long long count = record_count<RECORDS>(io, S);
    const bool dynamic = count > (long long)gridDim.x;

    // the last iteration executed, or the lightest solution so far: to the record's output row
    auto write_result = [&](long long rec) {
        for (int x = tid; x < n; x += nt) {
            const double val = V[x];
            const uint8_t hd = val < 0.0 ? 1 : 0;
            if constexpr (RECORDS) {
                best_hard[x] = hd;
            } else {
                const int v = G.svar[x];
                if (io.llr) io.llr[rec * n + v] = val;
                if (io.hard) io.hard[rec * n + v] = hd;
            }
        }
    };

    for (long long item = blockIdx.x; item < count;) {
        const long long rec = record_load_syndrome<RECORDS>(G, io, S, item);
        // ---- rule 1: Q = prior on the edges, V = prior ---------------------------------------------------------------
        for (int x = tid; x < n; x += nt) V[x] = prior_t[x];
        record_prior_to_edges(G, S, prior_t);
        __syncthreads();
        const int syn_weight = S.unsat[0];    // unsatisfied checks of the all-zero candidate

        int found = 0, total = 0, legs = 0;
        double best_w = 0.0;                  // (thread 0)
        for (int leg = 0; leg < P.L; ++leg) {
            ++legs;
            // (the last readers of gam passed barrier B of the previous leg; barrier A publishes the new row)
            if constexpr (LARGE) gam = P.gammas_sorted + (size_t)leg * n;
            else for (int x = tid; x < n; x += nt) gam_lds[x] = P.gammas_sorted[(size_t)leg * n + x];
            const int T = P.leg_iters[leg];
            bool solved = false;
            for (int t = 0; t < T && !solved; ++t) {
                // ================= check step (rule 2a) ==========================================================
                record_check_step_minsum(G, S, Lw, P.alpha);
                __syncthreads();                                          // ---- barrier A
                // ================= variable step (rules 2b - 2e) + incremental syndrome test =====================
                const int p = total & 1;
                // bias of the sorted variable x (rule 2b: every operation rounded on its own)
                record_variable_step<true>(G, S, p, syn_weight, P.clip_llr, [&](int x) {
                    const double g = gam[x];
                    return (1.0 - g) * prior_t[x] + g * V[x];
                });
                __syncthreads();                                          // ---- barrier B
                ++total;
                if (S.unsat[p] != 0) continue;
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
                if (*better) write_result(rec);       // the lightest so far
            }
            if (found >= P.stop_after) break;             // rule 3
        }
        if (found == 0) write_result(rec);            // no solution: the last iteration executed
        if constexpr (RECORDS) {
            __syncthreads();
            record_classify(G, io, S, rec, found > 0, [&](int x) { return (unsigned)best_hard[x]; });
        } else if (tid == 0) {
            if (io.converged) io.converged[rec] = (uint8_t)(found > 0 ? 1 : 0);
            if (io.iters) io.iters[rec] = total;
            if (P.legs) P.legs[rec] = legs;
            if (P.solutions) P.solutions[rec] = found;
        }
        item = record_next_item(G, S, dynamic);
    }
}

}  // namespace qbp
