// Localized statistics decoding (BP+LSD; Hillmann, Berent, Di Matteo, Eisert, Wille, Roffe 2024) on the GPU: a second
// stage for the syndromes BP does not converge on, next to OSD-0.  include/qbp.h (qbp_lsd_batch) states the rules;
// tests/lsd_oracle.py is the same statement in numpy, and this kernel reproduces it bit for bit.
//
// One wavefront per record, in the frame of osd0_kernel (qbp_osd.hpp): the bit-packed full-width rows of
// [H | residual syndrome] in LDS in their original column indexing, lane l owning rows l, l + 64, ..., the bitonic sort of
// (|llr| bits, column), the lowest unused row with a 1 as the pivot of a column -- the same pieces of
// qbp_osd_parts.hpp: order, load, the pivot of one column, solution and the record's tail.  Instead of one sweep over all
// columns, rounds: every cluster that still holds an unexplained syndrome bit activates its g least reliable
// neighbouring variables (all of them for g = 0), and the columns activated in a round are eliminated in ascending rank
// on the same rows.  Rows are full width, so a column that becomes active late already carries every earlier row
// operation; clusters share neither checks nor variables, so one sweep over the round's columns eliminates every
// cluster on its own.
//
// Cluster bookkeeping (all in LDS, per record): label[c] = lowest check index of the cluster of active check c (-1:
// inactive), kept current by min-label propagation over the active variables' checks after every round (labels only
// fall, clusters only merge); bad[L] = cluster L holds a row without pivot whose reduced syndrome bit is 1; for g >= 1,
// pick[L] / prev[L]: g times an atomicMin over ((rank << 16 | v) + 1) of the cluster's candidates above its previous
// pick, so a variable two clusters claim counts for both and is activated once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_osd.hpp"

namespace qbp {

struct LsdParams {
    // code
    int m, n, W, NP;                // as OsdParams
    const uint32_t* hbits;          // [m][W] bit-packed rows of H
    const int32_t* row_ptr;         // CSR of H
    const int32_t* col_idx;
    const int32_t* col_ptr;         // CSC of H: the checks of column v, ascending, at col_row[col_ptr[v] .. col_ptr[v + 1])
    const int32_t* col_row;
    int bits_per_step;              // g: variables an invalid cluster activates per round (0: all its candidates)
    // batch: record index of item i is list ? list[i] : i
    long long count;
    const long long* count_ptr;     // optional: number of records (device), overrides count
    const long long* list;
    const uint8_t* syndromes;       // [*][m]
    const double* llr;              // [*][n]
    const uint8_t* hard;            // [*][n]
    uint8_t* solution;              // [*][n] (may be null)
    int32_t* stats;                 // [*][4] (may be null): rounds, active variables, clusters, valid
    // Monte-Carlo classification of the result, as osd0_kernel's (RECORDS build only)
    const uint8_t* errors;          // [*][n]
    const unsigned long long* lx_cols;
    int half_distance;
    long long* counters;
};

// LDS: osd0_kernel's region { u64 keys[NP] | uint32 A[m][W+1] }; int pivcol[m], int label[m], uint32 pick[m],
// uint32 prev[m]; uint16 idx[NP], uint16 rank[n]; uint8 sol[n], uint8 act[n] (0 inactive, 1 active, 2 activated in this
// round), uint8 bad[m].
__host__ __device__ inline size_t lsd_lds_bytes(int m, int n, int W, int NP)
{
    return osd_region0_bytes(m, W, NP) + (size_t)m * 16 + (size_t)NP * 2 + (size_t)n * 2 + (size_t)n * 2 + (size_t)m + 16;
}

// RECORDS: the records are the failure records of a Monte-Carlo launch and are classified (counters 1, 3, 4, 5, 8, 9,
// 10, as osd0_kernel fills them).
template <bool RECORDS>
__global__ __launch_bounds__(64) void lsd_kernel(const LsdParams P)
{
    extern __shared__ double lsd_smem[];
    const int lane = threadIdx.x;
    const int m = P.m, n = P.n, W = P.W, NP = P.NP, g = P.bits_per_step;
    char* const base0 = reinterpret_cast<char*>(lsd_smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base0);
    uint32_t* A = reinterpret_cast<uint32_t*>(base0);                // (after the sort: same bytes)
    int* pivcol = reinterpret_cast<int*>(base0 + osd_region0_bytes(m, W, NP));
    int* label = pivcol + m;
    uint32_t* pick = reinterpret_cast<uint32_t*>(label + m);
    uint32_t* prev = pick + m;
    uint16_t* idx = reinterpret_cast<uint16_t*>(prev + m);
    uint16_t* rnk = idx + NP;
    uint8_t* sol = reinterpret_cast<uint8_t*>(rnk + n);
    uint8_t* act = sol + n;
    uint8_t* bad = act + n;

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        const long long rec = P.list ? P.list[item] : item;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;

        // ---- 1. order = argsort(|llr|), ties by column index (osd0_kernel's sort); rank = its inverse
        osd_order_fill(P, rec, keys, idx, lane, 64);
        for (int i = lane; i < n; i += 64) { sol[i] = hard[i] & 1u; act[i] = 0; }
        __syncthreads();
        osd_sort(keys, idx, NP, lane, 64);
        for (int k = lane; k < n; k += 64) rnk[idx[k]] = (uint16_t)k;    // (the n real columns sort before the padding)
        // ---- 2. A = [H | residual syndrome]; the seeds are clusters of one check
        // (A overwrites the sort keys: every lane passed the sort's last barrier)
        unsigned sb = osd_wave_load(P, syn, sol, A, pivcol, W, lane,       // bit i: reduced syndrome bit of row lane + 64 i
                                    [&](int r, unsigned par) { label[r] = par ? r : -1; });
        __syncthreads();
        unsigned used = 0;                           // bit i: row lane + 64 i already serves as a pivot row
        int rounds = 0, nactive = 0;
        // ---- 3. rounds (each activates at least one of the n variables: at most n of them)
        for (;;) {
            // validity at the start of the round
            if (!__ballot((sb & ~used) != 0u)) break;              // every cluster explains its syndrome
            for (int r = lane; r < m; r += 64) { bad[r] = 0; pick[r] = ~0u; prev[r] = 0u; }
            __syncthreads();
            {
                unsigned open = sb & ~used;
                while (open) {
                    const int i = __builtin_ctz(open);
                    open &= open - 1u;
                    // (a row with a syndrome bit is a seed or took it from a pivot row of its cluster: an active check)
                    const int L = label[lane + 64 * i];
                    if (L >= 0) bad[L] = 1;
                }
            }
            __syncthreads();
            // candidates: the inactive variables next to a check of an invalid cluster
            int added = 0;
            if (g == 0) {
                for (int v = lane; v < n; v += 64) {
                    if (act[v]) continue;
                    bool take = false;
                    for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                        const int L = label[P.col_row[e]];
                        take |= L >= 0 && bad[L];
                    }
                    if (take) { act[v] = 2; ++added; }
                }
                __syncthreads();
            } else {
                for (int step = 0; step < g; ++step) {
                    // the lowest candidate of every invalid cluster above the cluster's previous pick
                    for (int v = lane; v < n; v += 64) {
                        if (act[v] == 1) continue;               // (2: claimed in this round, still a candidate of others)
                        const uint32_t key = (((uint32_t)rnk[v] << 16) | (uint32_t)v) + 1u;
                        for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                            const int L = label[P.col_row[e]];
                            if (L >= 0 && bad[L] && key > prev[L]) atomicMin(&pick[L], key);
                        }
                    }
                    __syncthreads();
                    int got = 0;
                    for (int r = lane; r < m; r += 64) {
                        const uint32_t key = pick[r];
                        if (key != ~0u) {
                            act[(key - 1u) & 0xffffu] = 2;       // (two clusters, one variable: the same byte)
                            prev[r] = key;
                            pick[r] = ~0u;
                            got = 1;
                        }
                    }
                    __syncthreads();
                    if (!__ballot(got)) break;                   // (uniform) every cluster is out of candidates
                }
                for (int v = lane; v < n; v += 64) added += act[v] == 2;
            }
            for (int off = 32; off > 0; off >>= 1) added += __shfl_xor(added, off);
            if (added == 0) break;                   // (uniform) nothing left to activate: some cluster stays invalid
            ++rounds;
            nactive += added;
            // the checks of the new variables join; then the labels settle on the lowest check of every cluster
            for (int v = lane; v < n; v += 64) {
                if (act[v] != 2) continue;
                for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                    const int c = P.col_row[e];
                    if (label[c] < 0) label[c] = c;  // (several lanes: the same value)
                }
            }
            __syncthreads();
            for (;;) {
                int changed = 0;
                for (int v = lane; v < n; v += 64) {
                    if (!act[v]) continue;
                    int lo = 0x7fffffff;
                    for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) lo = min(lo, label[P.col_row[e]]);
                    for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                        const int c = P.col_row[e];
                        if (label[c] > lo) { atomicMin(&label[c], lo); changed = 1; }
                    }
                }
                __syncthreads();
                if (!__ballot(changed)) break;
            }
            // ---- elimination of the round's columns in ascending rank, on the same rows
            for (int k0 = 0; k0 < n; k0 += 64) {
                const int mine = k0 + lane < n ? (int)idx[k0 + lane] : 0;
                unsigned long long todo = __ballot(k0 + lane < n && act[mine] == 2);
                while (todo) {                       // (uniform)
                    const int c = __shfl(mine, (int)__builtin_ctzll(todo));
                    todo &= todo - 1ull;
                    unsigned has;
                    const int p = osd_wave_find(A, m, W, c, lane, used, has);
                    if (p < 0) continue;             // the column depends on earlier ones: it stays active, no pivot
                    osd_wave_eliminate<0>(A, m, W, p, has, lane, used, sb);
                    if (lane == 0) pivcol[p] = c;
                    __syncthreads();
                }
            }
            for (int v = lane; v < n; v += 64)
                if (act[v] == 2) act[v] = 1;
            __syncthreads();
        }
        // ---- 4. e[pivot column] = reduced syndrome bit; solution = hard + e; the statistics
        const bool valid = !__ballot((sb & ~used) != 0u);
        int clusters = 0;
        osd_wave_solution(A, pivcol, sol, m, W, lane, [&](int r) { clusters += label[r] == r; });
        for (int off = 32; off > 0; off >>= 1) clusters += __shfl_xor(clusters, off);
        __syncthreads();
        if (P.solution)
            for (int i = lane; i < n; i += 64) P.solution[rec * n + i] = sol[i];
        if (P.stats && lane < 4)
            P.stats[rec * 4 + lane] = lane == 0 ? rounds : lane == 1 ? nactive : lane == 2 ? clusters : (int)valid;

        // classification of the output, as osd0_kernel's (its `bad`: exactly the records with valid = 0)
        if constexpr (RECORDS) osd_tail_wave(P, rec, sol, syn, lane);
        __syncthreads();
    }
}

}  // namespace qbp
