// Localized statistics decoding beyond the LDS limit (QBP_OPT_LSD_MEM): lsd_kernel's statement (include/qbp.h,
// qbp_lsd_batch; tests/lsd_oracle.py), bit for bit, with the rows of [H | residual] in a per-workgroup global workspace
// and only the rows of the ACTIVE checks in existence.
//
// The invariant: a row that was never changed equals its original row of [H | r]; a row is only changed
// while it has a 1 in an active column, every check of an active variable is active, and a variable is activated
// before its round's elimination -- so every changed row belongs to an active check.  The pivot search and the XOR
// targets of a column look at the active checks' rows alone, and a check's row is written -- zeroed, then set from the
// CSR, with its original residual bit -- at the moment the check becomes active.  It is never read before that, so a
// workgroup that takes its next record never sees the previous record's rows and the slice is never cleared.
//
// One workgroup of 256 threads per record, handed out as in lsd_kernel.  The slice has room for all m checks, (W + 1)
// 32-bit words each, the residual bit in the last word, indexed by check: no slot map.  ROW-MAJOR: the active checks
// are a sparse set of rows, and everything that is wide -- writing a row, XORing the pivot row into a target -- runs
// along one row, W + 1 neighbouring words, coalesced over the threads; transposed word planes would put the words of
// one row m apart and coalesce over rows, which a sparse set of rows does not fill.  The one narrow access, word c / 32
// of every active row in the pivot search, is a scattered read in either layout.
//
// LDS: the per-check tables pivcol, label, pick, prev (pick doubles as the list of a column's XOR targets: it is idle
// between the candidate steps of two rounds), bad and the compact list `alist` of the active checks; the per-variable
// tables idx (the order), rank, sol, act.  The sort keys overlay the per-check tables while they fit
// (lsd_large_layout), else they live in the workspace, as osd0_big_kernel's.  Everything per check is initialised when
// the check turns active and read through alist or through a label: the work of a record scales with its clusters.
//
// The rows are shared between the four wavefronts, unlike the message workspaces of the other large builds: where
// lsd_kernel passes from one phase to the next with a ballot, this kernel has a workgroup barrier -- materialise ->
// scan -> XOR -> next column -- and every thread reaches every barrier (all loop conditions are uniform; a vote of the
// workgroup is block_sum, a sum through the head's slots: no static LDS).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_lsd.hpp"

namespace qbp {

constexpr int LSD_LARGE_THREADS = 256;
constexpr size_t LSD_LARGE_HEAD = 64;       // the tally and the workgroup's counters, in front of the dynamic LDS

struct LsdLargeWorkspace {
    uint32_t* rows;                 // [grid][m][W + 1]
    unsigned long long* keys;       // [grid][NP]   (only when the keys do not fit LDS)
    int keys_in_lds;
    int region0;                    // bytes of { keys | per-check tables }
};

// LDS: head[64]; region 0 { u64 keys[NP] (while they fit) | int pivcol[m], int label[m], uint32 pick[m], uint32 prev[m],
// int alist[m] }; uint16 idx[NP], uint16 rank[n]; uint8 sol[n], uint8 act[n], uint8 bad[m]; rounded up to 16.
struct LsdLargeLayout {
    int keys_in_lds;
    size_t region0, bytes;
};
__host__ __device__ inline LsdLargeLayout lsd_large_layout(int m, int n, int NP)
{
    const size_t tables = (size_t)m * 20, keys = (size_t)NP * 8;
    const size_t rest = LSD_LARGE_HEAD + (size_t)NP * 2 + (size_t)n * 4 + (size_t)m;
    LsdLargeLayout L;
    L.region0 = ((keys > tables ? keys : tables) + 7) & ~(size_t)7;
    L.keys_in_lds = ((L.region0 + rest + 15) & ~(size_t)15) <= (size_t)160 * 1024;
    if (!L.keys_in_lds) L.region0 = (tables + 7) & ~(size_t)7;
    L.bytes = (L.region0 + rest + 15) & ~(size_t)15;
    return L;
}
__host__ __device__ inline size_t lsd_large_lds_bytes(int m, int n, int NP)
{
    return lsd_large_layout(m, n, NP).bytes;
}

struct LsdLargeHead {
    OsdTally tally;
    unsigned piv[3], cnt[3];        // per column: lowest unused row with the bit, number of rows with the bit
    unsigned nact, sum[3];          // active checks; block_sum's slots
};
static_assert(sizeof(LsdLargeHead) <= LSD_LARGE_HEAD, "the head of lsd_large_kernel's LDS");

// The rows of the checks alist[from .. to): zeroed, then (a barrier later) set from the CSR, one thread per row, with
// the residual bit syn ^ (H hard).  The caller's next barrier makes them visible.
template <typename Params>
__device__ __forceinline__ void lsd_large_materialise(const Params& P, uint32_t* rows, const int* alist, int from,
                                                      int to, const uint8_t* syn, const uint8_t* sol, int tid, int nt)
{
    const int RS = P.W + 1;
    for (int it = tid; it < (to - from) * RS; it += nt) {
        const int j = it / RS;
        rows[(size_t)alist[from + j] * RS + (it - j * RS)] = 0u;
    }
    __syncthreads();
    for (int i = from + tid; i < to; i += nt) {
        const int r = alist[i];
        uint32_t* const row = rows + (size_t)r * RS;
        unsigned par = syn[r] & 1u;
        for (int e = P.row_ptr[r]; e < P.row_ptr[r + 1]; ++e) {
            const int c = P.col_idx[e];
            row[c >> 5] |= 1u << (c & 31);
            par ^= sol[c];
        }
        row[P.W] = par;
    }
}

template <bool RECORDS>
__global__ __launch_bounds__(LSD_LARGE_THREADS) void lsd_large_kernel(const LsdParams P, const LsdLargeWorkspace Wk)
{
    extern __shared__ double lsd_large_smem[];
    const int tid = threadIdx.x, nt = LSD_LARGE_THREADS, lane = tid & 63;
    const int m = P.m, n = P.n, W = P.W, NP = P.NP, g = P.bits_per_step, RS = W + 1;
    char* const lds = reinterpret_cast<char*>(lsd_large_smem);
    LsdLargeHead& S = *reinterpret_cast<LsdLargeHead*>(lds);
    char* const base0 = lds + LSD_LARGE_HEAD;
    unsigned long long* const keys = Wk.keys_in_lds ? reinterpret_cast<unsigned long long*>(base0)
                                                    : Wk.keys + (size_t)blockIdx.x * NP;
    int* const pivcol = reinterpret_cast<int*>(base0);               // (after the sort: same bytes as the keys in LDS)
    int* const label = pivcol + m;
    uint32_t* const pick = reinterpret_cast<uint32_t*>(label + m);
    uint32_t* const prev = pick + m;
    int* const alist = reinterpret_cast<int*>(prev + m);
    uint16_t* const idx = reinterpret_cast<uint16_t*>(base0 + Wk.region0);
    uint16_t* const rnk = idx + NP;
    uint8_t* const sol = reinterpret_cast<uint8_t*>(rnk + n);
    uint8_t* const act = sol + n;
    uint8_t* const bad = act + n;
    uint32_t* const rows = Wk.rows + (size_t)blockIdx.x * m * RS;
    int* const tl = reinterpret_cast<int*>(pick);                    // a column's rows with the bit (see the header)

    if (tid < 3) { S.piv[tid] = ~0u; S.cnt[tid] = 0u; }
    unsigned col_ctr = 0;                     // columns scanned so far: slot col_ctr % 3 of S.piv / S.cnt is the live one
    // The sum over the workgroup of one int per thread, with one barrier: slot sum_ctr % 3 of S.sum is the live one, and
    // the slot of two calls ahead, last read a barrier ago, is zeroed behind the barrier.
    unsigned sum_ctr = 0;
    auto block_sum = [&](int x) {
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        unsigned* const slot = &S.sum[sum_ctr % 3u];
        if (lane == 0 && x) atomicAdd(slot, (unsigned)x);
        __syncthreads();
        if (tid == 0) S.sum[(sum_ctr + 2u) % 3u] = 0u;
        ++sum_ctr;
        return (int)*slot;
    };
    if (tid < 3) S.sum[tid] = 0u;

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        const long long rec = P.list ? P.list[item] : item;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;

        // ---- 1. order = argsort(|llr|), ties by column index (osd0_kernel's sort); rank = its inverse
        osd_order_fill(P, rec, keys, idx, tid, nt);
        for (int i = tid; i < n; i += nt) { sol[i] = hard[i] & 1u; act[i] = 0; }
        if (tid == 0) S.nact = 0u;
        __syncthreads();
        osd_sort(keys, idx, NP, tid, nt);
        for (int k = tid; k < n; k += nt) rnk[idx[k]] = (uint16_t)k;     // (the n real columns sort before the padding)
        // ---- 2. the seeds are clusters of one check, and the first rows to exist
        // (the tables overwrite the sort keys: every thread passed the sort's last barrier)
        for (int r = tid; r < m; r += nt) {
            unsigned par = syn[r] & 1u;
            for (int e = P.row_ptr[r]; e < P.row_ptr[r + 1]; ++e) par ^= sol[P.col_idx[e]];
            label[r] = par ? r : -1;
            if (par) { alist[atomicAdd(&S.nact, 1u)] = r; pivcol[r] = -1; }
        }
        __syncthreads();
        int nact = (int)S.nact;               // active checks: alist[0 .. nact), in no particular order
        lsd_large_materialise(P, rows, alist, 0, nact, syn, sol, tid, nt);
        int rounds = 0, nactive = 0;
        bool valid;
        // ---- 3. rounds (each activates at least one of the n variables: at most n of them)
        for (;;) {
            // validity at the start of the round: an active row without pivot whose reduced syndrome bit is 1
            for (int i = tid; i < nact; i += nt) { const int r = alist[i]; bad[r] = 0; pick[r] = ~0u; prev[r] = 0u; }
            __syncthreads();                  // (and: the rows of the last materialisation, the last column's XOR)
            int open = 0;
            for (int i = tid; i < nact; i += nt) {
                const int r = alist[i];
                if (pivcol[r] < 0 && (rows[(size_t)r * RS + W] & 1u)) { bad[label[r]] = 1; open = 1; }
            }
            valid = block_sum(open) == 0;
            if (valid) break;                 // every cluster explains its syndrome
            // candidates: the inactive variables next to a check of an invalid cluster
            int added = 0;
            if (g == 0) {
                for (int v = tid; v < n; v += nt) {
                    if (act[v]) continue;
                    bool take = false;
                    for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                        const int L = label[P.col_row[e]];
                        take |= L >= 0 && bad[L];
                    }
                    if (take) { act[v] = 2; ++added; }
                }
            } else {
                for (int step = 0; step < g; ++step) {
                    // the lowest candidate of every invalid cluster above the cluster's previous pick
                    for (int v = tid; v < n; v += nt) {
                        if (act[v] == 1) continue;               // (2: claimed in this round, still a candidate of others)
                        const uint32_t key = (((uint32_t)rnk[v] << 16) | (uint32_t)v) + 1u;
                        for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                            const int L = label[P.col_row[e]];
                            if (L >= 0 && bad[L] && key > prev[L]) atomicMin(&pick[L], key);
                        }
                    }
                    __syncthreads();
                    int got = 0;
                    for (int i = tid; i < nact; i += nt) {
                        const int r = alist[i];
                        const uint32_t key = pick[r];
                        if (key != ~0u) {
                            act[(key - 1u) & 0xffffu] = 2;       // (two clusters, one variable: the same byte)
                            prev[r] = key;
                            pick[r] = ~0u;
                            got = 1;
                        }
                    }
                    if (block_sum(got) == 0) break;              // (uniform) every cluster is out of candidates
                }
                for (int v = tid; v < n; v += nt) added += act[v] == 2;
            }
            added = block_sum(added);         // (its barrier: act is written)
            if (added == 0) break;            // (uniform) nothing left to activate: some cluster stays invalid
            ++rounds;
            nactive += added;
            // the checks of the new variables join, each through the one thread that wins its label; their rows come
            // into existence; then the labels settle on the lowest check of every cluster
            for (int v = tid; v < n; v += nt) {
                if (act[v] != 2) continue;
                for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                    const int c = P.col_row[e];
                    if (label[c] < 0 && atomicCAS(&label[c], -1, c) == -1) {
                        alist[atomicAdd(&S.nact, 1u)] = c;
                        pivcol[c] = -1;
                    }
                }
            }
            __syncthreads();
            const int nact_was = nact;
            nact = (int)S.nact;
            lsd_large_materialise(P, rows, alist, nact_was, nact, syn, sol, tid, nt);
            for (;;) {
                int changed = 0;
                for (int v = tid; v < n; v += nt) {
                    if (!act[v]) continue;
                    int lo = 0x7fffffff;
                    for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) lo = min(lo, label[P.col_row[e]]);
                    for (int e = P.col_ptr[v]; e < P.col_ptr[v + 1]; ++e) {
                        const int c = P.col_row[e];
                        if (label[c] > lo) { atomicMin(&label[c], lo); changed = 1; }
                    }
                }
                if (block_sum(changed) == 0) break;          // (and: the new rows are written)
            }
            // ---- elimination of the round's columns in ascending rank, on the active rows; every wavefront walks the
            //      order and finds the same columns
            for (int k0 = 0; k0 < n; k0 += 64) {
                const int mine = k0 + lane < n ? (int)idx[k0 + lane] : 0;
                unsigned long long todo = __ballot(k0 + lane < n && act[mine] == 2);
                while (todo) {                       // (uniform over the workgroup)
                    const int c = __shfl(mine, (int)__builtin_ctzll(todo));
                    todo &= todo - 1ull;
                    const int wi = c >> 5;
                    const uint32_t bit = 1u << (c & 31);
                    unsigned* const piv = &S.piv[col_ctr % 3u];
                    unsigned* const cnt = &S.cnt[col_ctr % 3u];
                    // scan: the rows with a 1 in column c, and the lowest of them that is no pivot row yet
                    for (int i = tid; i < nact; i += nt) {
                        const int r = alist[i];
                        if (rows[(size_t)r * RS + wi] & bit) {
                            tl[atomicAdd(cnt, 1u)] = r;
                            if (pivcol[r] < 0) atomicMin(piv, (unsigned)r);
                        }
                    }
                    __syncthreads();
                    const unsigned pu = *piv;
                    const int nt_rows = (int)*cnt;
                    // (the slot of two columns ahead, last read a barrier ago: idle now)
                    if (tid == 0) { S.piv[(col_ctr + 2u) % 3u] = ~0u; S.cnt[(col_ctr + 2u) % 3u] = 0u; }
                    ++col_ctr;
                    if (pu == ~0u) continue;         // the column depends on earlier ones: it stays active, no pivot
                    const int p = (int)pu;
                    // XOR: the pivot row, over the full width and the residual word, into every other row with the bit
                    const uint32_t* const prow = rows + (size_t)p * RS;
                    for (int it = tid; it < nt_rows * RS; it += nt) {
                        const int j = it / RS, w = it - j * RS;
                        const int r = tl[j];
                        if (r != p) rows[(size_t)r * RS + w] ^= prow[w];
                    }
                    if (tid == 0) pivcol[p] = c;
                    __syncthreads();
                }
            }
            __syncthreads();                  // (every wavefront has walked the order: act may change)
            for (int v = tid; v < n; v += nt)
                if (act[v] == 2) act[v] = 1;
            // (the round's first barrier stands between this and the next reader of act)
        }
        // ---- 4. e[pivot column] = reduced syndrome bit; solution = hard + e; the statistics
        int clusters = 0;
        for (int i = tid; i < nact; i += nt) {
            const int r = alist[i];
            const int c = pivcol[r];
            if (c >= 0 && (rows[(size_t)r * RS + W] & 1u)) sol[c] ^= 1u;        // (distinct pivot columns: no race)
            clusters += label[r] == r;
        }
        if (tid == 0) S.tally = OsdTally{};
        clusters = block_sum(clusters);       // (its barrier: sol is complete, the tally is zero)
        if (P.solution)
            for (int i = tid; i < n; i += nt) P.solution[rec * n + i] = sol[i];
        if (P.stats && tid < 4)
            P.stats[rec * 4 + tid] = tid == 0 ? rounds : tid == 1 ? nactive : tid == 2 ? clusters : (int)valid;

        // classification of the output, as osd0_blocked_kernel's (its `bad`: exactly the records with valid = 0)
        if constexpr (RECORDS) osd_tail_block(P, rec, sol, syn, S.tally, tid, nt);
        __syncthreads();
    }
}

}  // namespace qbp
