// OSD-0 post-processing on the GPU: decoding/OSD.py:3-72 (performOSD + gf2_elimination).
//
// One wavefront per syndrome.  The reference permutes the columns of H by ascending |LLR|, runs a
// Gauss-Jordan elimination with row swaps and reads the solution off the pivot columns.  For a syndrome in
// the column space of H (every syndrome that comes from an error) the solution only depends on WHICH columns
// become pivots (the greedy, first-independent-columns basis in reliability order) -- not on which row
// serves as the pivot (for the others see osd_flag_inconsistent) -- so this kernel never
// swaps or permutes: it keeps the bit-packed rows of H in LDS in their original column indexing,
// walks the columns in sorted order, picks any not-yet-used row with a 1 in that column as the
// pivot and XORs it into every other row that has the bit (rows are n bits + the syndrome bit).
//
// The stages of a record -- column order, the sweeps, the classification of the result -- are stated once in
// qbp_osd_parts.hpp for all the OSD and LSD kernels; this file holds the three OSD-0 kernels built from them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_osd_parts.hpp"

namespace qbp {

// LDS: { u64 keys[NP] | uint32 A[m][W+1] } (the sort is over before the matrix is filled: one region
// for both -- 8.7 instead of 12.8 KB for [[288,12,18]], 18 instead of 12 resident wavefronts per CU for
// a kernel that lives on hiding LDS latency); uint16 idx[NP]; int pivcol[m]; uint8 sol[n]
// (osd_lds_bytes).  WW = W + 1 at compile time (0: any width, at most 32 rows per lane).
__host__ __device__ inline size_t osd_lds_bytes(int m, int n, int W, int NP)
{
    return osd_region0_bytes(m, W, NP) + (size_t)NP * 2 + (size_t)m * 4 + (size_t)n + 16;
}

template <int WW>
__global__ __launch_bounds__(64) void osd0_kernel(const OsdParams P)
{
    extern __shared__ double osd_smem[];
    const int lane = threadIdx.x;
    // (row stride W + 1 words.  An odd stride -- 11 for n = 288 -- was measured: no gain, the two halves of a
    // wavefront are served separately and lanes l, l + 32 are the only ones an even stride maps to one bank)
    // (the row stride as a compile-time constant where the instantiation knows it: the ten accesses of a
    // row become wide LDS instructions)
    const int m = P.m, n = P.n, W = WW > 0 ? WW - 1 : P.W, NP = P.NP;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(osd_smem);
    uint32_t* A = reinterpret_cast<uint32_t*>(osd_smem);             // (after the sort: same bytes)
    uint16_t* idx = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(osd_smem) + osd_region0_bytes(m, W, NP));
    int* pivcol = reinterpret_cast<int*>(idx + NP);
    uint8_t* sol = reinterpret_cast<uint8_t*>(pivcol + m);

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        const long long rec = P.list ? P.list[item] : item;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;

        // ---- 1. ordering = argsort(|llr|), or the record's row of P.order       OSD.py:10-11
        osd_order_fill(P, rec, keys, idx, lane, 64);
        for (int i = lane; i < n; i += 64) sol[i] = hard[i] & 1u;
        __syncthreads();
        osd_sort(keys, idx, NP, lane, 64);
        // ---- 2. A = [H | residual syndrome], residual = syndrome + hard @ H.T  OSD.py:7-8
        // (A overwrites the sort keys: every lane passed the sort's last barrier)
        unsigned sb = osd_wave_load(P, syn, sol, A, pivcol, W, lane);   // bit i: reduced syndrome bit of row lane + 64 i
        __syncthreads();
        // ---- 3. Gauss-Jordan over the columns in reliability order            OSD.py:31-72
        int rank = 0;
        unsigned used = 0;                           // bit i: row lane + 64 i already serves as a pivot row
        // The sweep ends at the rank of H (:42-43 stops at m rows; rank(H) <= m) -- or as soon as no row without
        // a pivot has a 1 left in the syndrome column: every pivot found from there on would be chosen with a
        // reduced syndrome bit of 0, XOR nothing into the syndrome bits of the rows above it and put a 0 at its
        // own column, so the solution is already what the full sweep leaves.  (The residual syndrome of a BP
        // failure is light: the sweep typically ends after a small part of the columns.)
        for (int k = 0; k < n && rank < P.rank; ++k) {
            if (!__ballot((sb & ~used) != 0u)) break;
            const int c = idx[k];
#if QBP_OSD_ORDERED
            if (c >= n) continue;                    // (uniform) not a column: skipped
#endif
            unsigned has;
            const int p = osd_wave_find(A, m, W, c, lane, used, has);
            if (p < 0) continue;                     // column depends on earlier ones (:52-53)
            osd_wave_eliminate<WW>(A, m, W, p, has, lane, used, sb);
            ++rank;
            if (lane == 0) pivcol[p] = c;
            __syncthreads();
        }
        const bool inconsistent = __ballot((sb & ~used) != 0u) != 0ull;
        if (inconsistent && lane == 0) osd_flag_inconsistent(P, rec);
        // ---- 4. e[pivot column] = reduced syndrome bit; solution = hard + e    OSD.py:14-26
        osd_wave_solution(A, pivcol, sol, m, W, lane);
        __syncthreads();
        if (P.solution)
            for (int i = lane; i < n; i += 64) P.solution[rec * n + i] = sol[i];
        if (osd_counts_record(P, inconsistent)) osd_tail_wave(P, rec, sol, syn, lane);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// OSD-0 for matrices whose bit-packed rows do not fit the LDS of one wavefront's workgroup (space-time
// and circuit-level matrices: 2592 x 7776 is 2.5 MB per syndrome).  One workgroup per syndrome; the
// working copy of [H | residual syndrome] lives in a per-workgroup global workspace, stored TRANSPOSED
// (word w of row r at At[w * m + r]) so that the threads of a wavefront -- one matrix row each -- read
// and write consecutive addresses; sort keys in LDS when n <= 8192, else in the workspace too.
// Same algorithm and tie rules as osd0_kernel above, hence the same solutions (tested on the small
// codes, where both kernels apply) -- one pivot at a time, full-width rows, and the one kernel that follows the
// reference's row swaps: it serves matrices beyond 8192 rows and the records the fast kernels list in P.redo.
#ifdef QBP_DEFINE_KERNELS   /* non-template kernel: defined in its translation unit only */
__global__ __launch_bounds__(256) void osd0_big_kernel(const OsdParams P, const OsdBigWorkspace Wk)
{
    extern __shared__ double osd_smem[];
    __shared__ unsigned long long s_piv[2];   // (two slots, by column parity: see the pivot search)
    __shared__ OsdTally s_tally;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int m = P.m, n = P.n, W = P.W, NP = P.NP, RS = P.W + 1;
    unsigned long long* keys;
    int* idx;
    if (Wk.keys_in_lds) {
        keys = reinterpret_cast<unsigned long long*>(osd_smem);
        idx = reinterpret_cast<int*>(keys + NP);
    } else {
        keys = Wk.keys + (size_t)blockIdx.x * NP;
        idx = Wk.idx + (size_t)blockIdx.x * NP;
    }
    uint32_t* const At = Wk.At + (size_t)blockIdx.x * RS * m;
    int* const pivcol = Wk.pivcol + (size_t)blockIdx.x * m;
    int* const posn = Wk.posn + (size_t)blockIdx.x * 2 * m;        // position of row r in the swapped arrangement
    int* const rowat = posn + m;                                   // row at position q
    uint8_t* const sol = Wk.sol + (size_t)blockIdx.x * n;

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        const long long rec = P.list ? P.list[item] : item;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;
        // ---- 1. ordering = argsort(|llr|), or the record's row of P.order            OSD.py:10-11
        osd_order_fill(P, rec, keys, idx, tid, nt);
        for (int i = tid; i < n; i += nt) sol[i] = hard[i] & 1u;
        __syncthreads();
        osd_sort(keys, idx, NP, tid, nt);
        // ---- 2. A = [H | residual syndrome]                                         OSD.py:7-8
        for (int r = tid; r < m; r += nt) {
            for (int w = 0; w < W; ++w) At[(size_t)w * m + r] = P.hbits[(size_t)r * W + w];
            unsigned par = syn[r] & 1u;
            for (int e = P.row_ptr[r]; e < P.row_ptr[r + 1]; ++e) par ^= sol[P.col_idx[e]];
            At[(size_t)W * m + r] = par;
            pivcol[r] = -1;
            posn[r] = r;
            rowat[r] = r;
        }
        __syncthreads();
        // ---- 3. Gauss-Jordan over the columns in reliability order                  OSD.py:31-72
        // The pivot of a column is the first row at or below position `rank` of the reference's arrangement,
        // which swaps every pivot row up (:46-59): rows keep their place here and carry that position along.
        int rank = 0;
        for (int k = 0; k < n && rank < P.rank; ++k) {
#if QBP_OSD_ORDERED
            // (an entry that is no column goes through the search as a column without a 1 -- not around it: the two
            // slots of s_piv alternate with k)
            const int c = idx[k];
            const uint32_t* const colw = At + (size_t)((c < 0 ? 0 : c) >> 5) * m;
            const uint32_t bit = c < 0 ? 0u : 1u << (c & 31);
#else
            const int c = idx[k];
            const uint32_t* const colw = At + (size_t)(c >> 5) * m;
            const uint32_t bit = 1u << (c & 31);
#endif
            // (slot k & 1: a column without pivot leaves this iteration without a trailing barrier, so the
            // next column's reset must not touch the word the slower threads are still reading)
            unsigned long long* const piv = &s_piv[k & 1];
            if (tid == 0) *piv = ~0ull;
            __syncthreads();
            unsigned long long mine = ~0ull;          // (position, row)
            for (int r = tid; r < m; r += nt)
                if ((colw[r] & bit) && pivcol[r] < 0) {
                    const unsigned long long key = ((unsigned long long)(unsigned)posn[r] << 32) | (unsigned)r;
                    mine = key < mine ? key : mine;
                }
            if (mine != ~0ull) atomicMin(piv, mine);
            __syncthreads();
            const unsigned long long key = *piv;      // the first unused row with a 1 (:46-50)
            if (key == ~0ull) continue;               // column depends on earlier ones (:52-53)
            const int q = (int)(key >> 32), p = (int)(unsigned)key;
            if (tid == 0 && q != rank) {              // :56-59 (only this thread reads rowat; the trailing barrier
                                                      // publishes posn)
                const int r0 = rowat[rank];
                rowat[rank] = p; rowat[q] = r0;
                posn[p] = rank; posn[r0] = q;
            }
            ++rank;
            for (int r = tid; r < m; r += nt) {
                if (r != p && (colw[r] & bit)) {
                    // (the word holding bit c goes last: it is the loop's own condition for no one,
                    // but rows are independent, so any order is fine; keep it simple)
                    for (int w = 0; w <= W; ++w) At[(size_t)w * m + r] ^= At[(size_t)w * m + p];   // :63-68
                }
            }
            if (tid == 0) pivcol[p] = c;
            __syncthreads();
        }
        // ---- 4. e[pivot column] = reduced syndrome bit; solution = hard + e         OSD.py:14-26
        for (int r = tid; r < m; r += nt) {
            const int c = pivcol[r];
            if (c >= 0 && (At[(size_t)W * m + r] & 1u)) sol[c] ^= 1u;   // distinct pivot columns: no race
        }
        if (tid == 0) s_tally = OsdTally{};
        __syncthreads();
        if (P.solution)
            for (int i = tid; i < n; i += nt) P.solution[rec * n + i] = sol[i];
        // (this kernel lists no record: it is the one that follows the swaps)
        if (osd_counts_record(P, false)) osd_tail_block(P, rec, sol, syn, s_tally, tid, nt);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// The same OSD-0, eight pivots at a time (qbp_osd_parts.hpp, osd_block_*): the kernel for space-time /
// circuit-level matrices of up to 8192 rows.  One workgroup of 1024 threads per syndrome.
//
//  * A sweep ends as soon as no row without a pivot has a syndrome bit left (see osd0_kernel): after some 200
//    of the 5184 / 7776 columns on the BP failures of the tests' space-time matrices, 1632 at most.  So only
//    the first K = 1024 columns in reliability order are kept: the working copy holds H[:, order[:K]] in
//    SORTED column order, built from the CSR through the inverse permutation: 64-bit words, transposed
//    (word w of row r at At[w * m + r]: a wavefront's rows are consecutive), the residual syndrome bit in a
//    word plane of its own behind them.  A sweep that runs out of columns before it may end starts over with
//    4 K columns, then 16 K, ... n (tests force that path: QBP_OPT_OSD_BIG = 3 begins with K = 24).
//  * Same pivot columns as the row-at-a-time kernels (the greedy basis in reliability order does not depend
//    on the blocking), hence the same solutions: tests/test_gpu_osd.py compares all three kernels.
template <int RPT>
__global__ __launch_bounds__(1024) void osd0_blocked_kernel(const OsdParams P, const OsdBigWorkspace Wk)
{
    extern __shared__ double osd_smem[];
    __shared__ unsigned s_piv[3];
    __shared__ unsigned s_nact[2];
    __shared__ unsigned long long s_item;
    __shared__ OsdTally s_tally;
    typedef unsigned long long u64;
    const int tid = threadIdx.x, nt = 1024;
    const int m = P.m, n = P.n, NP = P.NP;
    char* const lds = reinterpret_cast<char*>(osd_smem);
    unsigned* const act = reinterpret_cast<unsigned*>(lds + Wk.lds_act);      // [m]: the rows a block updates
    u64* const table = reinterpret_cast<u64*>(lds);                        // region 0: keys -> pos -> table
    u64* const Qs = reinterpret_cast<u64*>(lds + Wk.lds_region0);          // [8][wc_max]
    u64* keys;
    int *idx, *pos;
    uint8_t* sol;
    if (Wk.keys_in_lds) {
        keys = reinterpret_cast<u64*>(lds);
        pos = reinterpret_cast<int*>(lds);
        idx = reinterpret_cast<int*>(lds + Wk.lds_region0 + (size_t)8 * Wk.wc_max * 8);
        sol = reinterpret_cast<uint8_t*>(idx + NP);
    } else {
        keys = Wk.keys + (size_t)blockIdx.x * NP;
        pos = reinterpret_cast<int*>(keys);
        idx = Wk.idx + (size_t)blockIdx.x * NP;
        sol = Wk.sol + (size_t)blockIdx.x * n;
    }
    u64* const At = reinterpret_cast<u64*>(Wk.At) + (size_t)blockIdx.x * Wk.wc_max * m;
    OSD_T0();
    if (tid < 3) s_piv[tid] = ~0u;
    if (tid < 2) s_nact[tid] = 0u;
    unsigned col_ctr = 0;                     // columns swept so far: slot col_ctr % 3 of s_piv is the live one
    unsigned blk_ctr = 0;                     // blocks with pivots so far: s_nact[blk_ctr & 1] counts this one's rows
    __syncthreads();

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    // (syndromes one at a time from a counter: a sweep takes anything between 0.3 and 20 ms)
    for (;;) {
        if (tid == 0) s_item = atomicAdd(Wk.next, 1ull);
        __syncthreads();
        const long long item = (long long)s_item;
        if (item >= total) break;
        const long long rec = P.list ? P.list[item] : item;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;
        // ---- 1. ordering = argsort(|llr|), or the record's row of P.order            OSD.py:10-11
        osd_order_fill(P, rec, keys, idx, tid, nt);
        for (int i = tid; i < n; i += nt) sol[i] = hard[i] & 1u;
        __syncthreads();
        osd_sort(keys, idx, NP, tid, nt);
        OSD_T(0);
        bool inconsistent = false;            // listed for the kernel that follows the row swaps
        int pc[RPT];                          // pivot column (original index) of this thread's rows, -1: none yet
        int Wc = 0;
        unsigned sb = 0;                      // bit i: reduced syndrome bit of row tid + i * nt
        for (int K = Wk.k_first < n ? Wk.k_first : n;; K = K < n / 4 ? 4 * K : n) {
            Wc = ((K + 63) >> 6) + 1;         // word planes: K sorted columns, then the syndrome bit
            // ---- 2. A = [H[:, order[:K]] | residual syndrome]                       OSD.py:7-11
#if QBP_OSD_ORDERED
            // (a column the row does not name gets position n: in no sweep's working copy)
            for (int c = tid; c < n; c += nt) pos[c] = n;
            __syncthreads();
            for (int k = tid; k < n; k += nt)
                if (idx[k] >= 0) pos[idx[k]] = k;
#else
            for (int k = tid; k < n; k += nt) pos[idx[k]] = k;
#endif
            __syncthreads();
            sb = 0;
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int r = tid + i * nt;
                pc[i] = -1;
                if (r >= m) continue;
                for (int w = 0; w < Wc - 1; ++w) At[(size_t)w * m + r] = 0ull;
                unsigned par = syn[r] & 1u;
                for (int e = P.row_ptr[r]; e < P.row_ptr[r + 1]; ++e) {
                    const int c = P.col_idx[e];
                    par ^= sol[c];
                    const int k = pos[c];
                    if (k < K) At[(size_t)(k >> 6) * m + r] |= 1ull << (k & 63);
                }
                At[(size_t)(Wc - 1) * m + r] = par;
                sb |= par << i;
            }
            __syncthreads();                  // (pos is dead from here on: the table takes its place)
            OSD_T(1);
            // ---- 3. Gauss-Jordan over the sorted columns, a block of T at a time    OSD.py:31-72
            // The sweep ends at the rank of H (:42-43) -- or as soon as no row without a pivot has a 1 left in
            // the syndrome column: pivots found from there on would be chosen with a reduced syndrome bit of 0,
            // which XORs nothing into the syndrome bits above them and puts a 0 at their own column, so the
            // solution is already what the full sweep would leave.  (BP's residual syndromes are light: the
            // sweep typically ends after a small part of the columns.)
            int rank = 0, k0 = 0;
            bool open_rows = true;
            while (k0 < K && rank < P.rank) {
                {
                    unsigned mine = 0;
#pragma unroll
                    for (int i = 0; i < RPT; ++i) mine |= (pc[i] < 0 ? 1u : 0u) & (sb >> i);
                    open_rows = __syncthreads_or((int)mine) != 0;
                    if (!open_rows) break;
                }
                const OsdBlock B = osd_block_shape(k0, K, Wc, Wk.lds_table);
                unsigned bd[RPT];
                int prow[8];
                osd_block_bytes<RPT>(At, m, B, bd, tid, nt);
                OSD_T(2);
                const bool any = osd_block_pivots<RPT>(idx, s_piv, k0, B.Tc, P.rank, rank, col_ctr, pc, bd, prow,
                                                       tid, nt);
                k0 += B.T;
                OSD_T(3);
                if (!any) continue;
                const unsigned* const nact = osd_block_act<RPT>(act, s_nact, blk_ctr, bd, tid, nt);
                osd_block_stage(Qs, At, m, B, prow, tid, nt);
                __syncthreads();
                OSD_T(4);
                osd_block_table(table, Qs, B, tid, nt);
                __syncthreads();
                OSD_T(5);
                osd_block_update<RPT>(At, m, table, act, (int)*nact, B, bd, sb, tid, nt);
                // (the barrier at the top of the next block comes before anyone reads a row again or
                // overwrites Qs / the table)
                OSD_SYNC();
                if (tid == 0) { OSD_STAT(0, 1); }
                OSD_T(6);
            }
            OSD_STAT(7, tid == 0 ? 1 : 0);
#ifdef QBP_OSD_TIMING
            if (tid == 0) atomicMax(&g_osd_stat[3], (unsigned long long)k0);
#endif
            if (open_rows) {                  // (the loop ended on one of its other conditions: look once more)
                unsigned mine = 0;
#pragma unroll
                for (int i = 0; i < RPT; ++i) mine |= (pc[i] < 0 ? 1u : 0u) & (sb >> i);
                open_rows = __syncthreads_or((int)mine) != 0;
            }
            OSD_STAT(4, tid == 0 ? k0 : 0); OSD_STAT(5, tid == 0 ? rank : 0); OSD_STAT(6, tid == 0 && !open_rows ? 1 : 0);
            if (rank >= P.rank || !open_rows || K >= n) {
                if (open_rows && tid == 0) osd_flag_inconsistent(P, rec);
                inconsistent = open_rows;
                break;
            }
            __syncthreads();                  // (next sweep: pos overwrites the table)
        }
        // ---- 4. e[pivot column] = reduced syndrome bit; solution = hard + e         OSD.py:14-26
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            // (sb: the thread's running copy of its rows' bits in the syndrome plane)
            if (pc[i] >= 0 && ((sb >> i) & 1u)) sol[pc[i]] ^= 1u;                     // distinct pivot columns
        }
        if (tid == 0) s_tally = OsdTally{};
        __syncthreads();
        if (P.solution)
            for (int i = tid; i < n; i += nt) P.solution[rec * n + i] = sol[i];
        if (osd_counts_record(P, inconsistent)) osd_tail_block(P, rec, sol, syn, s_tally, tid, nt);   // (uniform)
        __syncthreads();
        OSD_T(7);
    }
    OSD_TEND();
}

#endif  // QBP_DEFINE_KERNELS

}  // namespace qbp
