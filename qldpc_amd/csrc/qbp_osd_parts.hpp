// The stages of "one record" of OSD / LSD post-processing, stated once for the six kernels that run them: osd0_kernel,
// osd0_big_kernel, osd0_blocked_kernel (qbp_osd.hpp), osd_order_kernel (qbp_osd_order.hpp), osd_order_blocked_kernel
// (qbp_osd_order_big.hpp) and lsd_kernel (qbp_lsd.hpp).
//
//   1. column order      osd_order_fill, osd_sort                       all six (LSD: never an ordered build)
//   2-4, one wavefront   osd_wave_load, osd_wave_find, osd_wave_eliminate, osd_wave_solution  osd0_kernel, osd_order_kernel, lsd_kernel
//   3, eight pivots      osd_block_shape / _bytes / _pivots / _act / _stage / _table / _update
//                                                                        osd0_blocked_kernel, osd_order_blocked_kernel
//   record tail          osd_tally, osd_tally_wave / osd_tally_block, osd_count_record  (osd_tail_wave, osd_tail_block)
// lsd_large_kernel (qbp_lsd_large.hpp) takes 1 and the workgroup's record tail; its rows live in a global workspace.
//
// Every piece is __forceinline__ and takes (tid, nt) -- (lane, 64) in the one-wavefront kernels -- and, where the
// kernels differ in it, the type of a column index (uint16_t in LDS, int in the workspace kernels).  None of them holds
// a barrier except osd_sort, osd_block_pivots (one per column) and osd_tail_block: the kernels keep the others where
// they were.  The statements are the ones every kernel used to carry as its own copy, but the instructions are not
// identical to those builds: the compiler simplifies a helper before it inlines it, so allocation and block order
// differ (profiles/r21_osd_isa.txt has the counts per kernel, r21_kernel_resources.txt the registers, r21_osd_ab.json
// the times against the copies).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_mc.hpp"

#ifndef QBP_OSD_SPECTRUM
// 1: the kernels that classify also add the residual weight of every record to OsdParams::spectrum
// (qbp_mc_run_spectrum).  Set by qbp_tu_osd.hip -DQBP_SPECTRUM_TU, which gives those kernels names of their own: the
// other builds keep their code, registers and LDS.
#define QBP_OSD_SPECTRUM 0
#endif

#ifndef QBP_OSD_SHOTS
// 1: the kernels' records are recorded shots (qbp_decode_shots): instead of classifying a residual they form the
// observable prediction Lx x of their solution x, store it and compare it with the shot's recorded observables.
// Set by qbp_tu_osd.hip -DQBP_SHOTS_TU, which gives those kernels names of their own: the other builds keep their code,
// registers and LDS.
#define QBP_OSD_SHOTS 0
#endif

#ifndef QBP_OSD_ORDERED
// 1: the column order is an input (OsdParams::order, qbp_osd_batch_ordered): step 1 of every kernel copies the
// record's row of it instead of sorting.  Set by qbp_tu_osd.hip -DQBP_ORDERED_TU, which gives those kernels names of
// their own: the other builds keep their code, registers and LDS.
#define QBP_OSD_ORDERED 0
#endif

namespace qbp {

struct OsdParams {
    // code
    int m, n, W;                    // W = 32-bit words per row of H ((n + 31) / 32)
    int NP;                         // power of two >= n (sort width)
    int rank;                       // rank of H over GF(2): no pivot exists beyond it
    const uint32_t* hbits;          // [m][W] bit-packed rows of H
    const int32_t* row_ptr;         // CSR of H
    const int32_t* col_idx;
    // batch: record index of syndrome i is list ? list[i] : i
    long long count;
    const long long* count_ptr;     // optional: number of records (device), overrides count
    const long long* list;
    const uint8_t* syndromes;       // [*][m]
    const double* llr;              // [*][n]
    const uint8_t* hard;            // [*][n]
    uint8_t* solution;              // [*][n] (may be null in Monte-Carlo mode)
    long long* redo;                // optional: [0] counts, [1..] lists the records whose sweep ended with a
                                    // syndrome bit left on a row without a pivot (see osd_flag_inconsistent)
    // Monte-Carlo classification (paperResults_GPU.py:127-144 on the OSD output)
    const uint8_t* errors;          // [*][n] or null
    const unsigned long long* lx_cols;
    int half_distance;
    long long* counters;
    // (last: QBP_OSD_SPECTRUM builds only) [SPECTRUM_ROWS][n + 1]: the weight w > 0 of a record's residual
    // solution ^ error is counted at [3][w] when the residual is a logical operator, else at [1][w] -- every
    // record here is a trial BP did not converge on (qbp_mc.hpp, mc_spectrum_row)
    long long* spectrum;
    // (last: QBP_OSD_SHOTS builds only; shots != 0 selects them) record `rec` is shot `rec` of the call: actual [*] (may
    // be null) the recorded observables, predictions [*] (may be null) written.  A record a fast kernel lists in redo is
    // left to the kernel that recomputes it: every shot is predicted and counted once.
    int shots;
    const unsigned long long* actual;
    unsigned long long* predictions;
    // (last: QBP_OSD_ORDERED builds only; non-null selects them) [*][n]: row `rec` is the order in which record `rec`
    // walks its columns, least reliable first -- a permutation of 0..n-1 (the host entry checks that; the _device entry
    // cannot).  The keys of |llr| then play no part in the order.  Memory safety for ANY int32 content: an entry outside
    // [0, n) is skipped; a repeated column is harmless (it is already eliminated: no unused row has a 1 there); a
    // column that never appears is never a pivot.  The output of such a row is unspecified, but nothing is read or
    // written out of bounds.
    const int32_t* order;
};

// Per-workgroup global workspace of the kernels for matrices whose rows do not fit LDS (osd0_big_kernel,
// osd0_blocked_kernel, osd_order_blocked_kernel).
struct OsdBigWorkspace {
    uint32_t* At;                   // [grid][(W + 1) * m]
    int32_t* pivcol;                // [grid][m]
    int32_t* posn;                  // [grid][2 m]: position of every row in the reference's swapped arrangement,
                                    // then the row at every position (osd0_big_kernel)
    uint8_t* sol;                   // [grid][n]
    unsigned long long* keys;       // [grid][NP]   (only when the keys do not fit LDS)
    int32_t* idx;                   // [grid][NP]
    int keys_in_lds;
    // osd0_blocked_kernel only (At: 64-bit words there, [grid][wc_max * m])
    int wc_max;                     // word planes of a full-width working copy: (n + 63) / 64 + 1
    int k_first;                    // sorted columns the first sweep keeps
    int lds_region0, lds_table;     // bytes: {keys | pos | table} region; the part of it the table may use
    int lds_act;                    // byte offset of the list of rows a block updates (m words)
    unsigned long long* next;       // work counter (zero at launch): syndromes are handed out one at a time
};

// The one-wavefront kernels keep the sort keys and, after the sort, the matrix in one LDS region:
// { u64 keys[NP] | uint32 A[m][W+1] }.
__host__ __device__ inline size_t osd_region0_bytes(int m, int W, int NP)
{
    const size_t a = (size_t)NP * 8, b = (size_t)m * (W + 1) * 4;
    return ((a > b ? a : b) + 7) & ~(size_t)7;
}

// A syndrome outside the column space of H (no error produces one; no caller of the reference passes one) ends its
// sweep with a 1 left in the syndrome column of a row without a pivot.  There, and only there, the reference's
// output depends on WHICH row served as the pivot of a column -- on its row swaps (OSD.py:56-59).  The fast kernels
// pick the first unused row in the original order; they list such a record in P.redo, and the host launches
// osd0_big_kernel, which follows the swaps, on the list (normally empty: the launch reads one counter and ends).
__device__ __forceinline__ void osd_flag_inconsistent(const OsdParams& P, long long rec)
{
    if (P.redo) {
        const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(P.redo), 1ull);
        P.redo[1 + at] = rec;
    }
}

// =====================================================================================================================
// 1. Column order: idx[0 .. n) = the columns, least reliable first                                    OSD.py:10-11
//
// Sorting builds: argsort(|llr|) by a bitonic network over (key, column) pairs; ties in |llr| fall back to the column
// index (the reference's np.argsort is unstable there; oracle/bp_oracle.c does the same); NaN sorts last, as in numpy;
// the padding up to the power of two NP sorts behind everything.
// Ordered builds (QBP_OSD_ORDERED): the record's row of P.order; (Idx)-1 -- 0xffff or -1 -- marks an entry outside
// [0, n), which every sweep skips, and the padding, which none reaches.  No keys, no network.
// A kernel fills its own per-column arrays next to osd_order_fill and puts ONE barrier between fill and sort.

// Sort key of |llr|: the IEEE bit pattern of a non-negative double is monotone as an unsigned
// integer (finite < inf < NaN), which is also numpy's order (np.argsort puts NaN last); every NaN
// gets the same pattern so that NaNs, like other ties, are ordered by column index.  A total order:
// the sorting network stays a permutation of the real columns whatever the LLRs contain.
__device__ __forceinline__ unsigned long long osd_order_key(double llr)
{
    const double a = __builtin_fabs(llr);
    return a != a ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(a);
}

__device__ __forceinline__ bool osd_less(unsigned long long ka, int ia, unsigned long long kb, int ib)
{
    return ka < kb || (ka == kb && ia < ib);
}

template <typename Idx, typename Params>
__device__ __forceinline__ void osd_order_fill(const Params& P, long long rec, unsigned long long* keys, Idx* idx,
                                               int tid, int nt)
{
    const int n = P.n, NP = P.NP;
#if QBP_OSD_ORDERED
    (void)keys;
    const int32_t* ord = P.order + rec * n;
    for (int i = tid; i < NP; i += nt) {
        const int c = i < n ? ord[i] : -1;
        idx[i] = (Idx)(c >= 0 && c < n ? c : -1);
    }
#else
    const double* llr = P.llr + rec * n;
    for (int i = tid; i < NP; i += nt) {
        keys[i] = i < n ? osd_order_key(llr[i]) : ~0ull;      // padding sorts behind everything
        idx[i] = (Idx)i;
    }
#endif
}

// (ends with a barrier whenever it does anything: the sorted idx is visible to every thread)
template <typename Idx>
__device__ __forceinline__ void osd_sort(unsigned long long* keys, Idx* idx, int NP, int tid, int nt)
{
#if !QBP_OSD_ORDERED
    for (int k = 2; k <= NP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < NP / 2; t += nt) {
                const int lo = ((t / j) * (2 * j)) + (t % j);   // element with bit j clear
                const int hi = lo + j;
                const bool up = (lo & k) == 0;
                const unsigned long long ka = keys[lo], kb = keys[hi];
                const int ia = idx[lo], ib = idx[hi];
                if (osd_less(kb, ib, ka, ia) == up) {
                    keys[lo] = kb; keys[hi] = ka; idx[lo] = (Idx)ib; idx[hi] = (Idx)ia;
                }
            }
            __syncthreads();
        }
    }
#endif
}

// =====================================================================================================================
// 2-4 for one wavefront: the bit-packed rows of A = [H | residual syndrome] in LDS, row stride W + 1 words, in their
// original column indexing; lane l owns rows l, l + 64, ... (at most 32 of them) and keeps one bit per owned row in
// registers: sb (the row's reduced syndrome bit) and used (the row already serves as a pivot).

// ---- 2. A = [H | residual syndrome], residual = syndrome + hard @ H.T; pivcol = -1            OSD.py:7-8
// Returns sb.  on_row(r, par): what else a kernel keeps per row (lsd_kernel: the seed clusters).
template <typename Params, typename OnRow>
__device__ __forceinline__ unsigned osd_wave_load(const Params& P, const uint8_t* syn, const uint8_t* sol, uint32_t* A,
                                                  int* pivcol, int W, int lane, const OnRow& on_row)
{
    const int m = P.m, RS = W + 1;
    unsigned sb = 0;
    for (int r = lane, i = 0; r < m; r += 64, ++i) {
        for (int w = 0; w < W; ++w) A[r * RS + w] = P.hbits[r * W + w];
        unsigned par = syn[r] & 1u;
        for (int e = P.row_ptr[r]; e < P.row_ptr[r + 1]; ++e) par ^= sol[P.col_idx[e]];
        A[r * RS + W] = par;
        sb |= par << i;
        pivcol[r] = -1;
        on_row(r, par);
    }
    return sb;
}
template <typename Params>
__device__ __forceinline__ unsigned osd_wave_load(const Params& P, const uint8_t* syn, const uint8_t* sol, uint32_t* A,
                                                  int* pivcol, int W, int lane)
{
    return osd_wave_load(P, syn, sol, A, pivcol, W, lane, [](int, unsigned) {});
}

// ---- 3, one column c, in two pieces with the kernel's own "no pivot: next column" between them.
// osd_wave_find: the pivot is the first row without one that has a 1 in column c (-1: the column depends on earlier
// ones, :52-53).  Per column one LDS read per owned row decides both the pivot search (ballot) and which rows take the
// XOR (has, bit i: row lane + 64 i has a 1 in column c).
// osd_wave_eliminate: row p becomes a pivot row (used) and is XORed into every other row with the bit (:63-68); the
// pivot row is read once (broadcast) into registers when it fits (WW = words per row incl. the syndrome word at
// compile time, 0: any width).  The caller notes the pivot and ends the column with a barrier.
__device__ __forceinline__ int osd_wave_find(const uint32_t* A, int m, int W, int c, int lane, unsigned used,
                                             unsigned& has)
{
    const int RS = W + 1;
    const int wi = c >> 5;
    const uint32_t bit = 1u << (c & 31);
    int p = -1;
    has = 0;
    for (int base = 0, i = 0; base < m; base += 64, ++i) {
        const int r = base + lane;
        const bool one = r < m && (A[r * RS + wi] & bit);
        has |= (one ? 1u : 0u) << i;
        const unsigned long long mask = __ballot(one && !((used >> i) & 1u));
        if (p < 0 && mask) p = base + (int)__builtin_ctzll(mask);
    }
    return p;
}

template <int WW>
__device__ __forceinline__ void osd_wave_eliminate(uint32_t* A, int m, int W, int p, unsigned has, int lane,
                                                   unsigned& used, unsigned& sb)
{
    const int RS = W + 1;
    if (lane == (p & 63)) used |= 1u << (p >> 6);
    if constexpr (WW > 0) {
        uint32_t prow[WW];
#pragma unroll
        for (int w = 0; w < WW; ++w) prow[w] = A[p * RS + w];
        for (int r = lane, i = 0; r < m; r += 64, ++i) {
            if (r != p && ((has >> i) & 1u)) {
#pragma unroll
                for (int w = 0; w < WW; ++w) A[r * RS + w] ^= prow[w];
                sb ^= (prow[WW - 1] & 1u) << i;
            }
        }
    } else {
        const unsigned ps = A[p * RS + W] & 1u;
        for (int r = lane, i = 0; r < m; r += 64, ++i) {
            if (r != p && ((has >> i) & 1u)) {
                for (int w = 0; w <= W; ++w) A[r * RS + w] ^= A[p * RS + w];
                sb ^= ps << i;
            }
        }
    }
}

// ---- 4. e[pivot column] = reduced syndrome bit; solution = hard + e (distinct pivot columns: no race)  OSD.py:14-26
template <typename OnRow>
__device__ __forceinline__ void osd_wave_solution(const uint32_t* A, const int* pivcol, uint8_t* sol, int m, int W,
                                                  int lane, const OnRow& on_row)
{
    const int RS = W + 1;
    for (int r = lane; r < m; r += 64) {
        const int c = pivcol[r];
        if (c >= 0 && (A[r * RS + W] & 1u)) sol[c] ^= 1u;
        on_row(r);
    }
}
__device__ __forceinline__ void osd_wave_solution(const uint32_t* A, const int* pivcol, uint8_t* sol, int m, int W,
                                                  int lane)
{
    osd_wave_solution(A, pivcol, sol, m, W, lane, [](int) {});
}

// =====================================================================================================================
// Record tail: what a kernel reports about the solution of one record.
//
// Classifying builds (paperResults_GPU.py:127-144 on the OSD output; every record is a trial BP did not converge on):
// with residual = solution ^ error,  lm = XOR of lx_cols over its support (non-zero: a logical error, counters 1, 8 and
// 3 | 4 by the weight ew of the error against half_distance), df = the residual is non-zero (0: counter 9; 1 on a valid
// non-logical record: counter 5), bad = H solution != syndrome (counter 10: never for a syndrome an error produces),
// and in QBP_OSD_SPECTRUM builds rw = the weight of the residual, counted in the spectrum row of mc_spectrum_row.
// QBP_OSD_SHOTS builds: lm = the observable prediction, XOR of lx_cols over the support of the solution itself,
// stored and compared with the recorded observables (a wrong prediction: counters 1 and 8); bad as above, where with
// recorded data a syndrome need not lie in the column space of H.
// (Not through mc_count_trial: that states counter 5 by BP's converged flag and counter 8 by its negation, and here 5
// hangs on the validity of the OSD output while 8 goes with every logical error.)
struct OsdTally {
    unsigned long long lm;
    unsigned bad;
#if !QBP_OSD_SHOTS
    int ew;
    unsigned df;
#endif
#if QBP_OSD_SPECTRUM
    int rw;
#endif
};

// One thread's share: columns tid, tid + nt, ... and the H solution == syndrome check of rows tid, tid + nt, ...
template <typename Params>
__device__ __forceinline__ OsdTally osd_tally(const Params& P, long long rec, const uint8_t* sol, const uint8_t* syn,
                                              int tid, int nt)
{
    const int m = P.m, n = P.n;
    OsdTally t = {};
#if QBP_OSD_SHOTS
    for (int i = tid; i < n; i += nt)
        if (sol[i]) t.lm ^= P.lx_cols[i];
#else
    const uint8_t* err = P.errors + rec * n;
    for (int i = tid; i < n; i += nt) {
        const unsigned e = err[i] & 1u;
        const unsigned res = sol[i] ^ e;
        t.ew += (int)e;
        t.df |= res;
#if QBP_OSD_SPECTRUM
        t.rw += (int)res;
#endif
        if (res) t.lm ^= P.lx_cols[i];
    }
#endif
    for (int r = tid; r < m; r += nt) {      // is_valid_osd: (detection @ H.T) % 2 == syndrome
        unsigned par = syn[r] & 1u;
        for (int e = P.row_ptr[r]; e < P.row_ptr[r + 1]; ++e) par ^= sol[P.col_idx[e]];
        t.bad |= par;
    }
    return t;
}

// The sum over one wavefront, by shuffles: every lane ends with the record's tally.
__device__ __forceinline__ void osd_tally_wave(OsdTally& t)
{
    for (int off = 32; off > 0; off >>= 1) {
        t.lm ^= __shfl_xor(t.lm, off);
#if !QBP_OSD_SHOTS
        t.ew += __shfl_xor(t.ew, off);
        t.df |= __shfl_xor(t.df, off);
#endif
        t.bad |= __shfl_xor(t.bad, off);
#if QBP_OSD_SPECTRUM
        t.rw += __shfl_xor(t.rw, off);
#endif
    }
}

// The sum over a workgroup, by LDS atomics into `s` (zeroed by one thread, a barrier ago; complete a barrier later).
__device__ __forceinline__ void osd_tally_block(OsdTally& s, const OsdTally& t)
{
#if QBP_OSD_SPECTRUM
    if (t.rw) atomicAdd(&s.rw, t.rw);
#endif
    if (t.lm) atomicXor(&s.lm, t.lm);
#if !QBP_OSD_SHOTS
    if (t.ew) atomicAdd(&s.ew, t.ew);
    if (t.df) atomicOr(&s.df, 1u);
#endif
    if (t.bad) atomicOr(&s.bad, 1u);
}

// The record's tally into the call's counters, by one thread.
template <typename Params>
__device__ __forceinline__ void osd_count_record(const Params& P, long long rec, const OsdTally& t)
{
    auto add = [&](int i) { atomicAdd(reinterpret_cast<unsigned long long*>(P.counters + i), 1ull); };
#if QBP_OSD_SHOTS
    if (P.predictions) P.predictions[rec] = t.lm;
    if (P.actual && P.actual[rec] != t.lm) { add(1); add(8); }
#else
    const bool logical = t.lm != 0ull;
#if QBP_OSD_SPECTRUM
    if (t.rw)
        atomicAdd(reinterpret_cast<unsigned long long*>(
                      P.spectrum + (long long)mc_spectrum_row(false, logical) * (P.n + 1) + t.rw), 1ull);
#endif
    if (!t.bad && !logical && t.df) add(5);
    if (logical) {
        add(1);
        add(t.ew < P.half_distance ? 3 : 4);
        add(8);
    }
    if (!t.df) add(9);
#endif
    if (t.bad) add(10);
}

// Does this launch count the record?  Classifying builds: when it was given the errors.  Shots builds: always, except
// a record this kernel has listed in P.redo (redo_listed: its sweep ended inconsistent) -- the kernel that recomputes
// it predicts it, so every shot is predicted and counted once.
__device__ __forceinline__ bool osd_counts_record(const OsdParams& P, bool redo_listed)
{
#if QBP_OSD_SHOTS
    return !(redo_listed && P.redo != nullptr);
#else
    return P.errors != nullptr;
#endif
}

// The whole tail of a one-wavefront kernel, and of a workgroup kernel (`s`: its __shared__ tally, zeroed by one thread
// before the kernel's last barrier; one barrier inside, so the call is uniform).
template <typename Params>
__device__ __forceinline__ void osd_tail_wave(const Params& P, long long rec, const uint8_t* sol, const uint8_t* syn,
                                              int lane)
{
    OsdTally t = osd_tally(P, rec, sol, syn, lane, 64);
    osd_tally_wave(t);
    if (lane == 0) osd_count_record(P, rec, t);
}

template <typename Params>
__device__ __forceinline__ void osd_tail_block(const Params& P, long long rec, const uint8_t* sol, const uint8_t* syn,
                                               OsdTally& s, int tid, int nt)
{
    osd_tally_block(s, osd_tally(P, rec, sol, syn, tid, nt));
    __syncthreads();
    if (tid == 0) osd_count_record(P, rec, s);
}

// =====================================================================================================================
// 3, eight pivots at a time ("four Russians" blocking of the Gauss-Jordan sweep), for the 1024-thread kernels on a
// working copy in SORTED column order, 64-bit word planes, transposed (word w of row r at At[w * m + r]); thread tid
// owns rows tid + i * nt, i < RPT.
//
// A block is T <= 8 neighbouring columns inside one word.  Every thread keeps the T bits of its rows in a register (a
// "byte"), and the sweep over the block's columns works on those bytes alone: per column one LDS atomicMin (first
// not-yet-used row with the bit: decoding/OSD.py:46-50) and ONE barrier; a row that has the bit XORs the pivot's byte
// into its own and notes which of the block's pivot rows it has to take (D, a T-bit set over the pivot rows AS THEY
// WERE WHEN THE BLOCK BEGAN; a pivot row's own D at the moment it is chosen travels with it through the atomicMin
// word).  Then the block's pivot rows go to LDS, all 2^T XOR combinations of them are tabulated there, and every row
// of the matrix is updated ONCE: row ^= table[D].  Global traffic per block: one read-modify-write of the live word
// planes instead of one per pivot.  Sorted order means a column is never looked at again once it is passed: row
// operations only touch the word planes from the block's on.
#ifdef QBP_DEFINE_KERNELS   /* (with the kernels that use them: the timing build's counters are defined once) */

#ifdef QBP_OSD_TIMING   /* tools/osd_phases.py: cycles of thread 0 per phase, summed over workgroups */
__device__ unsigned long long g_osd_timing[8];
#define OSD_T0() long long t_prev = clock64(); unsigned long long t_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define OSD_T(i) do { const long long t_now = clock64(); t_acc[i] += (unsigned long long)(t_now - t_prev); t_prev = t_now; } while (0)
#define OSD_TEND() do { if (threadIdx.x == 0) for (int q = 0; q < 8; ++q) atomicAdd(&g_osd_timing[q], t_acc[q]); } while (0)
__device__ unsigned long long g_osd_stat[8];   /* blocks, active rows, live words of active rows, columns swept */
#define OSD_STAT(i, v) atomicAdd(&g_osd_stat[i], (unsigned long long)(v))
#define OSD_SYNC() __syncthreads()
#else
#define OSD_STAT(i, v) do {} while (0)
#define OSD_SYNC() do {} while (0)
#define OSD_T0() do {} while (0)
#define OSD_T(i) do {} while (0)
#define OSD_TEND() do {} while (0)
#endif

// The block that begins at sorted column k0 of a working copy of Wc word planes whose columns end at kend: it lies in
// word plane wk from bit sh on, nw planes are live, T columns wide (as many as the table of 2^T rows of nw words has
// room for in lds_table bytes), Tc of them real.
struct OsdBlock {
    int wk, sh, nw, T, Tc;
};
__device__ __forceinline__ OsdBlock osd_block_shape(int k0, int kend, int Wc, int lds_table)
{
    OsdBlock B;
    B.wk = k0 >> 6; B.sh = k0 & 63; B.nw = Wc - B.wk;
    B.T = 8;
    while (B.T > 1 && ((k0 & (B.T - 1)) || ((size_t)B.nw << B.T) * 8 > (size_t)lds_table)) B.T >>= 1;
    B.Tc = kend - k0 < B.T ? kend - k0 : B.T;
    return B;
}

// bd: bits 0-7 the row's bits in the block's columns, bits 8-15 its set D (empty)
template <int RPT>
__device__ __forceinline__ void osd_block_bytes(const unsigned long long* At, int m, const OsdBlock& B,
                                                unsigned (&bd)[RPT], int tid, int nt)
{
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = tid + i * nt;
        bd[i] = r < m ? (unsigned)(At[(size_t)B.wk * m + r] >> B.sh) & ((1u << B.Tc) - 1u) : 0u;
    }
}

// The pivots of the block's columns k0 + j, on the bytes: prow[j] = the pivot row of column j (-1: none), pc[i] = the
// pivot column (original index) of a row that became one.  s_piv: three LDS words, ~0u at launch; slot col_ctr % 3 is
// the live one (col_ctr: columns swept so far in this workgroup's life).  Returns whether the block has a pivot.
template <int RPT>
__device__ __forceinline__ bool osd_block_pivots(const int* idx, unsigned* s_piv, int k0, int Tc, int max_rank,
                                                 int& rank, unsigned& col_ctr, int (&pc)[RPT], unsigned (&bd)[RPT],
                                                 int (&prow)[8], int tid, int nt)
{
    typedef unsigned long long u64;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        prow[j] = -1;
        if (j >= Tc || rank >= max_rank) continue;        // (uniform)
        // (this wavefront's first candidate through ballot + readlane, then one LDS atomic per
        // wavefront: a thousand lanes on one LDS word took 8 000 cycles per column)
        unsigned cand = ~0u;
#pragma unroll
        for (int i = RPT - 1; i >= 0; --i) {
            const u64 b = __ballot(pc[i] < 0 && ((bd[i] >> j) & 1u));
            if (b) {
                const int l = __builtin_ctzll(b);
                const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)bd[i], l);
                cand = ((unsigned)((tid & ~63) + l + i * nt) << 16) | v;
            }
        }
        unsigned* const slot = &s_piv[col_ctr % 3u];
        if ((tid & 63) == 0 && cand != ~0u) atomicMin(slot, cand);
        __syncthreads();
        const unsigned key = *slot;                       // first unused row with a 1 (:46-50)
        if (tid == 0) s_piv[(col_ctr + 2u) % 3u] = ~0u;   // (the slot of two columns ahead: idle now)
        ++col_ctr;
        if (key == ~0u) continue;                         // depends on earlier columns (:52-53)
        ++rank;
        any = true;
        const int p = (int)(key >> 16);
        // (the pivot's byte into the low bits, pivot j plus the pivot's own pending set into D)
        const unsigned upd = (key & 0xffffu) | (0x100u << j);
        prow[j] = p;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int r = tid + i * nt;
            if (r == p) pc[i] = idx[k0 + j];
            else if ((bd[i] >> j) & 1u) bd[i] ^= upd;                           // :63-68, on the bytes
        }
    }
    return any;
}

// The rows this block changes, as (row, D) words in LDS: the update is spread over all threads (a block touches some
// 40 of the rows of a sparse matrix).  s_nact: two LDS words, zero at launch; s_nact[blk_ctr & 1] counts this block's
// rows (blk_ctr: blocks with pivots so far).  Returns that counter: complete after the caller's next barrier.
template <int RPT>
__device__ __forceinline__ const unsigned* osd_block_act(unsigned* act, unsigned* s_nact, unsigned& blk_ctr,
                                                         const unsigned (&bd)[RPT], int tid, int nt)
{
    typedef unsigned long long u64;
    unsigned* const nact = &s_nact[blk_ctr & 1u];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const bool a = (bd[i] >> 8) != 0u;
        const u64 b = __ballot(a);
        if (b) {
            unsigned base = 0;
            if ((tid & 63) == 0) base = atomicAdd(nact, (unsigned)__builtin_popcountll(b));
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            if (a) act[base + (unsigned)__builtin_popcountll(b & ((1ull << (tid & 63)) - 1ull))] =
                       ((unsigned)(tid + i * nt) << 8) | (bd[i] >> 8);
        }
    }
    if (tid == 0) s_nact[(blk_ctr + 1u) & 1u] = 0u;       // (the next block's counter: idle now)
    ++blk_ctr;
    return nact;
}

// The block's pivot rows as they were when the block began -> LDS, Qs [8][nw]
__device__ __forceinline__ void osd_block_stage(unsigned long long* Qs, const unsigned long long* At, int m,
                                                const OsdBlock& B, const int (&prow)[8], int tid, int nt)
{
    const int nw = B.nw;
    for (int it = tid; it < 8 * nw; it += nt) {
        const int j = it / nw, w = it - j * nw;
        int p = -1;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q == j) p = prow[q];
        Qs[it] = p >= 0 ? At[(size_t)(B.wk + w) * m + p] : 0ull;
    }
}

// Every XOR combination of them: table [2^T][nw]
__device__ __forceinline__ void osd_block_table(unsigned long long* table, const unsigned long long* Qs,
                                                const OsdBlock& B, int tid, int nt)
{
    typedef unsigned long long u64;
    const int nw = B.nw, T = B.T;
    if (T == 8) {
        // an item: word w, the eight entries x = 8 xh .. 8 xh + 7 (Gray order over the low three rows)
        for (int it = tid; it < nw * 32; it += nt) {
            const int xh = it / nw, w = it - xh * nw;
            u64 v = 0ull;
#pragma unroll
            for (int j = 3; j < 8; ++j) if ((xh >> (j - 3)) & 1) v ^= Qs[j * nw + w];
            const u64 q0 = Qs[w], q1 = Qs[nw + w], q2 = Qs[2 * nw + w];
            u64* const t = table + (size_t)(xh * 8) * nw + w;
            t[0] = v;                     v ^= q0;
            t[(size_t)1 * nw] = v;        v ^= q1;
            t[(size_t)3 * nw] = v;        v ^= q0;
            t[(size_t)2 * nw] = v;        v ^= q2;
            t[(size_t)6 * nw] = v;        v ^= q0;
            t[(size_t)7 * nw] = v;        v ^= q1;
            t[(size_t)5 * nw] = v;        v ^= q0;
            t[(size_t)4 * nw] = v;
        }
    } else {
        for (int it = tid; it < (nw << T); it += nt) {
            const int x = it / nw, w = it - x * nw;
            u64 v = 0ull;
#pragma unroll
            for (int j = 0; j < 8; ++j) if ((x >> j) & 1) v ^= Qs[j * nw + w];
            table[it] = v;
        }
    }
}

// row ^= table[D] for the na rows of the act list, over the live planes, four items in flight per thread; sb follows
// from the table's syndrome plane for this thread's own rows.
// (QBP_OSD_TIMING builds: g_osd_stat[1] and [2] count here for whichever kernel calls -- osd_order_blocked_kernel too;
// tools/osd_phases.py launches OSD-0 only, so what it reads is still osd0_blocked_kernel's.)
template <int RPT>
__device__ __forceinline__ void osd_block_update(unsigned long long* At, int m, const unsigned long long* table,
                                                 const unsigned* act, int na, const OsdBlock& B,
                                                 const unsigned (&bd)[RPT], unsigned& sb, int tid, int nt)
{
    typedef unsigned long long u64;
    const int nw = B.nw, wk = B.wk;
#pragma unroll
    for (int i = 0; i < RPT; ++i)
        if (bd[i] >> 8) sb ^= ((unsigned)table[(size_t)(bd[i] >> 8) * nw + nw - 1] & 1u) << i;
    const int items = na * nw;
    OSD_STAT(1, tid == 0 ? na : 0); OSD_STAT(2, tid == 0 ? items : 0);
    for (int it0 = tid; it0 < items; it0 += 4 * nt) {
        u64 v[4], t[4];
        u64* a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int it = it0 + q * nt;
            if (it < items) {
                const int w = it / na;
                const unsigned e = act[it - w * na];
                a[q] = At + (size_t)(wk + w) * m + (e >> 8);
                t[q] = table[(size_t)(e & 0xffu) * nw + w];
                v[q] = *a[q];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (it0 + q * nt < items) *a[q] = v[q] ^ t[q];
    }
}

#endif  // QBP_DEFINE_KERNELS

}  // namespace qbp
