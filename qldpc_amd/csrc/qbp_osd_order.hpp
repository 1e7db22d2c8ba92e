// Order-w OSD on the GPU: the OSD-0 solution and a search over flip sets of the least reliable non-pivot
// columns (combination sweep "CS" or exhaustive "E"); the spec is in include/qbp.h (qbp_osd_batch) and DESIGN §3b.
//
// One wavefront per record, as osd0_kernel, with the same OsdParams (Monte-Carlo records, redo list).  The order, the
// elimination and the record's tail are osd0_kernel's -- the same pieces of qbp_osd_parts.hpp -- except that the sweep
// runs to the rank of H: the search needs the fully reduced matrix A, and its non-pivot columns T.  The search
// (steps 5-8) is this kernel's own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_osd.hpp"

namespace qbp {

enum { OSD_METHOD_CS = 1, OSD_METHOD_E = 2 };

// LDS of osd_order_kernel, in this order: { u64 keys[NP] | u32 A[m][W+1] } (osd_region0_bytes); u16 idx[NP];
// int pivcol[m]; double absl[n] (|llr| per column, the terms of the cost); u64 mask[m] (bit t of pivot row r:
// A[r][T[t]] for t < w'); int cinfo[n] (column c: its pivot row r >= 0, or ~t for T[t]); u16 T[n]; u8 sol[n].
struct OsdOrderLds {
    size_t idx, pivcol, absl, mask, cinfo, tcol, sol, total;
};
__host__ __device__ inline OsdOrderLds osd_order_lds(int m, int n, int W, int NP)
{
    OsdOrderLds L;
    L.idx = osd_region0_bytes(m, W, NP);
    L.pivcol = L.idx + (((size_t)NP * 2 + 3) & ~(size_t)3);
    L.absl = (L.pivcol + (size_t)m * 4 + 7) & ~(size_t)7;
    L.mask = L.absl + (size_t)n * 8;
    L.cinfo = L.mask + (size_t)m * 8;
    L.tcol = L.cinfo + (size_t)n * 4;
    L.sol = L.tcol + (size_t)n * 2;
    L.total = L.sol + (size_t)n + 16;
    return L;
}
__host__ __device__ inline size_t osd_order_lds_bytes(int m, int n, int W, int NP)
{
    return osd_order_lds(m, n, W, NP).total;
}

// Candidates besides OSD-0 (enumeration index 0): CS k' + w'(w'-1)/2, E 2^w' - 1.
__host__ __device__ inline long long osd_order_candidates(int method, int kp, int wp)
{
    return method == OSD_METHOD_CS ? (long long)kp + (long long)wp * (wp - 1) / 2 : (1ll << wp) - 1;
}

__device__ __forceinline__ int osd_binom(int a, int b)
{
    if (b < 0 || b > a) return 0;
    int r = 1;
    for (int i = 1; i <= b; ++i) r = r * (a - b + i) / i;   // (exact at every step; a <= 12 here)
    return r;
}

// Flip set of candidate `cand` (>= 1): bit t of *fm for T[t], t < w'; *tx = t >= w' for a CS weight-1 set beyond w'.
__device__ __forceinline__ void osd_flip_set(int method, int kp, int wp, long long cand, unsigned long long* fm,
                                             int* tx)
{
    *fm = 0ull;
    *tx = -1;
    long long q = cand - 1;
    if (method == OSD_METHOD_CS) {
        if (q < kp) {                                    // weight 1, all of T in order
            if (q < wp) *fm = 1ull << q; else *tx = (int)q;
            return;
        }
        q -= kp;                                         // weight 2 over T[0..w'): (a, b) in combinations order
        int a = 0;
        while (q >= wp - 1 - a) { q -= wp - 1 - a; ++a; }
        *fm = (1ull << a) | (1ull << (a + 1 + (int)q));
        return;
    }
    int k = 1;                                           // E: weight ascending, then combinations order
    for (int c; q >= (c = osd_binom(wp, k)); ++k) q -= c;
    int a = 0;
    for (int pos = 0; pos < k; ++pos) {
        for (;; ++a) {
            const int c = osd_binom(wp - 1 - a, k - 1 - pos);
            if (q < c) break;
            q -= c;
        }
        *fm |= 1ull << a;
        ++a;
    }
}

template <int WW>
__global__ __launch_bounds__(64) void osd_order_kernel(const OsdParams P, const int method, const int order)
{
    extern __shared__ double osd_smem[];
    const int lane = threadIdx.x;
    const int m = P.m, n = P.n, W = WW > 0 ? WW - 1 : P.W, NP = P.NP, RS = W + 1;
    const OsdOrderLds L = osd_order_lds(m, n, W, NP);
    char* const base = reinterpret_cast<char*>(osd_smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base);
    uint32_t* A = reinterpret_cast<uint32_t*>(base);                  // (after the sort: same bytes)
    uint16_t* idx = reinterpret_cast<uint16_t*>(base + L.idx);
    int* pivcol = reinterpret_cast<int*>(base + L.pivcol);
    double* absl = reinterpret_cast<double*>(base + L.absl);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(base + L.mask);
    int* cinfo = reinterpret_cast<int*>(base + L.cinfo);
    uint16_t* tcol = reinterpret_cast<uint16_t*>(base + L.tcol);
    uint8_t* sol = reinterpret_cast<uint8_t*>(base + L.sol);

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        const long long rec = P.list ? P.list[item] : item;
        const double* llr = P.llr + rec * n;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;

        // ---- 1. order: ascending (osd_order_key(llr), column), or the record's row of P.order
        osd_order_fill(P, rec, keys, idx, lane, 64);
        for (int i = lane; i < n; i += 64) {
            sol[i] = hard[i] & 1u;
            absl[i] = __builtin_fabs(llr[i]);
            cinfo[i] = -1;
        }
        __syncthreads();
        osd_sort(keys, idx, NP, lane, 64);
        // ---- 2. A = [H | residual syndrome], residual = syndrome + hard @ H.T
        unsigned sb = osd_wave_load(P, syn, sol, A, pivcol, W, lane);   // bit i: reduced syndrome bit of row lane + 64 i
        __syncthreads();
        // ---- 3. Gauss-Jordan in reliability order up to the rank of H (no early end: the search reads A)
        int rank = 0;
        unsigned used = 0;                           // bit i: row lane + 64 i already serves as a pivot row
        for (int k = 0; k < n && rank < P.rank; ++k) {
            const int c = idx[k];
#if QBP_OSD_ORDERED
            if (c >= n) continue;                    // (uniform) not a column: skipped
#endif
            unsigned has;
            const int p = osd_wave_find(A, m, W, c, lane, used, has);
            if (p < 0) continue;
            osd_wave_eliminate<WW>(A, m, W, p, has, lane, used, sb);
            ++rank;
            if (lane == 0) { pivcol[p] = c; cinfo[c] = p; }
            __syncthreads();
        }
        // a syndrome outside the column space: the OSD-0 output of the row-swapping kernel (redo list), no search
        const bool inconsistent = __ballot((sb & ~used) != 0u) != 0ull;
        if (inconsistent && lane == 0) osd_flag_inconsistent(P, rec);
        // ---- 4. OSD-0: e[pivot column] = reduced syndrome bit
        osd_wave_solution(A, pivcol, sol, m, W, lane);
        __syncthreads();
        if (!inconsistent) {
            // ---- 5. T = non-pivot columns in sort order (ordered builds: in the given order); cinfo[T[t]] = ~t
            int kp = 0;
            for (int b0 = 0; b0 < n; b0 += 64) {
                const int k = b0 + lane;
#if QBP_OSD_ORDERED
                const int c = k < n && idx[k] < n ? idx[k] : 0;
                const bool isT = k < n && idx[k] < n && cinfo[c] < 0;
#else
                const int c = k < n ? idx[k] : 0;
                const bool isT = k < n && cinfo[c] < 0;
#endif
                const unsigned long long bal = __ballot(isT);
                if (isT) {
                    const int t = kp + (int)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
                    tcol[t] = (uint16_t)c;
                    cinfo[c] = ~t;
                }
                kp += (int)__builtin_popcountll(bal);
            }
            const int wp = order < kp ? order : kp;
            __syncthreads();
            // ---- 6. per pivot row: A's entries on T[0..w') as a 64-bit mask
            for (int r = lane; r < m; r += 64) {
                unsigned long long mk = 0ull;
                if (pivcol[r] >= 0)
                    for (int t = 0; t < wp; ++t) {
                        const int c = tcol[t];
                        mk |= (unsigned long long)((A[r * RS + (c >> 5)] >> (c & 31)) & 1u) << t;
                    }
                mask[r] = mk;
            }
            __syncthreads();
            // ---- 7. candidates: lane l takes l, l + 64, ...; cost = sum of |llr| over the support, ascending
            //         column, in double from +0.0; best = smallest cost, ties to the lowest index, NaN never wins
            const long long ncand = 1 + osd_order_candidates(method, kp, wp);
            double bc = 0.0;
            long long bi = -1;                       // -1: no non-NaN candidate yet
            for (long long cand = lane; cand < ncand; cand += 64) {
                unsigned long long fm = 0ull;
                int tx = -1;
                if (cand > 0) osd_flip_set(method, kp, wp, cand, &fm, &tx);
                const int cx = tx >= 0 ? (int)tcol[tx] : 0;
                double cost = 0.0;
                for (int i = 0; i < n; ++i) {
                    const int ci = cinfo[i];
                    unsigned d;
                    if (ci >= 0) {
                        d = (unsigned)__builtin_popcountll(mask[ci] & fm) & 1u;
                        if (tx >= 0) d ^= (A[ci * RS + (cx >> 5)] >> (cx & 31)) & 1u;
                    } else {
                        const int t = ~ci;
                        d = (t < 64 ? (unsigned)(fm >> t) & 1u : 0u) | (t == tx ? 1u : 0u);
                    }
                    if (sol[i] ^ d) cost += absl[i];
                }
                if (cand == 0 && cost != cost) { bi = -2; break; }   // OSD-0's cost is NaN: OSD-0 wins outright
                if (cost == cost && (bi == -1 || cost < bc)) { bc = cost; bi = cand; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double oc = __shfl_xor(bc, off);
                const long long oi = __shfl_xor(bi, off);
                // -2 (NaN OSD-0) beats everything, -1 (nothing) loses to everything
                const bool take = oi == -2 ? bi != -2
                                : (oi >= 0 && bi != -2 && (bi < 0 || oc < bc || (oc == bc && oi < bi)));
                if (take) { bc = oc; bi = oi; }
            }
            // ---- 8. apply the winning flip set (bi is uniform across the wave after the reduction)
            if (bi > 0) {
                unsigned long long fm = 0ull;
                int tx = -1;
                osd_flip_set(method, kp, wp, bi, &fm, &tx);
                const int cx = tx >= 0 ? (int)tcol[tx] : 0;
                for (int r = lane; r < m; r += 64) {
                    const int c = pivcol[r];
                    if (c < 0) continue;
                    unsigned d = (unsigned)__builtin_popcountll(mask[r] & fm) & 1u;
                    if (tx >= 0) d ^= (A[r * RS + (cx >> 5)] >> (cx & 31)) & 1u;
                    if (d) sol[c] ^= 1u;
                }
                if (lane < wp && ((fm >> lane) & 1ull)) sol[tcol[lane]] ^= 1u;
                if (lane == 0 && tx >= 0) sol[cx] ^= 1u;
            }
            __syncthreads();
        }
        if (P.solution)
            for (int i = lane; i < n; i += 64) P.solution[rec * n + i] = sol[i];
        // ---- 9. the record's tail (a listed shot is the row-swapping kernel's record)
        if (osd_counts_record(P, inconsistent)) osd_tail_wave(P, rec, sol, syn, lane);
        __syncthreads();
    }
}

}  // namespace qbp
