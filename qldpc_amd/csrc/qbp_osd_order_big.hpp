// Order-w OSD for matrices beyond the one-wavefront kernel (QBP_FLAG_OSD_LARGE): osd0_blocked_kernel's sort, working
// copy and eight-pivots-at-a-time Gauss-Jordan, run to the rank of H over the full width, then osd_order_kernel's
// candidate search.  The spec is in include/qbp.h (qbp_osd_batch) and DESIGN §3b.
//
// One workgroup of 1024 threads per record; the working copy is H[:, order] in SORTED column order, 64-bit word
// planes, transposed, in the per-workgroup global workspace (qbp_osd_parts.hpp).  The sweep only touches the word planes
// from the current block on, and that is exact: a pivot row is zero left of its pivot column (earlier pivot columns
// were cleared in it; an earlier non-pivot column had no 1 in any row without a pivot when the sweep passed it), so
// the reduced column of a non-pivot column is final once the sweep has passed it.  The search reads those columns
// straight from the workspace.
// The order, the blocks of the sweep (osd_block_*) and the record's tail are the pieces of qbp_osd_parts.hpp that
// osd0_blocked_kernel is built from; the search (steps 5-8) is this kernel's own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_osd.hpp"
#include "qbp_osd_order.hpp"

namespace qbp {

// What the search adds to OsdBigWorkspace.  Per column c, after the sweep: cm[c] (u64) -- a pivot column: bit t =
// A[its pivot row][T[t]] for t < w'; T[t] itself: 1 << t for t < w', else 0 -- so that a flip set F within T[0..w')
// changes x_c by parity(cm[c] & F) whatever c is; cinfo[c] (int32) -- the pivot row of a pivot column, else -1.
// Both overlay the dead {keys | pos | table} and pivot-row regions of the LDS (12 n bytes) unless `spill`: then cm
// takes the workspace of the sort keys and cinfo the second half of `tk`.
struct OsdOrderBigArgs {
    int method, order;              // OSD_METHOD_CS / _E, w
    int spill;
    int32_t* tk;                    // [grid][2 n]: sorted position of T[t]; then cinfo when spilled
};

#ifdef QBP_DEFINE_KERNELS

template <int RPT>
__global__ __launch_bounds__(1024) void osd_order_blocked_kernel(const OsdParams P, const OsdBigWorkspace Wk,
                                                                 const OsdOrderBigArgs X)
{
    extern __shared__ double osd_smem[];
    __shared__ unsigned s_piv[3];
    __shared__ unsigned s_nact[2];
    __shared__ unsigned long long s_item, s_best;
    __shared__ OsdTally s_tally;              // (the search borrows .lm and .bad: the tail zeroes them first)
    typedef unsigned long long u64;
    const int tid = threadIdx.x, nt = 1024;
    const int m = P.m, n = P.n, NP = P.NP;
    char* const lds = reinterpret_cast<char*>(osd_smem);
    unsigned* const act = reinterpret_cast<unsigned*>(lds + Wk.lds_act);      // [m]: the rows a block updates
    u64* const table = reinterpret_cast<u64*>(lds);                        // region 0: keys -> pos -> table -> cm
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
    int32_t* const tk = X.tk + (size_t)blockIdx.x * 2 * n;
    u64* const cm = X.spill ? Wk.keys + (size_t)blockIdx.x * NP : reinterpret_cast<u64*>(lds);
    int32_t* const cinfo = X.spill ? tk + n : reinterpret_cast<int32_t*>(lds + (size_t)n * 8);
    const int method = X.method;
    if (tid < 3) s_piv[tid] = ~0u;
    if (tid < 2) s_nact[tid] = 0u;
    unsigned col_ctr = 0;                     // columns swept so far: slot col_ctr % 3 of s_piv is the live one
    unsigned blk_ctr = 0;                     // blocks with pivots so far: s_nact[blk_ctr & 1] counts this one's rows
    __syncthreads();

    const long long total = P.count_ptr ? *P.count_ptr : P.count;
    for (;;) {
        if (tid == 0) s_item = atomicAdd(Wk.next, 1ull);
        __syncthreads();
        const long long item = (long long)s_item;
        if (item >= total) break;
        const long long rec = P.list ? P.list[item] : item;
        const double* llr = P.llr + rec * n;
        const uint8_t* hard = P.hard + rec * n;
        const uint8_t* syn = P.syndromes + rec * m;
        // ---- 1. ordering = argsort(|llr|), ties by column index, or the record's row of P.order
        osd_order_fill(P, rec, keys, idx, tid, nt);
        for (int i = tid; i < n; i += nt) sol[i] = hard[i] & 1u;
        __syncthreads();
        osd_sort(keys, idx, NP, tid, nt);
        int pc[RPT];                          // pivot column (original index) of this thread's rows, -1: none yet
        unsigned sb = 0;                      // bit i: reduced syndrome bit of row tid + i * nt
        const int Wc = Wk.wc_max;             // word planes: all n sorted columns, then the syndrome bit
        // ---- 2. A = [H[:, order] | residual syndrome], full width
#if QBP_OSD_ORDERED
        // (a column the row does not name gets position n: not in the working copy)
        for (int c = tid; c < n; c += nt) pos[c] = n;
        __syncthreads();
        for (int k = tid; k < n; k += nt)
            if (idx[k] >= 0) pos[idx[k]] = k;
#else
        for (int k = tid; k < n; k += nt) pos[idx[k]] = k;
#endif
        __syncthreads();
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
                if (k < n) At[(size_t)(k >> 6) * m + r] |= 1ull << (k & 63);
            }
            At[(size_t)(Wc - 1) * m + r] = par;
            sb |= par << i;
        }
        // ---- 3. Gauss-Jordan over the sorted columns, a block of T at a time, as osd0_blocked_kernel -- up to the
        //         rank of H, no early end: the search reads the reduced non-pivot columns
        int rank = 0, k0 = 0;
        while (k0 < n && rank < P.rank) {
            // (before anyone reads a row again or overwrites pos / Qs / the table)
            __syncthreads();
            const OsdBlock B = osd_block_shape(k0, n, Wc, Wk.lds_table);
            unsigned bd[RPT];
            int prow[8];
            osd_block_bytes<RPT>(At, m, B, bd, tid, nt);
            const bool any = osd_block_pivots<RPT>(idx, s_piv, k0, B.Tc, P.rank, rank, col_ctr, pc, bd, prow, tid, nt);
            k0 += B.T;
            if (!any) continue;
            const unsigned* const nact = osd_block_act<RPT>(act, s_nact, blk_ctr, bd, tid, nt);
            osd_block_stage(Qs, At, m, B, prow, tid, nt);
            __syncthreads();
            osd_block_table(table, Qs, B, tid, nt);
            __syncthreads();
            osd_block_update<RPT>(At, m, table, act, (int)*nact, B, bd, sb, tid, nt);
        }
        // a syndrome outside the column space: the OSD-0 output of the row-swapping kernel (redo list), no search
        bool inconsistent;
        {
            unsigned mine = 0;
#pragma unroll
            for (int i = 0; i < RPT; ++i) mine |= (pc[i] < 0 ? 1u : 0u) & (sb >> i);
            inconsistent = __syncthreads_or((int)mine) != 0;      // (and: the last block's rows are written)
        }
        if (inconsistent && tid == 0) osd_flag_inconsistent(P, rec);
        // ---- 4. OSD-0: e[pivot column] = reduced syndrome bit
#pragma unroll
        for (int i = 0; i < RPT; ++i)
            if (pc[i] >= 0 && ((sb >> i) & 1u)) sol[pc[i]] ^= 1u;                     // distinct pivot columns
        if (!inconsistent) {              // (uniform)
            // ---- 5. per column: pivot row; T = non-pivot columns in sort order (ordered builds: the given order)
            for (int i = tid; i < n; i += nt) { cm[i] = 0ull; cinfo[i] = -1; }
            if (tid == 0) { s_tally.lm = ~0ull; s_best = ~0ull; s_tally.bad = 0u; }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < RPT; ++i)
                if (pc[i] >= 0) cinfo[pc[i]] = tid + i * nt;
            __syncthreads();
            int kp = 0;                       // (every wavefront counts, the first one writes)
            for (int b0 = 0; b0 < n; b0 += 64) {
                const int k = b0 + (tid & 63);
                const int c = k < n ? idx[k] : -1;
                const bool isT = c >= 0 && cinfo[c] < 0;
                const u64 bal = __ballot(isT);
                if (isT && tid < 64) {
                    const int t = kp + (int)__builtin_popcountll(bal & ((1ull << tid) - 1ull));
                    tk[t] = k;
                    if (t < X.order) cm[c] = 1ull << t;
                }
                kp += (int)__builtin_popcountll(bal);
            }
            const int wp = X.order < kp ? X.order : kp;
            __syncthreads();
            // ---- 6. per pivot row: A's entries on T[0..w') as a 64-bit mask, kept under the row's pivot column
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                if (pc[i] < 0) continue;
                const int r = tid + i * nt;
                u64 mk = 0ull;
                for (int t = 0; t < wp; ++t) {
                    const int k = tk[t];
                    mk |= ((At[(size_t)(k >> 6) * m + r] >> (k & 63)) & 1ull) << t;
                }
                cm[pc[i]] = mk;
            }
            __syncthreads();
            // ---- 7. candidates: thread t takes t, t + 1024, ...; cost = sum of |llr| over the support, ascending
            //         column, in double from +0.0, by this thread alone
            const long long ncand = 1 + osd_order_candidates(method, kp, wp);
            double bc = 0.0;
            long long bi = -1;                // -1: no non-NaN candidate yet, -2: OSD-0's cost is NaN
            for (long long cand = tid; cand < ncand; cand += nt) {
                u64 fm = 0ull;
                int tx = -1;
                if (cand > 0) osd_flip_set(method, kp, wp, cand, &fm, &tx);
                double cost = 0.0;
                if (tx < 0) {
                    for (int i = 0; i < n; ++i) {
                        const unsigned d = (unsigned)__builtin_popcountll(cm[i] & fm) & 1u;
                        if ((sol[i] ^ d) & 1u) cost += __builtin_fabs(llr[i]);
                    }
                } else {
                    // a CS weight-1 set beyond w': the pivot rows' bits from the column's plane in the workspace
                    const int kx = tk[tx], cx = idx[kx], sh = kx & 63;
                    const u64* const colp = At + (size_t)(kx >> 6) * m;
                    for (int i = 0; i < n; ++i) {
                        const int r = cinfo[i];
                        const unsigned d = r >= 0 ? (unsigned)(colp[r] >> sh) & 1u : (i == cx ? 1u : 0u);
                        if ((sol[i] ^ d) & 1u) cost += __builtin_fabs(llr[i]);
                    }
                }
                if (cand == 0 && cost != cost) { bi = -2; break; }   // OSD-0's cost is NaN: OSD-0 wins outright
                if (cost == cost && (bi == -1 || cost < bc)) { bc = cost; bi = cand; }
            }
            // least cost (a sum of fabs from +0.0: its bit pattern is monotone), then the lowest index at that cost
            const u64 bcb = (u64)__double_as_longlong(bc);
            if (bi == -2) s_tally.bad = 1u;
            if (bi >= 0) atomicMin(&s_tally.lm, bcb);
            __syncthreads();
            if (bi >= 0 && bcb == s_tally.lm) atomicMin(&s_best, (u64)bi);
            __syncthreads();
            const long long win = s_tally.bad ? 0 : (long long)s_best;
            __syncthreads();                  // (s_tally is the tail's from here on)
            // ---- 8. apply the winning flip set
            if (win > 0) {
                u64 fm = 0ull;
                int tx = -1;
                osd_flip_set(method, kp, wp, win, &fm, &tx);
                const int kx = tx >= 0 ? tk[tx] : 0;
#pragma unroll
                for (int i = 0; i < RPT; ++i) {
                    if (pc[i] < 0) continue;
                    const int r = tid + i * nt;
                    unsigned d = (unsigned)__builtin_popcountll(cm[pc[i]] & fm) & 1u;
                    if (tx >= 0) d ^= (unsigned)(At[(size_t)(kx >> 6) * m + r] >> (kx & 63)) & 1u;
                    if (d) sol[pc[i]] ^= 1u;
                }
                if (tid < wp && ((fm >> tid) & 1ull)) sol[idx[tk[tid]]] ^= 1u;
                if (tid == 0 && tx >= 0) sol[idx[kx]] ^= 1u;
            }
        }
        // ---- 9. the record's tail, as osd0_blocked_kernel (a listed shot is the row-swapping kernel's record)
        if (tid == 0) s_tally = OsdTally{};
        __syncthreads();
        if (P.solution)
            for (int i = tid; i < n; i += nt) P.solution[rec * n + i] = sol[i];
        if (osd_counts_record(P, inconsistent)) osd_tail_block(P, rec, sol, syn, s_tally, tid, nt);   // (uniform)
        __syncthreads();
    }
}

#endif  // QBP_DEFINE_KERNELS

}  // namespace qbp
