// Sliding-window decoding (include/qbp.h, qbp_window_*): the device-side glue between the windows of one call.
// The BP and OSD kernels of the sub-handles are launched unchanged; these kernels move a window's syndrome rows in,
// list the records its BP left unconverged for the OSD launch, commit its first rounds and fold the committed
// correction into the running syndrome -- so that nothing returns to the host between two windows.
// All of them are memory-bound byte movers: grid-stride loops of WINDOW_THREADS lanes over 64-bit item indices,
// consecutive lanes on consecutive bytes of one record's row, and no lane writes a byte another lane of the same
// launch reads.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_mc.hpp"

namespace qbp {

constexpr int WINDOW_THREADS = 256;
constexpr int WINDOW_MAX_GRID = 2048;     // blocks of a launch; the loops stride over the rest

// Rules 3-5 of a window (include/qbp.h).  Per record there are n_upd + n_commit + 1 items:
//   item t < n_upd: check upd_check[t] of H has entries in the commit set M_k -- upd_local[upd_ptr[t] .. upd_ptr[t + 1])
//     are their positions in U_k.  The lane XORs the committed bits into r[b][check]; it is the only lane of the
//     launch that touches that byte (no atomics);
//   the next n_commit items: committed variable commit_var[t], position commit_local[t] in U_k: x and llr_out;
//   the last item: iters += it, window_fails += !conv.
// The committed bit of a record is the OSD solution where BP did not converge and OSD ran (sol != null), else BP's.
struct WindowCommit {
    long long B;
    int m, n, nk;
    const uint8_t* hard;        // [B][nk] the sub-handle's outputs; null: a skipped window, llr is then its prior [nk]
    const uint8_t* sol;         // [B][nk] rows of the unconverged records, or null (no OSD)
    const uint8_t* conv;        // [B]
    const int32_t* it;          // [B]
    const double* llr;          // [B][nk]
    int n_upd, n_commit;
    const int32_t* upd_check;   // [n_upd]
    const int32_t* upd_ptr;     // [n_upd + 1]
    const int32_t* upd_local;
    const int32_t* commit_local;// [n_commit]
    const int32_t* commit_var;  // [n_commit]
    uint8_t* r;                 // [B][m] the running syndrome
    uint8_t* x;                 // [B][n] or null
    double* llr_out;            // [B][n] or null
    int32_t* iters;             // [B] or null
    int32_t* fails;             // [B] or null
    uint8_t* converged;         // [B] or null (FINAL launches only)
};

// The kernels themselves: in qbp_tu_window.hip only (the API unit sees the parameter struct above).
#ifdef QBP_WINDOW_TU

// Window k's syndrome rows: syn [B][mk] = r [B][m] at the checks C_k (ascending).
__global__ __launch_bounds__(WINDOW_THREADS) void window_gather_kernel(const uint8_t* __restrict__ r, long long B, int m,
                                                                        const int32_t* __restrict__ checks, int mk,
                                                                        uint8_t* __restrict__ syn)
{
    const long long total = B * (long long)mk, step = (long long)gridDim.x * WINDOW_THREADS;
    for (long long i = (long long)blockIdx.x * WINDOW_THREADS + threadIdx.x; i < total; i += step) {
        const long long b = i / mk;
        const int j = (int)(i - b * mk);
        syn[i] = r[b * m + checks[j]] & 1u;
    }
}

// The priors of every window at once: out [sum of n_k] = prior at the concatenated variable lists U_0, U_1, ...
__global__ __launch_bounds__(WINDOW_THREADS) void window_gather_prior_kernel(const double* __restrict__ prior,
                                                                              const int32_t* __restrict__ vars, int total,
                                                                              double* __restrict__ out)
{
    const int step = (int)gridDim.x * WINDOW_THREADS;
    for (int i = (int)blockIdx.x * WINDOW_THREADS + threadIdx.x; i < total; i += step) out[i] = prior[vars[i]];
}

// The records BP left unconverged, for OsdParams::list / count_ptr.  *count is zero before the launch.  The order of
// the list depends on the order the lanes arrive in; OSD treats every record on its own, so no output does.
__global__ __launch_bounds__(WINDOW_THREADS) void window_fail_list_kernel(const uint8_t* __restrict__ conv, long long B,
                                                                           long long* __restrict__ list,
                                                                           unsigned long long* __restrict__ count)
{
    const long long step = (long long)gridDim.x * WINDOW_THREADS;
    for (long long b = (long long)blockIdx.x * WINDOW_THREADS + threadIdx.x; b < B; b += step)
        if (!conv[b]) list[atomicAdd(count, 1ull)] = b;
}

// FINAL: the launch after the last window's commit -- converged[b] = (r[b] == 0 in bit 0, the only bit of a syndrome
// byte that counts), one wavefront per record.
template <bool FINAL>
__global__ __launch_bounds__(WINDOW_THREADS) void window_commit_kernel(WindowCommit P)
{
    if (FINAL) {
        const int lane = threadIdx.x & 63;
        const long long waves = (long long)gridDim.x * (WINDOW_THREADS / 64);
        for (long long b = (long long)blockIdx.x * (WINDOW_THREADS / 64) + (threadIdx.x >> 6); b < P.B; b += waves) {
            const uint8_t* row = P.r + b * P.m;
            unsigned any = 0;
            for (int c = lane; c < P.m; c += 64) any |= row[c] & 1u;
            const bool left = __ballot(any != 0u) != 0ull;
            if (lane == 0) P.converged[b] = left ? 0 : 1;
        }
        return;
    }
    const long long per = (long long)P.n_upd + P.n_commit + 1;
    const long long total = P.B * per, step = (long long)gridDim.x * WINDOW_THREADS;
    for (long long i = (long long)blockIdx.x * WINDOW_THREADS + threadIdx.x; i < total; i += step) {
        const long long b = i / per;
        int t = (int)(i - b * per);
        if (!P.hard) {      // a skipped window (no check or no variable): 0 and the prior for its variables, nothing else
            if (t < P.n_commit) {
                const long long at = b * P.n + P.commit_var[t];
                if (P.x) P.x[at] = 0;
                if (P.llr_out) P.llr_out[at] = P.llr[P.commit_local[t]];
            }
            continue;
        }
        const int cv = P.conv[b];
        const uint8_t* bits = (P.sol && !cv ? P.sol : P.hard) + b * P.nk;
        if (t < P.n_upd) {
            unsigned acc = 0;
            for (int e = P.upd_ptr[t]; e < P.upd_ptr[t + 1]; ++e) acc ^= bits[P.upd_local[e]];
            uint8_t* cell = P.r + b * P.m + P.upd_check[t];
            *cell = (uint8_t)((*cell ^ acc) & 1u);
            continue;
        }
        t -= P.n_upd;
        if (t < P.n_commit) {
            const int j = P.commit_local[t];
            const long long at = b * P.n + P.commit_var[t];
            if (P.x) P.x[at] = bits[j] & 1u;
            if (P.llr_out) P.llr_out[at] = P.llr[b * P.nk + j];
            continue;
        }
        if (P.iters) P.iters[b] += P.it[b];
        if (P.fails) P.fails[b] += cv ? 0 : 1;
    }
}

// syndromes [T][m] = H errors [T][n], bytes in and bytes out: one lane per (trial, check).
__global__ __launch_bounds__(WINDOW_THREADS) void window_syndrome_kernel(const uint8_t* __restrict__ errors, long long T,
                                                                          int m, int n, const int32_t* __restrict__ row_ptr,
                                                                          const int32_t* __restrict__ col_idx,
                                                                          uint8_t* __restrict__ syn)
{
    const long long total = T * (long long)m, step = (long long)gridDim.x * WINDOW_THREADS;
    for (long long i = (long long)blockIdx.x * WINDOW_THREADS + threadIdx.x; i < total; i += step) {
        const long long t = i / m;
        const int c = (int)(i - t * m);
        const uint8_t* e = errors + t * n;
        unsigned acc = 0;
        for (int k = row_ptr[c]; k < row_ptr[c + 1]; ++k) acc ^= e[col_idx[k]];
        syn[i] = (uint8_t)(acc & 1u);
    }
}

// Classification of T decoded trials (paperResults_GPU.py:127-144 as mc_count_trial states it), one wavefront per
// trial: `conv` of that rule is window_fails == 0 (every window's BP converged, which implies a valid correction);
// a correction OSD made valid counts as valid for degenerateErrors, as oracle.classify_trials checks H x == s itself;
// [10] counts the corrections that miss the syndrome.  Counters are summed per workgroup in LDS, then added to the
// global row with one atomic per counter and workgroup.
__global__ __launch_bounds__(WINDOW_THREADS) void window_classify_kernel(const uint8_t* __restrict__ errors,
                                                                          const uint8_t* __restrict__ x,
                                                                          const uint8_t* __restrict__ valid,
                                                                          const int32_t* __restrict__ iters,
                                                                          const int32_t* __restrict__ fails, long long T, int n,
                                                                          const unsigned long long* __restrict__ lx_cols,
                                                                          int half_distance, long long* __restrict__ counters)
{
    __shared__ unsigned long long block_cnt[NUM_COUNTERS];
    if (threadIdx.x < NUM_COUNTERS) block_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (WINDOW_THREADS / 64);
    for (long long t = (long long)blockIdx.x * (WINDOW_THREADS / 64) + (threadIdx.x >> 6); t < T; t += waves) {
        const uint8_t* e = errors + t * n;
        const uint8_t* d = x + t * n;
        unsigned long long lm = 0ull;
        int ew = 0, df = 0;
        for (int v = lane; v < n; v += 64) {
            const unsigned eb = e[v] & 1u, res = (d[v] ^ eb) & 1u;
            ew += (int)eb;
            df |= (int)res;
            if (res) lm ^= lx_cols[v];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lm ^= __shfl_xor(lm, o, 64);
            ew += __shfl_xor(ew, o, 64);
            df |= __shfl_xor(df, o, 64);
        }
        if (lane == 0) {
            int cnt[NUM_COUNTERS];
#pragma unroll
            for (int i = 0; i < NUM_COUNTERS; ++i) cnt[i] = 0;
            const int conv = fails[t] == 0, ok = valid[t] != 0;
            mc_count_trial(cnt, lm, ew, df, conv, iters[t], half_distance);
            if (!conv && ok && lm == 0ull && df) cnt[5] += 1;
            if (!ok) cnt[10] += 1;
#pragma unroll
            for (int i = 0; i < NUM_COUNTERS; ++i)
                if (cnt[i]) atomicAdd(&block_cnt[i], (unsigned long long)cnt[i]);
        }
    }
    __syncthreads();
    if (threadIdx.x < NUM_COUNTERS && block_cnt[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(counters) + threadIdx.x, block_cnt[threadIdx.x]);
}

#endif  // QBP_WINDOW_TU

}  // namespace qbp
