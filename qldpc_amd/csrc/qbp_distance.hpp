// Distance upper bound by a randomized information-set search over ker H (QDistRnd's algorithm; Pryadko, Shabashov,
// Kozin 2022) on the GPU.  include/qbp.h (qbp_distance_search) states the rules; tests/distance_oracle.py is the same
// statement in numpy, and this kernel reproduces it bit for bit.
//
// One wavefront per trial, in the frame of osd0_kernel (qbp_osd.hpp) and with the pieces of qbp_osd_parts.hpp unchanged:
// the bitonic sort of (key, column) pairs (osd_sort), the bit-packed full-width rows in LDS in their original column
// indexing at row stride W + 1 words, lane l owning rows l, l + 64, ..., the lowest unused row with a 1 as the pivot of a
// column (osd_wave_find) and the XOR of the pivot row into every other row with the bit (osd_wave_eliminate).  What
// differs from a decoder's record: the sort keys are the 32-bit words of a Philox stream of the trial instead of |llr|
// (so the fill is this header's own, not osd_order_fill), the rows are those of a generator matrix G of ker H with
// no syndrome column (word W of every row is zero and stays zero; the pieces' syndrome bits are ignored), and the
// sweep ends as soon as every row is a pivot row.  The tail is the search's own: the lightest reduced row a row of L
// detects.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_osd_parts.hpp"

namespace qbp {

constexpr unsigned DIST_PHILOX_WORD3 = 4u;     // QBP_DISTANCE_PHILOX_STREAM of include/qbp.h
constexpr int DIST_MAX_ROWS = 64 * 32;         // the 32-bit row masks of osd_wave_find / osd_wave_eliminate
constexpr int DIST_MAX_COLS = 65535;           // 16-bit column indices in LDS
constexpr int DIST_TRIAL_BITS = 47;            // trials of one call: the call's best is one 64-bit word,
                                               // (weight << 47) | (trial - trial_begin), weight <= 65535

struct DistParams {
    int r, n, W, NP, k;             // rows of G, columns, 32-bit words per row, power of two >= n (sort width), rows of L
    const uint32_t* gbits;          // [r][W] bit-packed rows of G (bit v & 31 of word v >> 5)
    const uint32_t* lbits;          // [k][W] bit-packed rows of L
    unsigned long long seed;
    long long trial_begin;          // global index of item 0
    long long count;                // trials of this launch
    // search build
    unsigned long long* hist;       // [n + 1]: += 1 at the weight of every trial with a result
    unsigned long long* best;       // [1]: atomic min of (weight << DIST_TRIAL_BITS) | item over those trials
    // capture build (one trial, one workgroup)
    long long* found;               // [2]: the weight and the row index of the trial's result (-1, -1: none)
    uint8_t* codeword;              // [n]: that row as 0/1 bytes
    unsigned long long* logical_mask;   // [1]: bit l = parity(L[l] & row)
};

// LDS: osd0_kernel's region { u64 keys[NP] | uint32 A[r][W+1] } (the rows overwrite the keys after the sort), then
// uint16 idx[NP].
__host__ __device__ inline size_t dist_lds_bytes(int r, int W, int NP)
{
    return osd_region0_bytes(r, W, NP) + (size_t)NP * 2;
}

// parity(L[l] & row) over W words
__device__ __forceinline__ unsigned dist_parity(const uint32_t* row, const uint32_t* lrow, int W)
{
    uint32_t acc = 0;
    for (int w = 0; w < W; ++w) acc ^= row[w] & lrow[w];
    return (unsigned)__builtin_popcount(acc) & 1u;
}

// CAPTURE: the launch repeats one trial (count = 1, one workgroup) and stores its result row instead of counting it.
template <bool CAPTURE>
__global__ __launch_bounds__(64) void dist_search_kernel(const DistParams P)
{
    extern __shared__ unsigned long long dist_smem[];
    const int lane = threadIdx.x;
    const int r = P.r, n = P.n, W = P.W, NP = P.NP, k = P.k, RS = W + 1;
    char* const base0 = reinterpret_cast<char*>(dist_smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base0);
    uint32_t* A = reinterpret_cast<uint32_t*>(base0);                // (after the sort: same bytes)
    uint16_t* idx = reinterpret_cast<uint16_t*>(base0 + osd_region0_bytes(r, W, NP));

    for (long long item = blockIdx.x; item < P.count; item += gridDim.x) {
        const unsigned long long trial = (unsigned long long)(P.trial_begin + item);
        // ---- 1. column order: ascending (Philox word, column); the padding up to NP sorts behind every 32-bit key
        for (int g = lane; 4 * g < NP; g += 64) {
            unsigned c[4] = {(unsigned)trial, (unsigned)(trial >> 32), (unsigned)g, DIST_PHILOX_WORD3};
            philox4x32_10(c, (unsigned)P.seed, (unsigned)(P.seed >> 32));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = 4 * g + j;
                if (v < NP) {
                    keys[v] = v < n ? (unsigned long long)c[j] : ~0ull;
                    idx[v] = (uint16_t)v;
                }
            }
        }
        __syncthreads();
        osd_sort(keys, idx, NP, lane, 64);
        // ---- 2. A = [G | 0] (A overwrites the sort keys: every lane passed the sort's last barrier)
        for (int i = lane; i < r * W; i += 64) {
            const int row = i / W;
            A[row * RS + (i - row * W)] = P.gbits[i];
        }
        for (int row = lane; row < r; row += 64) A[row * RS + W] = 0u;
        __syncthreads();
        unsigned used = 0;                           // bit i: row lane + 64 i already serves as a pivot row
        unsigned sb = 0;                             // (the pieces' syndrome bits: word W is zero, so this stays zero)
        int left = r;                                // rows without a pivot
        for (int pos = 0; pos < n && left > 0; ++pos) {
            const int c = idx[pos];                  // (the n real columns sort before the padding)
            unsigned has;
            const int p = osd_wave_find(A, r, W, c, lane, used, has);
            if (p < 0) continue;                     // (uniform) no unused row has a 1 here: next column
            osd_wave_eliminate<0>(A, r, W, p, has, lane, used, sb);
            --left;
            __syncthreads();
        }
        // ---- 3, 4. the candidate of smallest (weight, row): a lane walks its rows in ascending order and asks L only
        // about a row lighter than what it holds
        unsigned long long mine = ~0ull;             // (weight << 32) | row
        for (int row = lane; row < r; row += 64) {
            const uint32_t* a = A + row * RS;
            int w = 0;
            for (int q = 0; q < W; ++q) w += __builtin_popcount(a[q]);
            const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (unsigned)row;
            if (w == 0 || key >= mine) continue;
            unsigned detected = 0;
            for (int l = 0; l < k && !detected; ++l) detected = dist_parity(a, P.lbits + (size_t)l * W, W);
            if (detected) mine = key;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(mine, off);
            mine = other < mine ? other : mine;
        }
        if constexpr (CAPTURE) {
            if (mine == ~0ull) {
                if (lane < 2) P.found[lane] = -1;
            } else {
                const int row = (int)(unsigned)mine;
                const uint32_t* a = A + row * RS;
                if (lane == 0) { P.found[0] = (long long)(mine >> 32); P.found[1] = row; }
                for (int v = lane; v < n; v += 64) P.codeword[v] = (uint8_t)((a[v >> 5] >> (v & 31)) & 1u);
                const unsigned long long lm = __ballot(lane < k && dist_parity(a, P.lbits + (size_t)lane * W, W));
                if (lane == 0) *P.logical_mask = lm;
            }
        } else {
            if (lane == 0 && mine != ~0ull) {
                const unsigned long long w = mine >> 32;
                atomicAdd(P.hist + w, 1ull);
                atomicMin(P.best, (w << DIST_TRIAL_BITS) | (unsigned long long)item);
            }
        }
        __syncthreads();                             // (the next trial's keys overwrite the rows)
    }
}

}  // namespace qbp
