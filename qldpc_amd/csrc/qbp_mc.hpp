// Monte-Carlo pieces shared by the kernels: the counter-based error sampler (this build's own
// specification, restated in oracle/bp_oracle.c:oracle_mc_errors) and the counter layout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef QBP_MC_COLS
// 1: the Monte-Carlo kernels draw with a threshold per qubit (thr_cols; qbp_mc_run_probs).  Set by the translation
// units compiled for that (qbp_tu_fused.hip / qbp_tu_generic.hip with -DQBP_COLS_TU), which give those kernels
// names of their own, so that the builds of the uniform sampler keep their code, registers and scratch.
#define QBP_MC_COLS 0
#endif

#ifndef QBP_MC_BUDGETS
// 1: the Monte-Carlo kernels checkpoint a running trial at a ladder of iteration budgets (qbp_mc_run_budgets):
// when a trial ends iteration budgets[j] - 1 unconverged it is emitted for counter row j and keeps iterating.
// Set, together with QBP_MC_COLS, by the translation units compiled for that (-DQBP_BUDGETS_TU), which give those
// kernels names of their own: the other builds keep their code, registers and scratch.
#define QBP_MC_BUDGETS 0
#endif

#ifndef QBP_MC_SPECTRUM
// 1: the Monte-Carlo kernels also add every classified trial's residual weight to a table spectrum[4][n + 1] and
// the iteration its syndrome was first satisfied in to iter_hist[max_iter + 1] (qbp_mc_run_spectrum).  Set,
// together with QBP_MC_COLS, by the translation units compiled for that (-DQBP_SPECTRUM_TU), which give those
// kernels names of their own: the other builds keep their code, registers, scratch and LDS.
#define QBP_MC_SPECTRUM 0
#endif

#ifndef QBP_MC_SHOTS
// 1: the Monte-Carlo kernels decode RECORDED shots (qbp_decode_shots): a trial's syndrome is read from a bit-packed
// row of detection events instead of being sampled, and what is emitted is the observable prediction Lx x of the
// decoder's output x, compared with the shot's recorded observables where those are given -- no error pattern, no
// residual.  Set by the translation units compiled for that (-DQBP_SHOTS_TU), which give those kernels names of their
// own: the other builds keep their code, registers, scratch and LDS.
#define QBP_MC_SHOTS 0
#endif

#ifndef QBP_MC_LLRHIST
// 1: the Monte-Carlo kernels also bin the posterior LLRs of every emission -- per iteration budget, by BP's converged
// flag and by the true value of the bit -- into a table the workgroup keeps in LDS (qbp_mc_run_llr_hist).  Set,
// together with QBP_MC_COLS and QBP_MC_BUDGETS, by the translation units compiled for that (-DQBP_LLRHIST_TU), which
// give those kernels names of their own: the other builds keep their code, registers, scratch and LDS.  These builds
// take stored errors too (errors_in), as the QBP_MC_SPECTRUM builds do.
#define QBP_MC_LLRHIST 0
#endif

namespace qbp {

constexpr int NUM_COUNTERS = 12;
constexpr int MAX_BUDGETS = 16;        // QBP_MC_MAX_BUDGETS of include/qbp.h
constexpr int SPECTRUM_ROWS = 4;       // QBP_SPECTRUM_ROWS of include/qbp.h
constexpr int LLR_HIST_ROWS = 4;       // QBP_LLR_HIST_ROWS of include/qbp.h: 2 * !converged + error bit

// Bytes of a workgroup's posterior-LLR table in LDS (QBP_MC_LLRHIST builds), 8-byte aligned: [bins + 1] edges and the
// bin estimate's scale as doubles, then [n_budgets][LLR_HIST_ROWS][bins + 3] 32-bit counts.
__host__ __device__ inline size_t llr_hist_lds_bytes(int n_budgets, int bins)
{
    return ((size_t)bins + 2) * 8 + (((size_t)n_budgets * LLR_HIST_ROWS * ((size_t)bins + 3) + 1) & ~(size_t)1) * 4;
}

// Row of spectrum[SPECTRUM_ROWS][n + 1] a trial with a non-zero residual goes to (rework/main.py:96-110): by BP's
// converged flag and by whether the residual is a logical operator -- never by whether OSD ran or was valid.
__host__ __device__ inline int mc_spectrum_row(bool found, bool logical)
{
    return (logical ? 2 : 0) + (found ? 0 : 1);
}

__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// Error bits of qubits 4g .. 4g+3 of trial `trial` as bytes (0/1) packed in a u32: one Philox
// evaluation per draw serves four qubits (specification: oracle/bp_oracle.c, oracle_mc_errors:
// counter = (trial lo, trial hi, qubit / 4, draw), word qubit % 4, bit = word < floor(p 2^32)).
__device__ __forceinline__ unsigned mc_error_quad(unsigned long long trial, int g, int draws,
                                                  unsigned long long seed, unsigned thr)
{
    unsigned bytes = 0;
    for (int d = 0; d < draws; ++d) {
        unsigned c[4] = {(unsigned)trial, (unsigned)(trial >> 32), (unsigned)g, (unsigned)d};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        bytes ^= (c[0] < thr ? 1u : 0u) | (c[1] < thr ? 0x100u : 0u) | (c[2] < thr ? 0x10000u : 0u) |
                 (c[3] < thr ? 0x1000000u : 0u);
    }
    return bytes;
}

// The same with a threshold per qubit (qbp_mc_run_probs: detector error models, where every column has its
// own probability): thr [n rounded up to 4] = floor(p_v 2^32), 16-byte aligned, zero in the padding; one
// 16-byte load per quad.  With every threshold equal this draws exactly the bytes of mc_error_quad.
__device__ __forceinline__ unsigned mc_error_quad_cols(unsigned long long trial, int g, int draws,
                                                       unsigned long long seed, const uint32_t* thr)
{
    const uint4 t = reinterpret_cast<const uint4*>(thr)[g];
    unsigned bytes = 0;
    for (int d = 0; d < draws; ++d) {
        unsigned c[4] = {(unsigned)trial, (unsigned)(trial >> 32), (unsigned)g, (unsigned)d};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        bytes ^= (c[0] < t.x ? 1u : 0u) | (c[1] < t.y ? 0x100u : 0u) | (c[2] < t.z ? 0x10000u : 0u) |
                 (c[3] < t.w ? 0x1000000u : 0u);
    }
    return bytes;
}

// The same four bytes from a stored error pattern instead (errors [n] 0/1 bytes of one trial): the Monte-Carlo
// kernels run on given errors when FusedParams / GenericParams::errors_in is set (qbp_mc_run_errors: the
// reference-pinned classification test feeds the reference's own trials through the device pipeline).
__device__ __forceinline__ unsigned mc_stored_quad(const uint8_t* errors, int g, int n)
{
    unsigned bytes = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (4 * g + i < n) bytes |= (unsigned)(errors[4 * g + i] & 1u) << (8 * i);
    return bytes;
}

// Detector c of shot t in stim's b8 layout: bit c % 8 of byte t * row_bytes + c / 8, row_bytes = ceil(m / 8).  Rows
// are not padded to words (m = 36: five bytes), so this is a byte load whatever the address.
__device__ __forceinline__ unsigned mc_shot_bit(const uint8_t* det_bits, long long t, int row_bytes, int c)
{
    return ((unsigned)det_bits[t * row_bytes + (c >> 3)] >> (c & 7)) & 1u;
}

// BP bookkeeping of one recorded shot into a counter row (qbp_decode_shots): shots, unconverged shots, iterations.
__device__ __forceinline__ void mc_count_shot(int* cnt, int conv, int it)
{
    cnt[0] += 1;
    if (!conv) cnt[6] += 1;
    cnt[7] += it;
}

// Classification of one finished trial (paperResults_GPU.py:127-144 without the OSD call) into a
// counter row: lm = logical mask of hard ^ error, ew = weight of the error, df = hard != error.
__device__ __forceinline__ void mc_count_trial(int* cnt, unsigned long long lm, int ew, int df, int conv,
                                               int it, int half_distance)
{
    const bool logical = lm != 0ull;                       // (Lx @ residual) % 2 has a 1
    cnt[0] += 1;
    if (conv && !logical && df) cnt[5] += 1;               // degenerateErrors  (:134-135)
    if (logical) {
        cnt[1] += 1;                                       // logical_error     (:137-138)
        if (ew < half_distance) cnt[3] += 1; else cnt[4] += 1;   // (:140-144)
        if (!conv) cnt[8] += 1;
    }
    if (!conv) cnt[6] += 1;
    cnt[7] += it;
    if (!df) cnt[9] += 1;
}

}  // namespace qbp
