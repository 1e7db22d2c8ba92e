// Pauli-frame simulation of CSS circuits (include/qbp.h: qbp_frame_*): frame_sim_kernel propagates 32 records per lane
// through the op table -- sampled shots or enumerated faults, one propagation body, two injectors -- and
// frame_assemble_kernel XORs measurement records into detectors and observables, transposed to b8 rows and masks.
// tests/circuit_oracle.py states the same rules in numpy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qbp_mc.hpp"

namespace qbp {

constexpr unsigned FRAME_PHILOX_WORD3 = 5u;   // QBP_FRAME_PHILOX_STREAM of include/qbp.h
constexpr int FRAME_MAX_CLASSES = 16;         // QBP_FRAME_MAX_CLASSES of include/qbp.h
constexpr int FRAME_THREADS = 256;            // frame_assemble_kernel
// frame_sim_kernel: one wavefront per workgroup.  A lane is 32 records, so 1e6 shots are 31 250 lanes -- 489 workgroups
// of 64 against 123 of 256 on 256 CUs.  Measured, the two give the same times (profiles/README.md, r34_circuit.json):
// the small lane count and each lane's chain of dependent frame accesses bound the kernel, not the spread over CUs.
constexpr int FRAME_SIM_THREADS = 64;

// op kinds: QBP_FRAME_* of include/qbp.h
enum { FRAME_RZ = 0, FRAME_RX = 1, FRAME_CX = 2, FRAME_MZ = 3, FRAME_MX = 4, FRAME_XERR = 5, FRAME_ZERR = 6,
       FRAME_DEP1 = 7, FRAME_DEP2 = 8 };

// One row of the device op table: x = kind, y = first qubit, z = second qubit (CX, DEP2), w = the record index of a
// measurement or the site index of a noise row.
// site_info[j] (padded with zeros to a multiple of four): bits 0-3 K, bits 4-5 the Pauli of a site with K == 1
// (XERR: 1, ZERR: 2), bits 8-15 the rate class.
struct FrameParams {
    const int4* ops;
    long long n_ops;
    const uint32_t* site_info;
    const long long* site_base;        // enumeration: the first fault of every site
    int nq, n_rec;
    long long W;                       // lanes of this chunk = row stride of frame and rec (a multiple of 64)
    uint32_t* frame;                   // [2 nq][W]: row 2q the X bits of qubit q, row 2q + 1 its Z bits
    uint32_t* rec;                     // [n_rec][W]
    unsigned long long begin;          // global index of the chunk's first record (a shot or a fault)
    unsigned long long seed;
    unsigned thr[FRAME_MAX_CLASSES];   // sampling: floor(rate[class] 2^32)
    // frame_assemble_kernel
    const int32_t* det_ptr; const int32_t* det_idx; int m;
    const int32_t* obs_ptr; const int32_t* obs_idx; int k;
    long long T;                       // records of this chunk
    uint8_t* det_bits;                 // [T][ceil(m / 8)] or null
    unsigned long long* obs;           // [T] or null
};

#ifdef QBP_FRAME_TU      // the kernels: qbp_tu_frame.hip only (qbp.hip needs FrameParams alone)

// (x0, z0, x1, z1) bit masks of one site over a lane's 32 records
struct FrameMasks { unsigned x0, z0, x1, z1; };

__device__ __forceinline__ void frame_add_fault(FrameMasks& M, unsigned info, unsigned code, unsigned bit)
{
    const unsigned pauli = (info & 15u) == 1u ? (info >> 4) & 3u : code;
    if (pauli & 1u) M.x0 |= bit;
    if (pauli & 2u) M.z0 |= bit;
    if (pauli & 4u) M.x1 |= bit;
    if (pauli & 8u) M.z1 |= bit;
}

// Sampling injector: the masks of sites 4g .. 4g + 3 for records t0 .. t0 + 31.  Site j of record t takes word j % 4
// of Philox4x32-10(counter (t lo, t hi, j / 4, FRAME_PHILOX_WORD3), key seed); it faults iff u < thr, with code
// 1 + (u K) / thr.
__device__ __forceinline__ void frame_sample_group(const FrameParams& P, unsigned g, unsigned long long t0, FrameMasks M[4])
{
    unsigned info[4], thr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        info[s] = P.site_info[4ull * g + s];
        thr[s] = (info[s] & 15u) ? P.thr[(info[s] >> 8) & (FRAME_MAX_CLASSES - 1)] : 0u;
        M[s] = FrameMasks{0u, 0u, 0u, 0u};
    }
    if ((thr[0] | thr[1] | thr[2] | thr[3]) == 0u) return;
#pragma unroll 2
    for (int b = 0; b < 32; ++b) {
        const unsigned long long t = t0 + (unsigned)b;
        unsigned c[4] = {(unsigned)t, (unsigned)(t >> 32), g, FRAME_PHILOX_WORD3};
        philox4x32_10(c, (unsigned)P.seed, (unsigned)(P.seed >> 32));
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (c[s] < thr[s]) {
                const unsigned code = 1u + (unsigned)(((unsigned long long)c[s] * (info[s] & 15u)) / thr[s]);
                frame_add_fault(M[s], info[s], code, 1u << b);
            }
    }
}

// Enumeration injector: record f is fault f, so site j flips the records base[j] .. base[j] + K - 1 that the lane owns.
__device__ __forceinline__ FrameMasks frame_enum_site(const FrameParams& P, unsigned j, unsigned long long f0)
{
    FrameMasks M{0u, 0u, 0u, 0u};
    const unsigned info = P.site_info[j];
    const unsigned long long base = (unsigned long long)P.site_base[j];
    const unsigned K = info & 15u;
    if (base + K <= f0 || base >= f0 + 32ull) return M;
    for (unsigned code = 1; code <= K; ++code) {
        const unsigned long long f = base + code - 1u;
        if (f >= f0 && f < f0 + 32ull) frame_add_fault(M, info, code, 1u << (unsigned)(f - f0));
    }
    return M;
}

// One lane per 32 records; a lane reads and writes only column `w` of frame and rec: no barrier, no atomic.  The op
// table is indexed uniformly, so its rows arrive through scalar loads.
template <bool SAMPLE>
__global__ __launch_bounds__(FRAME_SIM_THREADS) void frame_sim_kernel(const FrameParams P)
{
    const long long w = (long long)blockIdx.x * FRAME_SIM_THREADS + threadIdx.x;
    if (w >= P.W) return;
    uint32_t* __restrict__ F = P.frame + w;
    uint32_t* __restrict__ R = P.rec + w;
    const long long W = P.W;
    for (int r = 0; r < 2 * P.nq; ++r) F[(long long)r * W] = 0u;
    const unsigned long long t0 = P.begin + 32ull * (unsigned long long)w;
    FrameMasks G[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) G[s] = FrameMasks{0u, 0u, 0u, 0u};
    for (long long i = 0; i < P.n_ops; ++i) {
        const int4 op = P.ops[i];
        const long long xa = 2ll * op.y * W, za = xa + W;
        if (op.x == FRAME_CX) {
            const long long xb = 2ll * op.z * W, zb = xb + W;
            const uint32_t vxa = F[xa], vzb = F[zb];
            F[xb] ^= vxa;
            F[za] ^= vzb;
        } else if (op.x == FRAME_RZ || op.x == FRAME_RX) {
            F[xa] = 0u; F[za] = 0u;
        } else if (op.x == FRAME_MZ) {
            R[(long long)op.w * W] = F[xa];
        } else if (op.x == FRAME_MX) {
            R[(long long)op.w * W] = F[za];
        } else {
            const unsigned j = (unsigned)op.w;
            FrameMasks M;
            if (SAMPLE) {
                if ((j & 3u) == 0u) frame_sample_group(P, j >> 2, t0, G);
                M = G[0];
#pragma unroll
                for (int s = 1; s < 4; ++s)
                    if ((j & 3u) == (unsigned)s) M = G[s];
            } else {
                M = frame_enum_site(P, j, t0);
            }
            if (M.x0) F[xa] ^= M.x0;
            if (M.z0) F[za] ^= M.z0;
            if (op.x == FRAME_DEP2) {
                const long long xb = 2ll * op.z * W, zb = xb + W;
                if (M.x1) F[xb] ^= M.x1;
                if (M.z1) F[zb] ^= M.z1;
            }
        }
    }
}

// Records -> outputs.  Items [0, T rb): byte `i % rb` of the detector row of record i / rb (bit c % 8 of byte c / 8 is
// detector c; the padding bits of the last byte stay zero).  Items [T rb, T rb + T): the observable mask of a record.
__global__ __launch_bounds__(FRAME_THREADS) void frame_assemble_kernel(const FrameParams P)
{
    const long long rb = (P.m + 7) / 8;
    const long long n_det = P.det_bits ? P.T * rb : 0, n_obs = P.obs ? P.T : 0;
    const long long stride = (long long)gridDim.x * FRAME_THREADS;
    for (long long i = (long long)blockIdx.x * FRAME_THREADS + threadIdx.x; i < n_det + n_obs; i += stride) {
        if (i < n_det) {
            const long long t = i / rb;
            const int byte = (int)(i - t * rb);
            const uint32_t* __restrict__ R = P.rec + (t >> 5);
            const int sh = (int)(t & 31);
            unsigned out = 0;
            for (int c = 8 * byte; c < P.m && c < 8 * byte + 8; ++c) {
                uint32_t x = 0;
                for (int e = P.det_ptr[c]; e < P.det_ptr[c + 1]; ++e) x ^= R[(long long)P.det_idx[e] * P.W];
                out |= ((x >> sh) & 1u) << (c & 7);
            }
            P.det_bits[i] = (uint8_t)out;
        } else {
            const long long t = i - n_det;
            const uint32_t* __restrict__ R = P.rec + (t >> 5);
            const int sh = (int)(t & 31);
            unsigned long long mask = 0;
            for (int l = 0; l < P.k; ++l) {
                uint32_t x = 0;
                for (int e = P.obs_ptr[l]; e < P.obs_ptr[l + 1]; ++e) x ^= R[(long long)P.obs_idx[e] * P.W];
                mask |= (unsigned long long)((x >> sh) & 1u) << l;
            }
            P.obs[t] = mask;
        }
    }
}

#endif  // QBP_FRAME_TU

}  // namespace qbp
