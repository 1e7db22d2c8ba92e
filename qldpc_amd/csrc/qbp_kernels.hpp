// Fused on-chip belief-propagation kernel for gfx950 (MI355X).
//
// One lane per CHECK node.  A workgroup decodes S syndromes concurrently ("slots"); slot s owns
// lanes [s*m, (s+1)*m).  A lane keeps its check's d_c variable->check messages Q in registers
// for the whole decode; the only data exchanged between lanes are the check->variable messages
// R, one double per edge, staged in LDS, variable-major: [slot][variable v][k], k the position of the
// check in v's column (ascending check order), so the DV messages of a variable are one contiguous
// record and a lane needs one gather address and one store address per edge.  Per BP iteration a lane
//   1. check step:   t_j = tanh(Q_j/2); row product; R_j = 2 atanh(clip(prod / t_j * sign))
//                    -> ds_write R_j                          (beliefPropagation.py:114-126)
//   2. barrier
//   3. variable step, done redundantly by every check lane for its own d_c variables: reads the
//      <= DV messages of each variable's column from LDS (ascending check order, the order
//      np.sum(R, axis=0) accumulates in), value_j = sum + prior_j, Q_j = value_j - R_j, hard
//      bit, parity of the row vs the syndrome bit -> per-slot "unsatisfied" flag (:129-139)
//   4. barrier, read the flag: converged / iteration limit -> emit outputs, fetch next syndrome.
//      (QBP_FLAG_FORCE_FULL launches of the (6, 3) shape skip this barrier: two copies of R, the flag
//      read one phase later -- see ONE_BAR in the kernel.)
// No message ever touches HBM: per syndrome the kernel reads m syndrome bytes and writes
// n hard bytes + n LLR doubles + 5 bytes.  Slots fetch work from a global atomic counter, so a
// slot whose syndrome converges early (reference semantics: return at the first syndrome match)
// immediately starts the next one, independent of its neighbours.
//
// Irregular rows/columns are padded: a missing edge has prior = +inf (its Q stays +inf, its tanh
// is exactly 1.0, its hard bit 0) and gathers from an all-zero record behind the last slot; the words
// a column with fewer than DV checks leaves free in its record hold 0.0 (x + 0.0 is exact) -- the
// kernel body has no degree-dependent branches.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qbp_check.hpp"
#include "qbp_hist_bin.hpp"
#include "qbp_mc.hpp"

// Register-budget choices of the shapes that do not fit 128 registers otherwise (A/B switches for
// tools/build_variants.sh; the defaults are the measured-best settings, profiles/r02_ab_wide_mc.txt)
#ifndef QBP_WIDE_JG
#define QBP_WIDE_JG 4          // (8, 4) shape: edges per LDS gather group
#endif
#ifndef QBP_WIDE_HOLD_R
#define QBP_WIDE_HOLD_R 1      // (8, 4) shape: own messages in registers across barrier B1
#endif
#ifndef QBP_WIDE_PACK
#define QBP_WIDE_PACK 0        // (8, 4) shape: two LDS offsets per register
#endif
#ifndef QBP_SMALL_HOLD_R
#define QBP_SMALL_HOLD_R 1     // (6, 3) decode builds: as above
#endif
#ifndef QBP_SMALL_PACK
#define QBP_SMALL_PACK 0
#endif
#ifndef QBP_MC_HOLD_R
#define QBP_MC_HOLD_R 0        // Monte-Carlo builds: as above
#endif
#ifndef QBP_MC_PACK
#define QBP_MC_PACK 0
#endif
#ifndef QBP_WORK_CHUNK_SMALL_CODES
#define QBP_WORK_CHUNK_SMALL_CODES 1   // 0: at most eight syndromes per fetch whatever the code size (A/B)
#endif
#ifndef QBP_WORK_CHUNK_FIXED
#define QBP_WORK_CHUNK_FIXED 0    // 1: eight syndromes per fetch from the work counter, always (A/B)
#endif

namespace qbp {

// Forced-iteration launches with ONE workgroup barrier per iteration keep two copies of the
// check->variable messages in LDS; the second copy sits at this constant byte distance from the first
// (a constant, so that the toggle costs nothing: it lands in the offset field of the ds instructions of a
// loop unrolled by two).  The first copy, fused_r_doubles() doubles, must fit below it.
constexpr int FUSED_R2_OFF_BYTES = 57344;

// One copy of R in LDS:
//   [S][slot_stride]  the slots' records, laid out by the host (build_tables);
//   [DV]              one all-zero record, which every padding edge gathers;
//   [1]               one dump word, which every padding edge stores to and nobody reads.
// A record is the DV consecutive words an edge gathers for its variable: the messages of the variable's column,
// adjacent and in summation order, and zeros in the words left over.
// INVARIANT: the message words of different records are disjoint; their zero words need not be.  A column with
// fewer than DV checks may have its zeros in front of its messages (a zero adds nothing wherever it stands in the
// left-to-right sum), and then shares them with the trailing zeros of the record before.  Zero words are written
// once per launch and by no edge.
// Why no 16-byte-aligned records for ds_read_b128: DV = 3 records padded to 32 bytes do not fit twice below
// FUSED_R2_OFF_BYTES for [[288,12,18]]; DV = 4 records of 32 bytes put the 864 x 2592 space-time matrix of
// [[144,12,12]] (column weights 3 and 2) past 160 KiB.
// The tables address the zero record and the dump word relative to the slot, as slot_stride and slot_stride + DV;
// the kernel moves those two behind the last slot ("per-lane static tables").
constexpr size_t fused_r_doubles(int slot_stride, int dv, int S) { return (size_t)S * (size_t)slot_stride + dv + 1; }

struct FusedParams {
    // problem
    const uint8_t* syndromes;   // [B][m] (decode mode)
    const double* prior;        // [n]
    long long B;                // syndromes / trials in this launch
    int m, n;
    int S;                      // slots per workgroup
    int slot_stride;            // doubles per slot in LDS (the records of the variables)
    int max_iter;
    unsigned flags;
    int padded;                 // some row has fewer than DC edges (irregular H)
    int n_words4;               // ceil(n / 4)
    int r0_table;               // LDS holds the first check step's messages (early-exit launches, when it fits)
    double alpha, damping, clip_llr;
    // outputs (decode mode; may be null)
    uint8_t* hard;
    uint8_t* converged;
    int32_t* iters;
    double* llr;
    // static tables of the code
    const int32_t* tab_var;     // [DC][m]   variable of edge j of check c, -1 = padding
    const uint16_t* tab_gather; // [DC][m]   slot-relative word offset of the record of that variable (padding: slot_stride)
    const uint16_t* tab_store;  // [DC][m]   ... of this edge's own word in it (padding: slot_stride + DV)
    const uint32_t* tab_writer; // [m] bit j: edge (c, j) is the first of its column
    const int32_t* iso_vars;    // variables with no check
    int n_iso;
    // work distribution
    unsigned long long* work_counter;   // zeroed before launch
    // Monte-Carlo mode
    const unsigned long long* lx_cols;  // [n] bit l = Lx[l][v]
    long long trial_begin;
    unsigned long long seed;
    unsigned threshold;         // floor(p * 2^32)
    int draws;
    int half_distance;          // distance // 2
    long long* counters;        // [NUM_COUNTERS], atomically added
    const uint8_t* errors_in;   // optional [B][n]: decode and classify THESE errors instead of sampling
    // Monte-Carlo + OSD: records of the trials BP did not converge on (indexed by the trial's
    // position b in this launch), and the list of those positions
    long long* fail_list;       // null = classify BP output directly
    unsigned long long* fail_count;
    uint8_t* fail_syn;          // [B][m]
    double* fail_llr;           // [B][n]
    uint8_t* fail_hard;         // [B][n]
    uint8_t* fail_err;          // [B][n]
    // (last, so that adding it moved no field the other builds read)
    const uint32_t* thr_cols;   // [n4 * 4] a threshold per qubit (QBP_MC_COLS builds: qbp_mc_run_probs)
    // QBP_MC_BUDGETS builds (qbp_mc_run_budgets): ascending iteration budgets, max_iter = the last one.  counters is
    // [n_budgets][NUM_COUNTERS] then; the failure records and lists are per (row j, trial b): record j * B + b,
    // list j at fail_list + j * B, its length at fail_count[j].
    int n_budgets;
    int budgets[MAX_BUDGETS];
    // QBP_MC_SPECTRUM builds (qbp_mc_run_spectrum): spectrum [SPECTRUM_ROWS][n + 1], the residual weights of the
    // classified trials by row (mc_spectrum_row), and iter_hist [max_iter + 1] (may be null), the iteration a trial's
    // syndrome was first satisfied in (bin max_iter: never); both atomically added to
    long long* spectrum;
    long long* iter_hist;
    // QBP_MC_SHOTS builds (qbp_decode_shots): det_bits [B][det_row_bytes], the recorded detection events bit-packed
    // (mc_shot_bit); actual [B] (may be null), the recorded observables, bit l = observable l; predictions [B] (may be
    // null), Lx x of the decoder's output x in the same encoding.  `converged` above (may be null) is written too.
    const uint8_t* det_bits;
    int det_row_bytes;
    const unsigned long long* actual;
    unsigned long long* predictions;
    // QBP_MC_LLRHIST builds (qbp_mc_run_llr_hist; budgets as above): llr_hist [n_budgets][LLR_HIST_ROWS][llr_bins + 3],
    // atomically added to; llr_edges [llr_bins + 1], np.linspace(lo, hi, llr_bins + 1) from the host
    long long* llr_hist;
    const double* llr_edges;
    int llr_bins;
};

// Rarely used launch parameters (output pointers, Monte-Carlo settings, ...) are re-read from the
// kernel-argument segment where they are needed instead of being kept in SGPRs for the whole
// kernel: the hot loop already needs ~60 SGPRs for FP64 constants, and every SGPR the compiler
// has to spill costs v_readlane/v_writelane slots on the (saturated) vector ALU.  The empty asm
// makes the pointer opaque so that the loads cannot be hoisted out of the cold branches.
typedef const FusedParams __attribute__((address_space(4)))* ColdArgs;
__device__ __forceinline__ ColdArgs cold_args()
{
    ColdArgs p = (ColdArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
#define COLD(field) (cold_args()->field)

// Syndromes a slot leader fetches at once when its syndromes have taken avg4 / 4 iterations on average
// (see "Work distribution" in the kernel).
__device__ __forceinline__ int work_chunk_for(int avg4)
{
    return avg4 < 12 ? 8 : avg4 < 28 ? 4 : avg4 < 60 ? 2 : 1;
}

// Classification of one finished trial by its slot leader (paperResults_GPU.py:127-144 without
// the OSD call): reads and clears the slot's accumulators, bumps the slot's counter row in LDS.
__device__ __forceinline__ void mc_classify(unsigned long long* mc_lmask, int* mc_weight,
                                            int* mc_diff, int* cnt, int slot, int conv, int it,
                                            int half_distance, bool deferred)
{
    if (deferred) {            // handed to OSD: only the BP bookkeeping is counted here
        cnt[0] += 1; cnt[6] += 1; cnt[7] += it;
        return;
    }
    const unsigned long long lm = mc_lmask[slot];
    const int ew = mc_weight[slot];
    const int df = mc_diff[slot];
    mc_lmask[slot] = 0ull; mc_weight[slot] = 0; mc_diff[slot] = 0;
    mc_count_trial(cnt, lm, ew, df, conv, it, half_distance);
}

// LDS carve (in units of 8 bytes after the message area):
//   [DC][m] priors of the edges' variables (+inf for padding edges)
//   [S]  next work index per slot
//   [S]  end of the chunk of work indices the slot is drawing from (leader only)
//   [S]  MC logical-mask accumulator
//   then 32-bit words: flag[2][S], mc_weight[S], mc_diff[S], active_count,
//   mc_count[S][NUM_COUNTERS] (Monte-Carlo mode only; [S][2][n_budgets][NUM_COUNTERS] in the QBP_MC_BUDGETS builds),
//   var_lds[DC][m], err_lds[2][S][n4] bytes (MC),
//   then 32-bit words again in the QBP_MC_SPECTRUM builds: mc_resw[S] (residual weight accumulator of the slot),
//   it_hist[max_iter + 1] (the workgroup's iteration histogram)
//   or, in the QBP_MC_LLRHIST builds, from the next 8-byte boundary: the workgroup's posterior-LLR table
//   (llr_hist_lds_bytes: edges and scale as doubles, then the counts)
template <int DC, int DV, int VARIANT, bool MC, bool FORCE_FULL, int MAX_THREADS, int MIN_WAVES_PER_SIMD,
          bool ONE_BARRIER = false>
__global__ __launch_bounds__(MAX_THREADS, MIN_WAVES_PER_SIMD) void bp_fused_kernel(const FusedParams P)
{
    // ONE_BAR (forced-iteration decode launches only): one workgroup barrier per iteration instead of two.
    // The second barrier of an iteration orders (a) the next check step's writes of R after this variable
    // step's reads and (b) the slot's convergence flag before its readers.  (a) goes away with two copies
    // of R used alternately; (b) is deferred: whether iteration k satisfied the syndrome is looked at after
    // the barrier of iteration k + 1 -- the posterior values of iteration k are still in registers then --
    // which is only affordable when nothing is decided by it but WHEN the outputs are written: in forced
    // mode every syndrome runs max_iter iterations anyway (and all slots switch syndromes in the same
    // phase, so the last iteration, which must settle before the registers are reused, keeps its second
    // barrier for the whole workgroup).  With early exit the next check step would be wasted work.
    constexpr bool ONE_BAR = ONE_BARRIER && FORCE_FULL && !MC;
    // BUDGETS (qbp_mc_run_budgets; the -DQBP_BUDGETS_TU builds only): a trial that ends iteration budgets[j] - 1
    // unconverged is emitted for counter row j -- what a run with max_iter = budgets[j] reports -- and keeps
    // iterating.  A slot then has 2 * n_budgets counter rows instead of one: "exactly row j" (checkpoints, and
    // the last budget) and "from row j upwards" (a trial that converged in iteration k, entered at the first j
    // with budgets[j] > k); row j of the result = exact[j] + sum of from[0 .. j], formed once per workgroup.
    constexpr bool BUDGETS = MC && QBP_MC_BUDGETS != 0;
    // SPECTRUM (qbp_mc_run_spectrum; the -DQBP_SPECTRUM_TU builds only): a classified trial's residual weight goes to
    // the global table spectrum[row][w] (w > 0 only: rare at the error rates of interest, so straight to global
    // memory with a 64-bit atomic), every trial's iteration index to the workgroup's histogram in LDS (one LDS atomic
    // per trial by its slot leader; one global atomic per non-zero bin when the workgroup ends).
    constexpr bool SPECTRUM = MC && QBP_MC_SPECTRUM != 0;
    // SHOTS (qbp_decode_shots; the -DQBP_SHOTS_TU builds only): a trial is a recorded shot.  Its check lanes read their
    // syndrome bits from the shot's bit row (no sampler, hence no error bytes in LDS and no barrier B0); the emission
    // forms the parity of lx_cols over the support of the hard decision -- the observable prediction -- which the slot
    // leader stores, with the converged flag, and compares with the recorded observables.
    constexpr bool SHOTS = MC && QBP_MC_SHOTS != 0;
    // LLRHIST (qbp_mc_run_llr_hist; the -DQBP_LLRHIST_TU builds only, which are BUDGETS builds): every emission -- a
    // checkpoint, the last budget or the trial's convergence, classified here or left to OSD -- bins the posterior
    // value of each of the trial's n variables into the workgroup's table in LDS, plane bj, row 2 * !conv + error bit.
    // The unconverged rows are exact per budget; a converged trial is binned once, in the plane of the budget it
    // converged in, and counts for every later one: the prefix sum is formed when the workgroup ends, with the
    // counters'.  Counts are 32 bits: the host keeps n * (trials of a launch) below 2^32.
    constexpr bool LLRHIST = MC && QBP_MC_LLRHIST != 0;
    static_assert(!LLRHIST || BUDGETS, "the LLR histogram builds are budgets builds");
    // dynamic LDS: the tables of the two elementary functions (qbp_math.hpp, NpImage) first -- a constant
    // address, so that a table access is a row offset plus an immediate -- then the carve described above
    extern __shared__ __attribute__((aligned(16))) double smem_all[];
    constexpr NpT np_tab = 0u;          // = the LDS address of smem_all: this kernel has no static LDS (checked below)
    double* const smem = smem_all + NP_LDS_DOUBLES;
    const int tid = threadIdx.x;
    const int m = P.m;
    const int S = P.S;
    const int slot = tid / m;
    const int c = tid - slot * m;
    const bool lane_valid = slot < S;
    const bool leader = lane_valid && c == 0;
    const int sl = lane_valid ? slot : 0;

    const int stride = P.slot_stride;
    const int r_doubles = S * stride + DV + 1;      // one copy of R (fused_r_doubles)
    // priors of this check's variables, [edge j][check c], shared by all slots (an LDS read per
    // use instead of 12 VGPRs per lane for the whole kernel)
    double* const pri_lds = smem + (ONE_BAR ? FUSED_R2_OFF_BYTES / 8 : 0) + r_doubles;
    // Early-exit launches: the check->variable messages of a syndrome's FIRST check step, which depend
    // on nothing but the priors and the check's syndrome bit -- r0_lds[bit][edge j][check c], computed once
    // per workgroup by the kernel's own check-step code (same bits).  At low error rates most syndromes
    // need one or two iterations, and the first check step is most of the first one.
    const bool use_r0 = !FORCE_FULL && P.r0_table != 0;
    double* const r0_lds = pri_lds + DC * m;
    long long* const next_work = reinterpret_cast<long long*>(r0_lds + (use_r0 ? 2 * DC * m : 0));
    // (the variable indices of the edges, needed only when a syndrome is emitted, sit behind the
    // 32-bit words below: var_lds[DC][m])
    long long* const chunk_ends = next_work + S;     // (LDS, not a register: touched once per syndrome)
    unsigned long long* const mc_lmask = reinterpret_cast<unsigned long long*>(chunk_ends + S);
    int* const words = reinterpret_cast<int*>(mc_lmask + S);
    int* const flag0 = words;            // [3][S] (two in use, three with ONE_BAR)
    int* const mc_weight = words + 3 * S;
    int* const mc_diff = words + 4 * S;
    int* const work_avg = words + 5 * S;     // [0]: 4 x running mean of the workgroup's iterations per syndrome ([S] reserved)
    int* const active_count = words + 6 * S;
    // counter ints per slot: one row, or (BUDGETS) [2][n_budgets] rows, "exactly row j" then "from row j upwards"
    int slot_counters = NUM_COUNTERS;
    if constexpr (BUDGETS) slot_counters = 2 * COLD(n_budgets) * NUM_COUNTERS;
    int* const mc_count = words + 6 * S + 1 + sl * slot_counters;  // this slot's row(s)
    int* const var_lds = words + 6 * S + 1 + S * slot_counters;    // [DC][m], -1 = padding
    // Monte-Carlo mode: sampled error bytes of the slot's trials, [2][S][n4] (n4 = n rounded up to a
    // multiple of 4), written by the slot's first ceil(n/4) lanes one barrier before use.  Two
    // buffers per slot, used alternately by consecutive trials: the emission of a finished trial still
    // reads the bytes of its isolated variables after barrier B2, while faster waves of the same slot
    // may already be sampling the next trial at the top of the loop (no barrier in between).
    unsigned err_par = 0;                         // buffer of the trial being decoded (uniform per slot)
    // (recomputed where it is used -- all of them once-per-trial places -- instead of being held in
    // registers across the hot loop)
    auto err_buf = [&]() -> unsigned char* {
        const int n4 = COLD(n_words4) * 4;
        return reinterpret_cast<unsigned char*>(var_lds + DC * m) + (size_t)(sl + (err_par ? S : 0)) * n4;
    };

    // SPECTRUM: mc_resw[S] then it_hist[max_iter + 1], behind the error bytes (recomputed where used, as err_buf)
    auto spec_words = [&]() -> int* {
        return var_lds + DC * m + 2 * S * COLD(n_words4);
    };

    // LLRHIST: [llr_bins + 1] edges and the scale, then the counts [n_budgets][LLR_HIST_ROWS][llr_bins + 3], behind
    // the error bytes on an 8-byte boundary (recomputed where used, as err_buf)
    auto llr_edges_lds = [&]() -> double* {
        return reinterpret_cast<double*>(
            (reinterpret_cast<uintptr_t>(var_lds + DC * m + 2 * S * COLD(n_words4)) + 7) & ~(uintptr_t)7);
    };

    // ---- check step of one row: q[DC] -> put(j, r) for its DC edges (qbp_check.hpp) -----------------
    auto check_step = [&](const double (&q)[DC], unsigned sb, auto&& put) {
        check_row<VARIANT, DC, (DC > 6)>(q, sb, P.alpha, true, np_tab, put);
    };

    // ---- per-lane static tables (registers for the whole kernel) ---------------------------
    // Per edge, the word offsets (in a copy of R) of the record of its variable and of the edge's own word in
    // that record: one register each, or (PACK_NBR) both as 16-bit halves of one register -- half the registers,
    // one extra shift/mask per use.  A padding edge, whose table entries lie past the slot's records, gets the
    // workgroup's zero record and dump word behind the last slot.
    constexpr bool PACK_NBR = (DC > 6 && QBP_WIDE_PACK != 0) || (MC && QBP_MC_PACK != 0) ||
                              (DC <= 6 && !MC && QBP_SMALL_PACK != 0);
    unsigned gat[DC];              // (PACK_NBR: gather | store << 16)
    unsigned sto[PACK_NBR ? 1 : DC];
    unsigned wmask = 0;
    unsigned vmask = 0;            // bit j: edge j of this check exists (not padding)
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        const int v = lane_valid ? P.tab_var[j * m + c] : -1;
        vmask |= (v >= 0 ? 1u : 0u) << j;
        if (slot == 0) {
            pri_lds[j * m + c] = v >= 0 ? P.prior[v] : __builtin_inf();
            var_lds[j * m + c] = v;
        }
        unsigned og = lane_valid ? P.tab_gather[j * m + c] : (unsigned)stride;
        unsigned os = lane_valid ? P.tab_store[j * m + c] : (unsigned)(stride + DV);
        og += (unsigned)((og < (unsigned)stride ? sl : S - 1) * stride);
        os += (unsigned)((os < (unsigned)stride ? sl : S - 1) * stride);
        if constexpr (PACK_NBR) {
            gat[j] = og | (os << 16);
        } else {
            gat[j] = og;            // (the compiler keeps the 12 byte addresses in registers)
            sto[j] = os;
        }
    }
    // word offsets of edge j: its variable's record, its own word
    auto rec_of = [&](int j) -> unsigned {
        if constexpr (PACK_NBR) {
            // (opaque: otherwise the unpacked byte addresses are hoisted out of the iteration loop --
            // loop-invariant -- and spilled to scratch)
            unsigned pk = gat[j];
            asm volatile("" : "+v"(pk));
            return pk & 0xffffu;
        } else {
            return gat[j];
        }
    };
    auto own_of = [&](int j) -> unsigned {
        if constexpr (PACK_NBR) {
            unsigned pk = gat[j];
            asm volatile("" : "+v"(pk));
            return pk >> 16;
        } else {
            return sto[j];
        }
    };
    if (lane_valid) wmask = P.tab_writer[c];
    if (lds_address(smem_all) != np_tab) __builtin_trap();
    np_tables_to_lds(smem_all, tid, blockDim.x);
    if (use_r0) __syncthreads();                    // (the table of first check steps uses them)
    if (use_r0 && lane_valid && slot == 0) {
        // (this lane wrote the priors it reads here; the table is published by the barrier before the loop)
        double qp[DC];
#pragma unroll
        for (int j = 0; j < DC; ++j) qp[j] = pri_lds[j * m + c];
        check_step(qp, 0u, [&](int j, double r) { r0_lds[j * m + c] = r; });
        check_step(qp, 1u, [&](int j, double r) { r0_lds[(DC + j) * m + c] = r; });
    }

    const long long B = P.B;
    const long long total_slots = (long long)gridDim.x * S;
    const double one_minus_damping = 1.0 - P.damping;
    const int max_iter = P.max_iter;

    // Work distribution: the first syndrome of a slot is static; afterwards the slot leader draws
    // chunks of consecutive indices from one global counter.  A single word sustains only ~88
    // dequeues/us (MI355X_MICROARCH.md 'dequeue'), which early-exit decoding at low error rates
    // would exceed with one atomic per syndrome -- and a chunk of eight syndromes that all run
    // max_iter iterations is a 8 x max_iter iteration tail on one slot while others idle (the
    // reference driver's 5 000-syndrome batches at p = 0.05, maxIter 150: 3.5 ms instead of 2.05).
    // Chunk = the larger of
    //   * a share of what is left: 8 / 4 / 2 / 1 syndromes while >= 16 / 8 / 4 / 0 per slot remain
    //     (judged by the slot's own last index: the counter may be a chunk per slot further), and
    //   * what the workgroup's recent syndromes cost: 8 while they took < 3 iterations on average,
    //     4 / 2 below 7 / 15, else 1 (work_chunk_for).  That running mean starts at max_iter, jumps
    //     up with one slow syndrome and decays by a quarter per finished one: the first syndromes
    //     to finish are the easy ones, and must not earn a slot eight hard ones.
    // Measured against a fixed chunk of 8 and three other rules: profiles/r02_ab_work_chunk.txt.
    auto work_chunk = [&](long long handed_out, int by_cost) -> int {
        if (QBP_WORK_CHUNK_FIXED) return FORCE_FULL ? 1 : 8;                       // (A/B: round 1's rule)
        const long long rem = B - handed_out;
        const int share = rem >= 16 * total_slots ? 8 : rem >= 8 * total_slots ? 4 : rem >= 4 * total_slots ? 2 : 1;
        const int ch = share > by_cost ? share : by_cost;
        // (small codes decode so many syndromes per microsecond -- [[72,12,6]]: 640 at p = 0.01 -- that eight per
        // atomic still is 80 fetches/us on one word: two or four times as many while plenty remain)
        const int f = QBP_WORK_CHUNK_SMALL_CODES ? (m <= 36 ? 4 : m <= 72 ? 2 : 1) : 1;
        return (f > 1 && ch == 8 && rem >= (long long)16 * f * total_slots) ? 8 * f : ch;
    };
    long long b = lane_valid ? (long long)blockIdx.x * S + slot : B;
    bool active = b < B;

    // the zero record, and the trailing words of the records of columns with fewer than DV checks, which nobody
    // writes afterwards (both copies): published by the barrier before the loop
    for (int i = tid; i < r_doubles; i += blockDim.x) {
        smem[i] = 0.0;
        if constexpr (ONE_BAR) smem[FUSED_R2_OFF_BYTES / 8 + i] = 0.0;
    }
    if (leader) {
        flag0[slot] = 0;
        flag0[S + slot] = 0;
        flag0[2 * S + slot] = 0;
        mc_lmask[slot] = 0ull;
        mc_weight[slot] = 0;
        mc_diff[slot] = 0;
        if constexpr (SPECTRUM) spec_words()[slot] = 0;
        if (slot == 0) *work_avg = 4 * P.max_iter;
        if constexpr (BUDGETS) {
            for (int i = 0; i < slot_counters; ++i) mc_count[i] = 0;
        } else if constexpr (MC) {
            for (int i = 0; i < NUM_COUNTERS; ++i) mc_count[i] = 0;
        }
        // (a launch whose syndromes are all some slot's first one never touches the counter: tens of
        // thousands of atomics on one word in the same microsecond are not free -- 40 us for 10 000)
        const int ch = work_chunk(9 * total_slots, 1);      // (every slot fetches at this moment)
        const long long first =
            B > total_slots ? total_slots + (long long)atomicAdd(P.work_counter, (unsigned long long)ch) : B;
        next_work[slot] = first;
        chunk_ends[slot] = first + ch;
    }
    if (tid == 0) {
        long long first = (long long)blockIdx.x * S;
        long long cnt = B - first;
        *active_count = (int)(cnt < 0 ? 0 : (cnt > S ? S : cnt));
    }
    if constexpr (SPECTRUM) {
        int* const it_hist = spec_words() + S;
        for (int i = tid; i <= P.max_iter; i += blockDim.x) it_hist[i] = 0;
    }
    if constexpr (LLRHIST) {
        const int bins = COLD(llr_bins);
        double* const le = llr_edges_lds();
        const double* const ge = COLD(llr_edges);
        for (int i = tid; i <= bins; i += blockDim.x) le[i] = ge[i];
        if (tid == 0) le[bins + 1] = (double)bins / (ge[bins] - ge[0]);
        unsigned* const tab = reinterpret_cast<unsigned*>(le + bins + 2);
        const int cells = COLD(n_budgets) * LLR_HIST_ROWS * (bins + 3);
        for (int i = tid; i < cells; i += blockDim.x) tab[i] = 0u;
    }

    // The lane's own check->variable messages are needed again in the variable step (Q = value - R):
    // kept in registers across barrier B1, or re-read from LDS through the edge's store address (one
    // ds_read_b64 per edge, no vector-ALU cost, but a scatter over the banks like the store) to save
    // 2 * DC registers.  The defaults date from the check-major layout (profiles/r02_ab_wide_mc.txt:
    // Monte-Carlo builds 6.6 % faster re-reading, the (8, 4) shape 4 % faster holding), where the re-read
    // was conflict-free and the Monte-Carlo builds spilled.  On the variable-major layout
    // (profiles/r20_ab_r_layout.txt): the headline decode build is 2.2 % faster holding; every leg with
    // these defaults is at or above its check-major time; the (6, 3) Monte-Carlo builds, which no longer
    // spill either way, measured 2.2 % faster HOLDING at p = 0.05 (0.9 % at p = 0.01, inside that leg's
    // spread) -- QBP_MC_HOLD_R=1 is the candidate for the next change, not yet run through the suite.
    constexpr bool HOLD_R = MC ? (QBP_MC_HOLD_R != 0 && DC <= 6) : (DC <= 6 ? QBP_SMALL_HOLD_R != 0 : QBP_WIDE_HOLD_R != 0);

    // ---- per-syndrome state ---------------------------------------------------------------
    double Q[DC];
    double R[HOLD_R ? DC : 1];
    unsigned sbit = 0, ebits = 0;
    int it = 0;
    bool frozen = false;
    // BUDGETS: row of the trial's next checkpoint and the iteration that ends that budget (uniform per slot);
    // comparing `it` with ck_it is all an iteration gains
    int bj = 0, ck_it = 0;

    auto start_syndrome = [&]() {
        it = 0;
        frozen = false;
        if constexpr (BUDGETS) { bj = 0; ck_it = COLD(budgets)[0] - 1; }
#pragma unroll
        for (int j = 0; j < DC; ++j) Q[j] = pri_lds[j * m + c];   // Q = where(mask, initialBelief, 0)
        if constexpr (SHOTS) {
            sbit = mc_shot_bit(COLD(det_bits), b, COLD(det_row_bytes), c);
        } else if constexpr (MC) {
            ebits = 0;
            const unsigned char* const err_lds = err_buf();
#pragma unroll
            for (int j = 0; j < DC; ++j) {
                const int v = var_lds[j * m + c];
                if (v >= 0) ebits |= (unsigned)err_lds[v] << j;
            }
            sbit = __builtin_popcount(ebits) & 1u;       // syndrome = H e mod 2
        } else {
            sbit = COLD(syndromes)[b * m + c] & 1u;
        }
    };
    bool need_start = active;     // (re)initialise at the loop top, where Q / val / R are dead
    __syncthreads();

    // leader-only bookkeeping (refill: 0, or the size of the next chunk should one be needed)
    int refill = 0;
    bool mc_pending = false;
    int mc_pending_conv = 0, mc_pending_it = 0;
    int mc_pending_row = 0;       // BUDGETS: the row of the pending emission (a checkpoint and the trial's convergence
                                  // one phase later are consecutive emissions of one slot)
    // the slot's counter row of a pending emission
    auto pending_row = [&]() -> int* {
        if constexpr (BUDGETS)
            return mc_count + ((mc_pending_conv ? COLD(n_budgets) : 0) + mc_pending_row) * NUM_COUNTERS;
        else
            return mc_count;
    };

    // SPECTRUM: the pending emission's share of the two tables, by the slot leader just before mc_classify (which
    // clears the logical mask): the iteration bin of every trial, deferred to OSD or not, and the residual weight of
    // a trial classified here (the OSD kernels add those of the deferred ones)
    auto spectrum_pending = [&]() {
        const ColdArgs ca = cold_args();
        int* const sw = spec_words();
        atomicAdd(&sw[S + (mc_pending_conv ? mc_pending_it : ca->max_iter)], 1);
        if (ca->fail_list != nullptr && !mc_pending_conv) return;
        const int w = sw[slot];
        if (w) {
            sw[slot] = 0;
            const int row = mc_spectrum_row(mc_pending_conv != 0, mc_lmask[slot] != 0ull);
            atomicAdd(reinterpret_cast<unsigned long long*>(ca->spectrum + (long long)row * (ca->n + 1) + w), 1ull);
        }
    };

    // SHOTS: the pending emission by the slot leader: bookkeeping counters, the converged flag, and -- unless the shot
    // is left to OSD, whose kernel does the same for its records -- the prediction and its compare with the record
    // (the shot of a pending emission -- the slot may be on its next one by then -- waits in the slot's words of
    // mc_weight / mc_diff, its iteration and converged flag in the slot's word of the third flag buffer, none of which
    // these builds use otherwise: written and read by the leader alone, and three registers fewer across the loop)
    auto shots_pending = [&]() {
        const ColdArgs ca = cold_args();
        const int mc_pending_conv = flag0[2 * S + slot] & 1, mc_pending_it = flag0[2 * S + slot] >> 1;
        const long long mc_pending_b = (long long)(((unsigned long long)(unsigned)mc_diff[slot] << 32) |
                                                   (unsigned)mc_weight[slot]);
        mc_count_shot(mc_count, mc_pending_conv, mc_pending_it);
        if (ca->converged) ca->converged[mc_pending_b] = (uint8_t)mc_pending_conv;
        if (ca->fail_list != nullptr && !mc_pending_conv) return;
        const unsigned long long pred = mc_lmask[slot];
        mc_lmask[slot] = 0ull;
        if (ca->predictions) ca->predictions[mc_pending_b] = pred;
        if (ca->actual && ca->actual[mc_pending_b] != pred) {
            mc_count[1] += 1;
            if (!mc_pending_conv) mc_count[8] += 1;
        }
    };

    double val_keep[DC];          // ONE_BAR: posterior values of the lane's edges, alive until the next phase
    // decode-mode emission of the values in val[] (one read of the output pointers per emission --
    // adjacent kernel arguments: a single scalar load -- not one per use)
    auto emit_decode = [&](const double (&val)[DC], bool conv, int it_out) {
        const ColdArgs ca = cold_args();
        double* const o_llr = ca->llr;
        uint8_t* const o_hard = ca->hard;
        const long long row = b * ca->n;
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            if ((wmask >> j) & 1u) {
                const long long o = row + var_lds[j * m + c];
                if (o_llr) o_llr[o] = val[j];
                if (o_hard) o_hard[o] = (uint8_t)(val[j] < 0.0);
            }
        }
        const int n_iso = ca->n_iso;
        for (int i = c; i < n_iso; i += m) {
            const int v = COLD(iso_vars)[i];
            const double pv = COLD(prior)[v];
            if (o_llr) o_llr[row + v] = pv;
            if (o_hard) o_hard[row + v] = pv < 0.0;
        }
        if (c == 0) {
            if (ca->converged) ca->converged[b] = conv;
            if (ca->iters) ca->iters[b] = it_out;
        }
    };
    // flag buffers: written in phase p (f_cur), read after the next synchronisation, cleared by the leader
    // one phase ahead (f_next); ONE_BAR reads them one phase later (f_prev), hence three of them
    int f_cur = 0, f_next = 1, f_prev = 2;
    int wg_it = 0;                // ONE_BAR: iteration index of every active slot (they run in step)

    auto phase_body = [&](auto par_tag) -> bool {
        constexpr int PAR = decltype(par_tag)::value;
        double* const Rw = ONE_BAR ? smem + PAR * (FUSED_R2_OFF_BYTES / 8) : smem;     // this phase's copy of R
        double val_phase[DC];     // (two-barrier builds: the values do not outlive the phase)
        double (&val)[DC] = ONE_BAR ? val_keep : val_phase;
        if constexpr (MC && !SHOTS) {
            // Sample the errors of a trial that starts in this phase: one Philox evaluation per
            // four qubits, by the first ceil(n/4) lanes of the slot; the extra barrier (Monte-Carlo
            // builds only) orders the bytes before the check lanes gather them.
            if (need_start) {
                err_par ^= 1u;
                unsigned* const err_words = reinterpret_cast<unsigned*>(err_buf());
                const unsigned long long trial = (unsigned long long)(COLD(trial_begin) + b);
#if QBP_MC_SPECTRUM || QBP_MC_LLRHIST   /* per-qubit thresholds, or stored errors (qbp_mc_run_errors_spectrum, _llr_hist) */
                const uint32_t* const thr = COLD(thr_cols);
                const uint8_t* const ein = COLD(errors_in);
                for (int g = c; g < P.n_words4; g += m)
                    err_words[g] = ein ? mc_stored_quad(ein + b * COLD(n), g, COLD(n))
                                       : mc_error_quad_cols(trial, g, COLD(draws), COLD(seed), thr);
#elif QBP_MC_COLS
                const uint32_t* const thr = COLD(thr_cols);
                for (int g = c; g < P.n_words4; g += m)
                    err_words[g] = mc_error_quad_cols(trial, g, COLD(draws), COLD(seed), thr);
#else
                const uint8_t* const ein = COLD(errors_in);
                for (int g = c; g < P.n_words4; g += m)
                    err_words[g] = ein ? mc_stored_quad(ein + b * COLD(n), g, COLD(n))
                                       : mc_error_quad(trial, g, COLD(draws), COLD(seed), COLD(threshold));
#endif
            }
            __syncthreads();                                      // B0
        }
        if (need_start) { start_syndrome(); need_start = false; }
        // ================= check step =======================================================
        if (active) {
            if (use_r0 && it == 0) {
                // first check step of a syndrome: from the workgroup's table (see r0_lds)
                const double* const r0 = r0_lds + (sbit ? DC * m : 0);
#pragma unroll
                for (int j = 0; j < DC; ++j) {
                    const double r = r0[j * m + c];
                    Rw[own_of(j)] = r;
                    if constexpr (HOLD_R) R[j] = r;
                }
            } else {
                check_step(Q, sbit, [&](int j, double r) {
                    Rw[own_of(j)] = r;
                    if constexpr (HOLD_R) R[j] = r;
                });
            }
        }
        __syncthreads();                                          // B1
        if (*active_count == 0) return true;

        // ================= variable step (per edge of this check) ============================
        if constexpr (ONE_BAR) {
            // iteration it - 1 of this syndrome satisfied it (its flag is complete since the barrier above):
            // its posterior values, still in val[], are the outputs (beliefPropagationGPU.py:160-167)
            // (every active slot is in iteration wg_it: the scalar stands for the per-slot `it`, which these builds
            // do not keep)
            if (active && wg_it > 0 && !frozen && flag0[f_prev * S + slot] == 0) {
                emit_decode(val, true, wg_it - 1);
                frozen = true;
            }
        }
        if (active) {
            bool odd = sbit != 0;                                 // parity of the row vs syndrome
            // Issue the LDS gathers of a group of edges before the first add (one lgkmcnt wait per
            // group instead of two per edge): all 18 for the (6, 3) shape, QBP_WIDE_JG edges at a time
            // for the (8, 4) shape, whose register budget is the tighter constraint.  An edge's DV reads
            // go off one address with immediate offsets, as ds_read_b64: records are not 16-byte aligned
            // (24 bytes for DV = 3; for DV = 4 they overlap on their zero words, see fused_r_doubles).
            constexpr int JG = (DC * DV <= 18) ? DC : QBP_WIDE_JG;
#pragma unroll
            for (int j0 = 0; j0 < DC; j0 += JG) {
                double rr[JG][DV];
                double rown[HOLD_R ? 1 : JG];
#pragma unroll
                for (int jj = 0; jj < JG; ++jj) {
                    if (j0 + jj < DC) {
                        const double* const rec = Rw + rec_of(j0 + jj);
                        // (volatile: neighbouring words would otherwise be fetched by one ds_read2_b64,
                        // which needs an address add of its own -- its offsets are too short for the second
                        // copy -- and moves half the bytes per LDS cycle of ds_read_b64)
                        const volatile __attribute__((address_space(3))) double* const rv =
                            (const volatile __attribute__((address_space(3))) double*)rec;
#pragma unroll
                        for (int k = 0; k < DV; ++k) rr[jj][k] = rv[k];
                        if constexpr (!HOLD_R) rown[jj] = Rw[own_of(j0 + jj)];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int jj = 0; jj < JG; ++jj) {
                    const int j = j0 + jj;
                    if (j >= DC) break;
                    double s = rr[jj][0];
#pragma unroll
                    for (int k = 1; k < DV; ++k) s = s + rr[jj][k];   // ascending check order
                    val[j] = s + pri_lds[j * m + c];
                    odd ^= val[j] < 0.0;                              // hard decision: values < 0
                    double r_own;
                    if constexpr (HOLD_R) r_own = R[j]; else r_own = rown[jj];
                    const double qn = val[j] - r_own;
                    if constexpr (VARIANT == 0) {
                        Q[j] = qn;
                    } else {
                        Q[j] = damped_q(qn, Q[j], P.damping, one_minus_damping, P.clip_llr);
                    }
                }
            }
            if (P.padded) {                                       // wave-uniform branch
#pragma unroll
                for (int j = 0; j < DC; ++j)
                    if (!((vmask >> j) & 1u)) Q[j] = __builtin_inf();   // padding stays neutral
            }
            if (odd) flag0[f_cur * S + slot] = 1;                 // this check is unsatisfied
        }
        if (leader) {
            flag0[f_next * S + slot] = 0;
            if (refill) {
                long long nx = next_work[slot] + 1;
                if (nx == chunk_ends[slot]) {
                    const int ch = work_chunk(nx, refill);
                    nx = total_slots +
                         (long long)atomicAdd(COLD(work_counter), (unsigned long long)ch);
                    chunk_ends[slot] = nx + ch;
                }
                next_work[slot] = nx;
                refill = 0;
            }
            if constexpr (MC) {
                if (mc_pending) {
                    if constexpr (SHOTS) {
                        shots_pending();
                    } else {
                    if constexpr (SPECTRUM) spectrum_pending();
                    mc_classify(mc_lmask, mc_weight, mc_diff, pending_row(), slot, mc_pending_conv,
                                mc_pending_it, COLD(half_distance),
                                COLD(fail_list) != nullptr && !mc_pending_conv);
                    }
                    mc_pending = false;
                }
            }
        }
        // (ONE_BAR: only the last iteration of a syndrome settles here; wg_it is workgroup-uniform)
        const bool settle = !ONE_BAR || wg_it == max_iter - 1;
        if (settle) __syncthreads();                              // B2

        // ================= convergence / output / next syndrome ==============================
        if (active && settle) {
            const bool conv = flag0[f_cur * S + slot] == 0;
            // (ONE_BAR: this block runs once per syndrome; reading the limit from the kernel-argument
            // segment here is also what tells tools/valu_mix.py so -- its rule for once-per-syndrome code)
            const int it_now = ONE_BAR ? wg_it : it;
            const bool last = it_now == (ONE_BAR ? COLD(max_iter) : max_iter) - 1;
            // (BUDGETS: the end of budget bj is an emission too -- for row bj -- whether it is the last one or not)
            bool emit_now = conv || last;
            if constexpr (BUDGETS) emit_now = conv || it == ck_it;
            if (!frozen && emit_now) {
                if constexpr (MC) {
                    const ColdArgs ca = cold_args();     // one read of the cold arguments per emission
                    long long rec = b;                   // failure record of this emission
                    if constexpr (BUDGETS) rec = (long long)bj * ca->B + b;
                    const long long row = rec * ca->n;
                    const int n_iso = ca->n_iso;
                    if (ca->fail_list != nullptr && !conv) {
                        // BP failed: leave the trial to the OSD kernel (record indexed by b)
                        double* const f_llr = ca->fail_llr;
                        uint8_t* const f_hard = ca->fail_hard;
                        uint8_t* const f_err = ca->fail_err;
                        ca->fail_syn[rec * m + c] = (uint8_t)sbit;
#pragma unroll
                        for (int j = 0; j < DC; ++j) {
                            if ((wmask >> j) & 1u) {
                                const long long o = row + var_lds[j * m + c];
                                f_llr[o] = val[j];
                                f_hard[o] = (uint8_t)(val[j] < 0.0);
                                if constexpr (!SHOTS) f_err[o] = (uint8_t)((ebits >> j) & 1u);
                            }
                        }
                        const unsigned char* const err_lds = SHOTS ? nullptr : err_buf();
                        for (int i = c; i < n_iso; i += m) {
                            const int v = COLD(iso_vars)[i];
                            const double pv = COLD(prior)[v];
                            f_llr[row + v] = pv;
                            f_hard[row + v] = (uint8_t)(pv < 0.0);
                            if constexpr (!SHOTS) f_err[row + v] = err_lds[v];
                        }
                        if constexpr (BUDGETS) {         // list bj, of the records of plane bj
                            if (c == 0) ca->fail_list[bj * ca->B + (long long)atomicAdd(ca->fail_count + bj, 1ull)] = b;
                        } else {
                            if (c == 0) ca->fail_list[atomicAdd(ca->fail_count, 1ull)] = b;
                        }
                    } else if constexpr (SHOTS) {
                        // prediction = Lx x mod 2 over the support of the hard decision x (this lane's share)
                        unsigned long long lm = 0ull;
                        const unsigned long long* const lx = ca->lx_cols;
#pragma unroll
                        for (int j = 0; j < DC; ++j)
                            if (((wmask >> j) & 1u) && val[j] < 0.0) lm ^= lx[var_lds[j * m + c]];
                        for (int i = c; i < n_iso; i += m) {
                            const int v = COLD(iso_vars)[i];
                            if (COLD(prior)[v] < 0.0) lm ^= lx[v];
                        }
                        if (lm) atomicXor(&mc_lmask[slot], lm);
                    } else {
                    unsigned long long lm = 0ull;
                    int ew = 0;
                    unsigned df = 0;
                    int rw = 0;                          // SPECTRUM: weight of the residual (this lane's share)
                    const unsigned long long* const lx = ca->lx_cols;
#pragma unroll
                    for (int j = 0; j < DC; ++j) {
                        if ((wmask >> j) & 1u) {
                            const unsigned e = (ebits >> j) & 1u;
                            const unsigned res = (val[j] < 0.0 ? 1u : 0u) ^ e;
                            ew += (int)e;
                            df |= res;
                            if constexpr (SPECTRUM) rw += (int)res;
                            const int v = var_lds[j * m + c];
                            if (res) lm ^= lx[v];
                        }
                    }
                    const unsigned char* const err_lds = err_buf();
                    for (int i = c; i < n_iso; i += m) {
                        const int v = COLD(iso_vars)[i];
                        const unsigned e = err_lds[v];
                        const unsigned res = (COLD(prior)[v] < 0.0 ? 1u : 0u) ^ e;
                        ew += (int)e;
                        df |= res;
                        if constexpr (SPECTRUM) rw += (int)res;
                        if (res) lm ^= lx[v];
                    }
                    if constexpr (SPECTRUM) {
                        if (rw) atomicAdd(&spec_words()[slot], rw);
                    }
                    if (lm) atomicXor(&mc_lmask[slot], lm);
                    if (ew) atomicAdd(&mc_weight[slot], ew);
                    if (df) atomicOr(&mc_diff[slot], 1);
                    }
                    if constexpr (LLRHIST) {
                        // this lane's variables into plane bj, rows 2 * !conv + error bit, behind the classification
                        // (its accumulators are dead by now): a run of equal cells among the lane's own values, in edge
                        // order, is one LDS atomic; only the previous cell and the length of its run are kept
                        const int bins = ca->llr_bins, ncol = bins + 3;
                        const double* const le = llr_edges_lds();
                        unsigned* const rows = reinterpret_cast<unsigned*>(const_cast<double*>(le) + bins + 2) +
                                               (bj * LLR_HIST_ROWS + (conv ? 0 : 2)) * ncol;
                        int prev = -1;                       // the run of equal cells so far, and its length
                        unsigned run = 0u;
#pragma unroll
                        for (int j = 0; j < DC; ++j) {
                            if ((wmask >> j) & 1u) {
                                const int cell = (int)((ebits >> j) & 1u) * ncol + llr_hist_col(val[j], le, bins);
                                if (cell != prev) {
                                    if (run) atomicAdd(&rows[prev], run);
                                    prev = cell; run = 0u;
                                }
                                ++run;
                            }
                        }
                        if (run) atomicAdd(&rows[prev], run);
                        const unsigned char* const err_lds = err_buf();
                        for (int i = c; i < n_iso; i += m) {         // isolated variables: the value is the prior
                            const int v = COLD(iso_vars)[i];
                            atomicAdd(&rows[(int)(err_lds[v] & 1u) * ncol + llr_hist_col(COLD(prior)[v], le, bins)], 1u);
                        }
                    }
                    if (c == 0) {
                        mc_pending = true;
                        if constexpr (!SHOTS) { mc_pending_conv = conv; mc_pending_it = it; }
                        if constexpr (BUDGETS) mc_pending_row = bj;
                        if constexpr (SHOTS) {
                            flag0[2 * S + slot] = (it << 1) | (conv ? 1 : 0);
                            mc_weight[slot] = (int)(unsigned)b;
                            mc_diff[slot] = (int)(unsigned)((unsigned long long)b >> 32);
                        }
                    }
                } else {
                    emit_decode(val, conv, it_now);
                }
            }
            if (conv) frozen = true;
            const bool finished = last || (conv && !FORCE_FULL);
            if (finished) {
                b = next_work[slot];
                if (b < B) {
                    need_start = true;
                    if (c == 0) {                  // (the counter only grows: past B, nothing to fetch)
                        if constexpr (FORCE_FULL) {
                            refill = 1;
                        } else {
                            // (shared by the slot leaders of the workgroup: a lost update is harmless)
                            const int a4 = *work_avg;
                            const int n4 = it * 4 > a4 ? it * 4 : a4 - (a4 >> 2) + it;
                            *work_avg = n4;
                            refill = work_chunk_for(n4);
                        }
                    }
                } else {
                    active = false;
                    if (c == 0) atomicSub(active_count, 1);
                }
            } else {
                if constexpr (BUDGETS) {
                    // budget bj ends here and is not the last one: on to the next checkpoint
                    if (it == ck_it) { ++bj; ck_it = COLD(budgets)[bj] - 1; }
                }
                ++it;
            }
        }
        {   // next phase
            const int t = f_prev; f_prev = f_cur; f_cur = f_next; f_next = ONE_BAR ? t : f_prev;
            if constexpr (ONE_BAR) wg_it = wg_it == max_iter - 1 ? 0 : wg_it + 1;
        }
        return false;
    };
    for (;;) {
        if (phase_body(std::integral_constant<int, 0>{})) break;
        if constexpr (ONE_BAR) {
            if (phase_body(std::integral_constant<int, 1>{})) break;
        }
    }

    if constexpr (MC) {
        if (leader) {
            // the last emitted trial of this slot may still be pending (emitted after B2 of the
            // final phase; everybody passed B1 since, so the accumulators are complete)
            if (mc_pending) {
                if constexpr (SHOTS) {
                    shots_pending();
                } else {
                if constexpr (SPECTRUM) spectrum_pending();
                mc_classify(mc_lmask, mc_weight, mc_diff, pending_row(), slot, mc_pending_conv,
                            mc_pending_it, COLD(half_distance),
                            COLD(fail_list) != nullptr && !mc_pending_conv);
                }
            }
            if constexpr (!BUDGETS) {
                for (int i = 0; i < NUM_COUNTERS; ++i)
                    if (mc_count[i])
                        atomicAdd(reinterpret_cast<unsigned long long*>(COLD(counters) + i),
                                  (unsigned long long)mc_count[i]);
            }
        }
        if constexpr (SPECTRUM) {
            // the workgroup's iteration histogram: one global atomic per non-zero bin.  (The loop above ends for all
            // threads in the same phase.)
            __syncthreads();
            long long* const out = COLD(iter_hist);
            const int* const it_hist = spec_words() + S;
            if (out != nullptr)
                for (int i = tid; i <= COLD(max_iter); i += blockDim.x)
                    if (it_hist[i])
                        atomicAdd(reinterpret_cast<unsigned long long*>(out + i), (unsigned long long)it_hist[i]);
        }
        if constexpr (BUDGETS) {
            // counters[j][i] += sum over the slots of exact[j][i] + from[0 .. j][i]: one thread per (j, i), one
            // atomic per non-zero entry and workgroup.  (The loop above ends for all threads in the same phase.)
            __syncthreads();
            const int K = COLD(n_budgets);
            const int* const tab = words + 6 * S + 1;            // [S][2][K][NUM_COUNTERS]
            for (int t = tid; t < K * NUM_COUNTERS; t += blockDim.x) {
                const int j = t / NUM_COUNTERS, i = t - j * NUM_COUNTERS;
                long long sum = 0;
                for (int s = 0; s < S; ++s) {
                    const int* const rows = tab + s * slot_counters;
                    sum += rows[j * NUM_COUNTERS + i];
                    for (int jj = 0; jj <= j; ++jj) sum += rows[(K + jj) * NUM_COUNTERS + i];
                }
                if (sum)
                    atomicAdd(reinterpret_cast<unsigned long long*>(COLD(counters) + t), (unsigned long long)sum);
            }
            if constexpr (LLRHIST) {
                // llr_hist[j][r][col] += exact[j] for the unconverged rows, the sum of from[0 .. j] for the converged
                // ones: one thread per cell, one atomic per non-zero cell and workgroup
                const int bins = COLD(llr_bins), ncol = bins + 3;
                const unsigned* const lt = reinterpret_cast<const unsigned*>(llr_edges_lds() + bins + 2);
                for (int t = tid; t < K * LLR_HIST_ROWS * ncol; t += blockDim.x) {
                    const int j = t / (LLR_HIST_ROWS * ncol), rc = t - j * (LLR_HIST_ROWS * ncol);
                    unsigned long long sum = lt[t];
                    if (rc < 2 * ncol)
                        for (int jj = 0; jj < j; ++jj) sum += lt[jj * LLR_HIST_ROWS * ncol + rc];
                    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(COLD(llr_hist) + t), sum);
                }
            }
        }
    }
}

#ifdef QBP_DEFINE_KERNELS   /* non-template kernels: defined in their translation unit only */
// Device evaluation of the math functions (accuracy tests).
__global__ void debug_math_kernel(int kind, const double* x, double* y, long long n)
{
    __shared__ __attribute__((aligned(16))) double np_lds[NP_LDS_DOUBLES];
    np_tables_to_lds(np_lds, threadIdx.x, blockDim.x);
    const NpT np_tab = lds_address(np_lds);
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    switch (kind) {
        case 0: y[i] = tanh_half_msg<0>(v, np_tab); break;        // the kernels' tanh(q / 2)
        case 1: y[i] = atanh2_msg(v, np_tab); break;               // the kernels' 2 atanh(y)
        case 4: y[i] = tanh_half(v); break;                        // round-1/2 forms (QBP_MATH_FAST builds)
        case 5: y[i] = atanh2(v); break;
        case 2: y[i] = __builtin_amdgcn_rcp(v); break;          // raw v_rcp_f64 (seed accuracy)
        default: y[i] = div_nr(1.0, v); break;
    }
}

// The Monte-Carlo sampler on its own (qbp_mc_sample_errors): errors [T][n] of trials trial_begin .. + T, one
// Philox evaluation per four qubits -- the bytes every Monte-Carlo kernel draws for itself (mc_error_quad).
__global__ void mc_sample_kernel(uint8_t* errors, int n, long long T, long long trial_begin, int draws,
                                 unsigned long long seed, unsigned threshold)
{
    const int n4 = (n + 3) / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * n4) return;
    const long long b = i / n4;
    const int g = (int)(i - b * n4);
    const unsigned q = mc_error_quad((unsigned long long)(trial_begin + b), g, draws, seed, threshold);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * g + k < n) errors[b * n + 4 * g + k] = (uint8_t)((q >> (8 * k)) & 1u);
}

// ... with a threshold per qubit (qbp_mc_sample_errors_probs; thr as in mc_error_quad_cols)
__global__ void mc_sample_cols_kernel(uint8_t* errors, int n, long long T, long long trial_begin, int draws,
                                      unsigned long long seed, const uint32_t* thr)
{
    const int n4 = (n + 3) / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * n4) return;
    const long long b = i / n4;
    const int g = (int)(i - b * n4);
    const unsigned q = mc_error_quad_cols((unsigned long long)(trial_begin + b), g, draws, seed, thr);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * g + k < n) errors[b * n + 4 * g + k] = (uint8_t)((q >> (8 * k)) & 1u);
}

// The fixed-weight sampler (qbp_mc_run_weight, qbp_mc_sample_errors_weight; specification: include/qbp.h): row b of
// errors [T][n] becomes a uniform w-subset of the n columns, by Floyd's algorithm on the Philox stream of trial
// trial_begin + b -- step i draws u in [0, j], j = n - w + i, and takes u, or j when u is taken already (j itself
// cannot be: every earlier step chose below j).  One lane per trial: the w steps depend on each other, trials do
// not.  The trial's own row is the membership map, so any n works without LDS or an indexed register array; it has
// to be ZERO on entry (launch_mc_sample_weight clears it on the same stream).  The inner loop is unrolled so that
// the four Philox words are indexed statically.
__global__ void mc_sample_weight_kernel(uint8_t* errors, int n, int w, long long T, long long trial_begin,
                                        unsigned long long seed)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= T) return;
    const unsigned long long trial = (unsigned long long)(trial_begin + b);
    uint8_t* const row = errors + b * n;
    for (int i0 = 0; i0 < w; i0 += 4) {
        unsigned c[4] = {(unsigned)trial, (unsigned)(trial >> 32), (unsigned)(i0 >> 2), 2u};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < w) {
                const unsigned j = (unsigned)(n - w + i0 + k);
                const unsigned u = __umulhi(c[k], j + 1u);       // (r (j + 1)) >> 32, in [0, j]
                row[row[u] ? j : u] = 1;
            }
        }
    }
}

// The fixed-weight FAULT sampler (qbp_mc_run_fault_weight, qbp_mc_sample_errors_fault_weight; specification:
// include/qbp.h): trial trial_begin + b picks w of the N fault sites by Floyd's algorithm, as the sampler above picks
// columns, draws one of the K[s] codes of every picked site from a second Philox block (counter word 2 with its top bit
// set), and toggles column fault_column[first_fault[s] + code] of row b of errors [T][n]; a fault mapped to -1 toggles
// nothing, two faults of one column cancel.  One lane per trial.  Sites are not columns, so the row cannot be the
// membership map: the lane's picks go to picks [w][stride] (trial-minor: lane b owns column b, a wavefront's accesses
// coalesce), and step i tests u against rows 0 .. i - 1 of its own column -- a lane reads back its own stores only.  No
// LDS and no indexed register array; unrolled by four so that the Philox words are indexed statically.  The rows have
// to be ZERO on entry (launch_mc_sample_fault_weight clears them).  N <= 2^32 - 4, so j + 1 does not wrap; every picked
// s is in [0, N), first_fault[s] + code < n_faults and every column is in [-1, n) by the checks of qbp_fault_table_set.
constexpr unsigned FAULT_PHILOX_WORD3 = 6u;   // QBP_FAULT_PHILOX_STREAM of include/qbp.h
__global__ void mc_sample_fault_weight_kernel(uint8_t* errors, int n, int w, long long T, long long trial_begin,
                                              unsigned long long seed, const long long* first_fault,
                                              const uint8_t* site_k, const int32_t* fault_column, unsigned n_sites,
                                              uint32_t* picks, long long stride)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= T) return;
    const unsigned long long trial = (unsigned long long)(trial_begin + b);
    uint8_t* const row = errors + b * n;
    uint32_t* const mine = picks + b;
    for (int i0 = 0; i0 < w; i0 += 4) {
        unsigned c[4] = {(unsigned)trial, (unsigned)(trial >> 32), (unsigned)(i0 >> 2), FAULT_PHILOX_WORD3};
        unsigned d[4] = {(unsigned)trial, (unsigned)(trial >> 32), 0x80000000u | (unsigned)(i0 >> 2), FAULT_PHILOX_WORD3};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        philox4x32_10(d, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < w) {
                const int i = i0 + k;
                const unsigned j = n_sites - (unsigned)w + (unsigned)i;
                const unsigned u = __umulhi(c[k], j + 1u);       // (r (j + 1)) >> 32, in [0, j]
                bool taken = false;
                for (int q = 0; q < i; ++q) taken |= mine[(long long)q * stride] == u;
                const unsigned s = taken ? j : u;
                mine[(long long)i * stride] = s;
                const long long f = first_fault[s] + (long long)__umulhi(d[k], (unsigned)site_k[s]);
                const int v = fault_column[f];
                if (v >= 0) row[v] ^= 1;
            }
        }
    }
}

// The weight-w enumeration (qbp_mc_run_enum, qbp_mc_sample_errors_enum; specification: include/qbp.h): row b of
// errors [T][n] becomes the pattern of rank rank_begin + b in the lexicographic order of the ascending column tuples.
// With D = C(n, w) - 1 - rank the rule of the header is the combinadic of D: for t = w .. 1 take the largest j below
// the previous one with C(j, t) <= D, set column n - 1 - j and subtract C(j, t) (hockey stick: the sum over the
// skipped columns is C(n - lo, t) - C(j + 1, t)).  binom [w + 1][n + 1] holds C(j, t) at t * (n + 1) + j, saturated at
// 2^63 - 1 (every D is below 2^62); row t is monotone in j, so each step is a binary search in it.  One lane per
// pattern, w searches and w byte stores; the row has to be ZERO on entry (launch_mc_enum_weight clears it).  j stays in
// [t - 1, n - 1] whatever the table holds, so every store lands in the lane's own row.
__global__ void mc_enum_weight_kernel(uint8_t* errors, int n, int w, long long T, long long rank_begin,
                                      const unsigned long long* binom)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= T) return;
    uint8_t* const row = errors + b * n;
    const int stride = n + 1;
    unsigned long long D = binom[(size_t)w * stride + n] - 1ull - (unsigned long long)(rank_begin + b);
    int prev = n;
    for (int t = w; t >= 1; --t) {
        const unsigned long long* col = binom + (size_t)t * stride;
        int lo = t - 1, hi = prev - 1;           // C(t - 1, t) = 0 <= D: the answer is in [lo, hi]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (col[mid] <= D) lo = mid; else hi = mid - 1;
        }
        D -= col[lo];
        row[n - 1 - lo] = 1;
        prev = lo;
    }
}

// qbp_enum_failures, between the enumeration and the shots launches: the shot of every error row.  Item (b, g) with
// g < row_bytes packs checks 8 g .. 8 g + 7 of s = H e into byte g of det_bits [T][row_bytes] (stim's b8 layout,
// mc_shot_bit), padding bits zero; item (b, row_bytes) is actual[b] = Lx e, bit l = logical operator l.
__global__ void enum_pack_kernel(const uint8_t* errors, long long T, int m, int n, const int32_t* row_ptr,
                                 const int32_t* col_idx, const unsigned long long* lx_cols, uint8_t* det_bits,
                                 unsigned long long* actual)
{
    const int row_bytes = (m + 7) / 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * (row_bytes + 1)) return;
    const long long b = i / (row_bytes + 1);
    const int g = (int)(i - b * (row_bytes + 1));
    const uint8_t* const row = errors + b * n;
    if (g == row_bytes) {
        unsigned long long a = 0ull;
        for (int v = 0; v < n; ++v)
            if (row[v] & 1) a ^= lx_cols[v];
        actual[b] = a;
        return;
    }
    unsigned bits = 0u;
    for (int c = 8 * g; c < min(8 * g + 8, m); ++c) {
        unsigned s = 0u;
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) s ^= row[col_idx[e]];
        bits |= (s & 1u) << (c - 8 * g);
    }
    det_bits[b * row_bytes + g] = (uint8_t)bits;
}

// qbp_enum_failures, behind the shots launches: kind = (prediction != actual) | 2 (BP did not converge) of pattern
// rank_begin + b; the patterns with kind & what are appended to ranks / kinds.  A wavefront counts its hits with one
// ballot and reserves their places with one atomic on *found, which counts every hit; entries past cap are dropped.
__global__ void enum_capture_kernel(const unsigned long long* predictions, const unsigned long long* actual,
                                    const uint8_t* converged, long long T, long long rank_begin, int what,
                                    long long cap, long long* ranks, uint8_t* kinds, unsigned long long* found)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int kind = 0;
    if (b < T) kind = (predictions[b] != actual[b] ? 1 : 0) | (converged[b] ? 0 : 2);
    const bool hit = (kind & what) != 0;
    const unsigned long long mask = __ballot(hit);
    if (mask == 0ull) return;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0ull;
    if (lane == leader) base = atomicAdd(found, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader);
    if (!hit) return;
    const unsigned long long pos = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    if (pos < (unsigned long long)cap) {
        ranks[pos] = rank_begin + b;
        kinds[pos] = (uint8_t)kind;
    }
}

#endif  // QBP_DEFINE_KERNELS

}  // namespace qbp
