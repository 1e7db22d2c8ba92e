/*
 * qbp.h -- C ABI of libqbp.so, the MI355X (gfx950) belief-propagation decoder.
 *
 * The reference (michelebanfi/qLDPC) has no FFI layer: its operator API for this path is a set
 * of Python functions.  Each entry point below names the reference function(s) it replaces;
 * qldpc_amd/bp.py and qldpc_amd/dropin/decoding/ mirror those Python signatures on top of
 * this ABI through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every function returns 0 on success and a negative QBP_E_* code on failure; the message
 *     is available from qbp_last_error() (thread-local); no C++ exception crosses the ABI;
 *   - the caller owns every buffer; "host" entry points take host pointers, copy to and from
 *     the device on the handle's stream and synchronise before returning; "_device" entry
 *     points take device pointers, enqueue on the given HIP stream and return immediately;
 *   - a handle owns the device copies of the code's tables, is bound to one device and is not
 *     thread-safe (one handle per thread / GPU); distinct handles are independent;
 *   - launches of ONE handle share its work counter and scratch workspaces: "_device" calls on
 *     the same handle must be ordered on one stream (or by events); to overlap launches on
 *     several streams use one handle per stream;
 *   - every entry point makes the handle's device current for the duration of the call and
 *     restores the calling thread's device before returning;
 *   - there is NO CPU fallback: without a usable HIP device qbp_create fails with
 *     QBP_E_NO_DEVICE.
 */
#ifndef QBP_H
#define QBP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qbp_handle qbp_handle;

enum {
    QBP_OK = 0,
    QBP_E_INVALID = -1,     /* bad argument (shape, range, null pointer)            */
    QBP_E_NO_DEVICE = -2,   /* no HIP device / device index out of range            */
    QBP_E_HIP = -3,         /* a HIP runtime call failed                            */
    QBP_E_UNSUPPORTED = -4, /* operation not available for this matrix (Monte-Carlo / OSD limits) */
    QBP_E_NOMEM = -5
};

/* message-update rule */
enum {
    QBP_SUM_PRODUCT = 0, /* decoding/beliefPropagation.py:88-144 performBeliefPropagationFast
                            (= :6-85 performBeliefPropagation, rework/decoding.py:77-129,
                            decoding/beliefPropagationGPU.py:22-78 and :81-178 per sample) */
    QBP_DAMPED_SP = 1,   /* rework/decoding.py:131-191 performBeliefPropagation_Symmetric   */
    QBP_MIN_SUM = 2      /* rework/decoding.py:5-75    performMinSum_Symmetric              */
};

/* flags */
enum {
    QBP_FLAG_FORCE_FULL = 1u, /* run all max_iter iterations for every syndrome; outputs are still
                                 those of the first converged iteration (bench mode "M2") */
    QBP_FLAG_OSD0 = 2u,       /* qbp_mc_run only: trials BP does not converge on go through OSD-0
                                 (decoding/OSD.py) before classification, as paperResults.py:73-77 */
    QBP_FLAG_PAIRWISE_COLSUM = 4u, /* column sums in the order of np.sum over the gathered 1-D column,
                                 i.e. numpy's pairwise summation from 8 entries per column on: the
                                 loop form performBeliefPropagation (decoding/beliefPropagation.py:68).
                                 The dense forms (:129, rework/decoding.py) accumulate row by row =
                                 left to right, the default.  Only matrices with a column of weight
                                 >= 8 see a difference (they run on the general-H kernel). */
    QBP_FLAG_DENSE_F_COLSUM = 8u, /* column sums in the order of np.sum(R, axis=0) on a FORTRAN-ordered dense
                                 R: what the dense single-syndrome forms (decoding/beliefPropagation.py:129,
                                 rework/decoding.py:61,:119,:173) compute when the caller's H is Fortran-ordered,
                                 as the Hx of the reference's codes/ files is -- every (m, n) temporary inherits
                                 the layout of `mask = H != 0`, a column is contiguous, and numpy reduces it
                                 with its pairwise sum over all m entries (association by row index mod 8 and
                                 by halves above 128 rows).  The batch form (decoding/beliefPropagationGPU.py:147)
                                 works on C-ordered (B, m, n) arrays whatever H is: default order.
                                 QBP_E_UNSUPPORTED when some column's association is not a left-to-right sum
                                 of a reordering of its entries (possible from 4 entries per column on). */
    QBP_FLAG_FAST_MATH = 32u, /* opt-in, on-chip kernel only (matrices of the (6,3) / (8,4) shape classes; the other
                                 kernels ignore it): tanh and arctanh by rational / polynomial approximations of
                                 2.3 and 1.2 ulp (round 2's functions) instead of numpy's own two routines.  Posterior
                                 LLRs then follow numpy's to ~1e-6 relative while a syndrome converges early and
                                 drift apart like any other libm's on late convergers (tests/test_gpu_fast_math.py
                                 prints the table); hard decision, converged flag and iteration were identical
                                 to the reference's on every stored vector.  +28 % throughput on forced-50
                                 [[288,12,18]].  Default (flag clear): every output bit equal to the reference's. */
    QBP_FLAG_DENSE_F_COLSUM_ITER0 = 16u, /* ... at iteration 0 only: the damped variants (rework/decoding.py:5,
                                 :131) on a Fortran-ordered H of fewer than 32768 entries -- `Q_old = Q.copy()`
                                 is C-ordered and C order wins in `damping * Q_new + (1 - damping) * Q_old` (:65,
                                 :179) from then on (from 256 KiB numpy reuses the F-ordered temporary instead:
                                 QBP_FLAG_DENSE_F_COLSUM).  Host-pointer entry point only; implemented for
                                 the case where iteration 0 cannot depend on the order (uniform priors, checks
                                 of equal weight, columns of at most 3 entries), else QBP_E_UNSUPPORTED. */
    QBP_FLAG_OSD_CS = 64u,    /* order-w OSD, combination sweep (qbp_osd_batch below); order: QBP_OSD_ORDER_FLAGS.
                                 With qbp_mc_run* only together with QBP_FLAG_OSD0 */
    QBP_FLAG_OSD_E = 128u,    /* order-w OSD, exhaustive over the w least reliable non-pivot columns (same rules) */
    QBP_FLAG_OSD_LARGE = 256u,/* order-w OSD also on matrices beyond the one-wavefront kernel: up to 8192 rows, on a
                                 workgroup-per-record kernel (osd_order_blocked_kernel).  Only with QBP_FLAG_OSD_CS or
                                 QBP_FLAG_OSD_E (else QBP_E_INVALID); same results, rule for rule.  On a matrix the
                                 one-wavefront kernel takes it changes nothing */
    QBP_FLAG_RELAY = 512u,    /* qbp_mc_run, _device, _errors, _probs(_device), _weight(_device) only: trials the first-stage
                                 BP (any variant) does not converge on go through Relay-BP (qbp_relay_decode_batch, as
                                 configured by qbp_relay_configure) instead of OSD, then to classification */
    QBP_FLAG_LAYERED = 1024u, /* the layered (check-serial) schedule instead of flooding: qbp_layered_configure below.
                                 Honoured by qbp_decode_batch(_device), qbp_mc_run(_device), qbp_mc_run_errors,
                                 qbp_mc_run_probs(_device), qbp_mc_run_weight(_device) */
    QBP_FLAG_GD = 2048u,      /* qbp_mc_run, _device, _errors, _probs(_device), _weight(_device) only: trials the first
                                 stage (any variant, flooding or QBP_FLAG_LAYERED) does not converge on go through BP
                                 guided decimation (qbp_gd_decode_batch, as configured by qbp_gd_configure), then to
                                 classification */
    QBP_FLAG_LSD = 4096u,     /* the same entries only: those trials go through localized statistics decoding
                                 (qbp_lsd_batch, as configured by qbp_lsd_configure) on the first stage's posterior and
                                 hard decision, then to classification */
    QBP_FLAG_QUANT = 8192u    /* qbp_mc_run, _device, _errors, _probs(_device), _weight(_device) only: the first stage is
                                 fixed-point min-sum (qbp_quant_decode_batch, as configured by qbp_quant_configure below)
                                 instead of double-precision BP */
};
/* The order w of QBP_FLAG_OSD_CS / QBP_FLAG_OSD_E, in bits 16..23 of the flags (a macro: the enum above holds
 * single bits only).  CS: 1 <= w <= 64, E: 1 <= w <= 12. */
#define QBP_OSD_ORDER_FLAGS(w) ((uint32_t)(w) << 16)
#define QBP_MC_OSD_MAX_TRIALS (1 << 20) /* per qbp_mc_run call with QBP_FLAG_OSD0 (record buffers) */

/*
 * Build a decoder for the parity-check matrix H given in CSR form.
 *   row_ptr [m+1], col_idx [E] (ascending within each row, no duplicates), m checks, n variables.
 * Replaces the per-call setup of the reference (csr_matrix(H), mask, adjacency lists:
 * decoding/beliefPropagation.py:12-23 and :93-101), done once per code instead of per syndrome.
 */
int qbp_create(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n,
               int32_t device, qbp_handle** out);
void qbp_destroy(qbp_handle* h);

/*
 * Host-only: what qbp_create would derive from the same CSR arrays, without touching a device
 * (used by the CPU test-suite).  info[8] = {kernel kind (1 on-chip, 2 general-H), DC, DV, max row
 * weight, max column weight, isolated variables, padded (0/1), LDS bytes of one slot}.  When the
 * on-chip kernel applies, the optional outputs receive its tables: tab_var [DC][m] (variable of
 * edge j of check c, -1 = padding), tab_nbr [DC][DV][m] (the column of that variable as edges j'*m + c'
 * in ascending check order, DC*m = no edge; a description of the columns -- where the kernel keeps their
 * messages: qbp_plan_r_layout), tab_writer [m] (bit j: edge
 * (c, j) is the first of its column).
 */
int qbp_plan(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, int32_t info[8],
             int32_t* tab_var, uint16_t* tab_nbr, uint32_t* tab_writer);

/*
 * Host-only: where the on-chip kernel keeps the check->variable messages of a matrix in LDS when a workgroup
 * decodes S syndromes at once (col_order as in qbp_column_order).
 *   - A slot holds one record of DV doubles per variable that has a check.
 *   - A record holds the messages of the variable's column, adjacent and in summation order; its other words
 *     are 0.0 and may stand in front of the messages or behind them.
 *   - Message words of different records never overlap.  Zero words may: a record can begin on the trailing
 *     zeros of the record before it.
 *   - Behind the last slot follow, once per workgroup, an all-zero record and one dump word (written, never read).
 * Outputs (optional), both [DC][m] and relative to the slot, in doubles:
 *   tab_gather  the record of the variable of edge j of check c;
 *   tab_store   that edge's own word inside the record.
 *   A padding edge has info[1] and info[1] + DV: the zero record and the dump word, which the kernel takes
 *   relative to the LAST slot.
 * info[8]:
 *   [0] DV                                   [1] doubles per slot
 *   [2] doubles of one copy of the messages  [3] LDS bytes of a workgroup with one copy (0: S slots do not fit)
 *   [4] LDS bytes with the two copies of the one-barrier forced kernel (0: no such launch at this S)
 *   [5] byte offset of the second copy from the first
 *   [6] byte offset of the first copy in the workgroup's LDS   [7] 0
 * QBP_E_UNSUPPORTED when the matrix does not run on the on-chip kernel.
 */
int qbp_plan_r_layout(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, int32_t col_order,
                      int32_t S, int32_t info[8], uint16_t* tab_gather, uint16_t* tab_store);

/*
 * Host-only: the order in which the kernels add up the check->variable messages of every column
 * (left to right).  col_order 0: ascending check -- np.sum(R, axis=0) on a C-ordered dense R
 * (decoding/beliefPropagation.py:129) adds row by row; col_order 1: the association numpy's pairwise sum
 * gives the column of a Fortran-ordered R (QBP_FLAG_DENSE_F_COLSUM).  Outputs: col_ptr [n+1] and col_edge [E]
 * (CSR edge ids, column by column, in summation order).  QBP_E_UNSUPPORTED when col_order 1 is not a
 * left-to-right sum for some column.
 */
int qbp_column_order(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, int32_t col_order,
                     int32_t* col_ptr, int32_t* col_edge);

/*
 * Decode B syndromes (host buffers).
 *   syndromes [B][m] 0/1 bytes, prior [n] LLRs (initialBelief; +-inf allowed, NaN rejected with
 *   QBP_E_INVALID -- the _device entry points cannot check and clip NaN messages away), max_iter >= 1,
 *   variant QBP_*, alpha / damping / clip_llr as in rework/decoding.py (ignored by
 *   QBP_SUM_PRODUCT; alpha is R-scaling for QBP_DAMPED_SP and the normalisation for QBP_MIN_SUM).
 * Outputs (any may be NULL): hard [B][n] 0/1, converged [B] 0/1, iters [B] (0-based iteration of
 * the first syndrome match, max_iter-1 if none: rework/decoding.py:127,129), llr [B][n].
 * Replaces performBeliefPropagationBatch (decoding/beliefPropagationGPU.py:81-178) and, with
 * B = 1, every single-syndrome entry point listed under the variant enum.
 */
int qbp_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B,
                     int32_t max_iter, int32_t variant, double alpha, double damping,
                     double clip_llr, uint32_t flags, uint8_t* hard, uint8_t* converged,
                     int32_t* iters, double* llr);

/* Same, all pointers are DEVICE pointers, enqueued on `stream` (a hipStream_t, may be NULL),
 * asynchronous.  This is the call bench.py times with inputs resident in HBM. */
int qbp_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior,
                            int64_t B, int32_t max_iter, int32_t variant, double alpha,
                            double damping, double clip_llr, uint32_t flags, uint8_t* d_hard,
                            uint8_t* d_converged, int32_t* d_iters, double* d_llr, void* stream);

/*
 * Check->variable messages after the check update of iteration `iteration` (0-based), for B
 * syndromes: messages [B][E] in CSR edge order (host buffers).  This is the `alpha_estimation=True`
 * return value of the reference, restricted to the edges of H:
 *   QBP_MIN_SUM   rework/decoding.py:58-59   R_new / alpha at iteration 0
 *   QBP_DAMPED_SP rework/decoding.py:168-169 R (before scaling by alpha) at iteration 10
 * (QBP_SUM_PRODUCT: the plain update, i.e. alpha = damping = 1 and no LLR clip whatever is passed.)
 * flags: the column-sum order bits (QBP_FLAG_PAIRWISE_COLSUM / _DENSE_F_COLSUM / _DENSE_F_COLSUM_ITER0) of the
 * iterations before the dump; everything else is ignored.
 */
int qbp_check_messages(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B,
                       int32_t variant, double alpha, double damping, double clip_llr,
                       int32_t iteration, uint32_t flags, double* messages);

/*
 * The two histograms behind the alpha fit of rework/Alvarado.py:10-66 (estimate_alpha_from_code), on
 * the device: the check->variable messages of qbp_check_messages for B syndromes are binned by the
 * true value of the bit they address (errors [B][n] 0/1 bytes: class of message (b, e) =
 * errors[b][col_idx[e]], Alvarado.py:33-36) over their common range (:41-44) into `bins` equal bins
 * with np.histogram's rules (:46-47).  Outputs: edges [bins + 1] (= np.linspace(min, max, bins + 1)),
 * hist0 / hist1 [bins] raw counts.  The density normalisation and the one-parameter fit (:49-62)
 * are a few flops on 2 * bins numbers and stay with the caller (qldpc_amd/alvarado.py).
 * QBP_E_INVALID, with edges, hist0 and hist1 untouched: a null pointer, B = 0, a matrix without edges, bins outside
 * 1 .. 4096, or a message range that is not finite -- ANY message NaN or infinite (a NaN prior entry; min-sum on a
 * check of weight 1): np.histogram raises on that range, no histogram of the remaining messages is returned.
 */
int qbp_message_histograms(qbp_handle* h, const uint8_t* syndromes, const uint8_t* errors,
                           const double* prior, int64_t B, int32_t variant, double alpha,
                           double damping, double clip_llr, int32_t iteration, uint32_t flags, int32_t bins,
                           double* edges, int64_t* hist0, int64_t* hist1);

/*
 * Monte-Carlo trials [trial_begin, trial_end) entirely on the device: sample errors, form
 * syndromes, decode, classify, count.  Replaces the body of the trial loop of
 * paperResults_GPU.py:89-144 (= paperResults.py:57-100) without its OSD call:
 *   generate_errors_and_syndromes_batch (decoding/beliefPropagationGPU.py:181-200), `draws` = 2
 *   reproduces the XOR of two Bernoulli(p) draws (paperResults_GPU.py:96-105);
 *   performBeliefPropagationBatch; residual / logical check / counters (:113-144).
 * Errors come from Philox4x32-10 keyed by (seed, global trial index, qubit): the union of trials
 * is identical however the range is split over GPUs (oracle/bp_oracle.c states the sampler).
 *   Lx [k][n] 0/1 bytes (k <= 64), distance as in codes/<name>.npz, prior [n] (the decoder's
 *   prior is an input, as in the reference, and need not match p).
 * counters[QBP_NUM_COUNTERS] (int64, ADDED to):
 *   [0] trials  [1] logical_error  [2] BPs_fault (always 0, as in the reference)
 *   [3] BPs_miscorrected  [4] incorrectable  [5] degenerateErrors          (:80-84, :133-144)
 *   [6] not_converged (= trials the reference would hand to OSD)  [7] sum of iteration indices
 *   [8] logical_error among not_converged  [9] detection == error exactly
 *   [10] OSD outputs that miss the syndrome (always 0)  [11] reserved (0).
 * Any matrix: those that fit the on-chip kernel (m <= 1024, row weight <= 8, column weight <= 4) run
 * the fused loop, all others the Monte-Carlo mode of the general-H kernel; QBP_FLAG_OSD0 works with
 * both (matrices whose bit-packed rows exceed 64 KiB of LDS go through the workgroup-per-syndrome
 * OSD kernel, whose matrix copy lives in global memory).  With QBP_FLAG_OSD0 a call keeps per-trial
 * records (m + 10 n bytes each): at most QBP_MC_OSD_MAX_TRIALS trials and 16 GiB per call.
 * QBP_FLAG_OSD0 | QBP_FLAG_OSD_CS (or _E) | QBP_OSD_ORDER_FLAGS(w): order-w OSD (qbp_osd_batch) instead of OSD-0,
 * on matrices the one-wavefront OSD kernel takes; with | QBP_FLAG_OSD_LARGE also on every matrix of up to 8192 rows
 * that OSD-0 runs eight pivots at a time on (else QBP_E_UNSUPPORTED).  QBP_E_INVALID: a method bit without
 * QBP_FLAG_OSD0, both method bits, order bits or QBP_FLAG_OSD_LARGE without a method bit, an order out of range.
 */
#define QBP_NUM_COUNTERS 12
int qbp_mc_run(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, double p,
               int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
               const double* prior, int32_t max_iter, int32_t variant, double alpha,
               double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS]);

/* Asynchronous form: d_prior and d_counters (int64[QBP_NUM_COUNTERS], ADDED to) are device
 * pointers; Lx stays a host pointer (uploaded once per handle and cached). */
int qbp_mc_run_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                      double p, int32_t draws, uint64_t seed, int64_t trial_begin,
                      int64_t trial_end, const double* d_prior, int32_t max_iter,
                      int32_t variant, double alpha, double damping, double clip_llr,
                      uint32_t flags, int64_t* d_counters, void* stream);

/*
 * The same pipeline -- syndrome = H e, BP, [OSD-0,] classification, all on the device -- on T GIVEN error
 * patterns (errors [T][n] 0/1 bytes, host) instead of sampled ones.  This is how the reference-pinned fixture of
 * the classification rule (tests/golden/classify.npz: trials sampled and classified by the reference's own
 * paperResults_GPU.py:113-144) is fed through the product path.  With QBP_FLAG_OSD0 at most
 * QBP_MC_OSD_MAX_TRIALS patterns per call.
 */
int qbp_mc_run_errors(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                      int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                      double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS]);

/*
 * OSD-0 post-processing of B decoder outputs: decoding/OSD.py:3-28 performOSD (= OSD_enhanced.py
 * with order 0), any matrix size.  syndromes [B][m], llr [B][n], hard [B][n] -> solution [B][n].  Columns are
 * ordered by ascending |llr|; equal values by ascending column index (np.argsort's order of
 * equal keys is unspecified in the reference).  A syndrome outside the column space of H gets the reference's
 * output too: there it depends on the row swaps of gf2_elimination (OSD.py:56-59); the records whose sweep
 * shows that are recomputed by a kernel that follows the swaps, in a second launch on the same stream.
 */
int qbp_osd0_batch(qbp_handle* h, const uint8_t* syndromes, const double* llr, const uint8_t* hard,
                   int64_t B, uint8_t* solution);
int qbp_osd0_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_llr,
                          const uint8_t* d_hard, int64_t B, uint8_t* d_solution, void* stream);

/*
 * Order-w OSD of B decoder outputs (same buffers as qbp_osd0_batch).  osd_flags: 0 (or QBP_FLAG_OSD0 alone) is
 * exactly qbp_osd0_batch; else QBP_FLAG_OSD_CS or QBP_FLAG_OSD_E with QBP_OSD_ORDER_FLAGS(w) (QBP_FLAG_OSD0 may be
 * set: one encoding serves this call and qbp_mc_run).  Per record:
 *   1. columns sorted by (|llr| as in OSD-0, NaN last, column index) ascending;
 *   2. Gauss-Jordan in that order up to rank(H): pivot columns S, fully reduced matrix A, reduced syndrome s;
 *   3. candidate 0 is OSD-0 (bit-identical to qbp_osd0_batch): e_S = s, e_T = 0, x = hard ^ e;
 *   4. T: the k' = n - rank non-pivot columns in sort order; w' = min(w, k');
 *   5. a candidate flips F within T: e_T = 1_F, e_S(r) = s_r ^ XOR_{j in F} A[r][j].  CS: every weight-1 set
 *      over all of T in order, then the weight-2 sets over T[0..w') in itertools.combinations order.  E: every
 *      non-empty subset of T[0..w'), by weight, then in combinations order.  Candidate index: 0, then that order;
 *   6. cost(x) = sum of fabs(llr_i) over x_i = 1, added in ascending column index from +0.0 in double;
 *   7. the result is the first candidate of least cost; an OSD-0 cost of NaN returns OSD-0, NaN costs never win;
 *   8. a syndrome outside the column space of H returns the OSD-0 output, without a search.
 * Order > 0 on matrices the one-wavefront order-w kernel takes (every code of codes/), else QBP_E_UNSUPPORTED -- unless
 * QBP_FLAG_OSD_LARGE is set: then every other matrix of up to 8192 rows runs on the workgroup-per-record kernel
 * (space-time and detector-error-model matrices; eight pivots at a time, working copy in global memory), also where
 * OSD-0 itself still fits one wavefront, and QBP_E_UNSUPPORTED is left only beyond those (more than 8192 rows,
 * QBP_OPT_OSD_BIG = 2).  Same eight rules, same bits.
 * QBP_E_INVALID for any other bit, QBP_FLAG_OSD_LARGE without a method bit, or an order out of range (CS 1..64,
 * E 1..12: at most 4095 flip sets).
 */
int qbp_osd_batch(qbp_handle* h, uint32_t osd_flags, const uint8_t* syndromes, const double* llr,
                  const uint8_t* hard, int64_t B, uint8_t* solution);
int qbp_osd_batch_device(qbp_handle* h, uint32_t osd_flags, const uint8_t* d_syndromes, const double* d_llr,
                         const uint8_t* d_hard, int64_t B, uint8_t* d_solution, void* stream);

/*
 * qbp_osd_batch with the column order as an input: order [B][n] int32, row b a permutation of 0..n-1, the columns
 * of record b from the least reliable on.  Rule 1 above becomes "columns in the given order" (the |llr| keys and
 * their NaN rule play no part in the order), rule 4 "the non-pivot columns in the given order"; everything else --
 * the cost of rule 6 as the sum of fabs(llr), its NaN rules, the output for syndromes outside the column space,
 * which follows the reference's row swaps in the given order -- stays.  With order[b] = the (|llr|, column) sort the
 * call is qbp_osd_batch bit for bit; with order[b] = what the reference computes, np.argsort(np.abs(llr[b])), OSD-0 is
 * the reference's performOSD also where equal |llr| leave np.argsort's order to the numpy build (the Python drop-in
 * does that under QBP_OSD_NUMPY_ORDER=1: then performOSD is the reference's function on tied inputs wherever the
 * host's numpy is the reference's numpy).  Flags, limits, kernel selection and QBP_E_UNSUPPORTED cases are those of
 * qbp_osd_batch.  The host entry returns QBP_E_INVALID, naming the record, for a null order or a row that is not a
 * permutation, before any GPU work and with `solution` untouched.  The _device entry cannot check d_order (null is
 * QBP_E_INVALID): for any int32 content an entry outside [0, n) is skipped and a repeated column finds no pivot;
 * the output of such a record is unspecified, but nothing is read or written out of bounds.
 */
int qbp_osd_batch_ordered(qbp_handle* h, uint32_t osd_flags, const uint8_t* syndromes, const double* llr,
                          const uint8_t* hard, const int32_t* order, int64_t B, uint8_t* solution);
int qbp_osd_batch_ordered_device(qbp_handle* h, uint32_t osd_flags, const uint8_t* d_syndromes, const double* d_llr,
                                 const uint8_t* d_hard, const int32_t* d_order, int64_t B, uint8_t* d_solution,
                                 void* stream);

/*
 * Relay-BP (Mueller et al. 2025): min-sum whose prior is blended with the previous posterior by a memory strength per
 * variable, run as a chain of legs with different strengths that continue on each other's messages; it stops after a
 * few solutions and keeps the lightest.  No elimination: the alternative to BP + OSD on the codes of codes/ and their
 * space-time matrices.  The reference has no such decoder; the rules below are this build's specification
 * (tests/relay_oracle.py states them in numpy, and the kernel reproduces that statement bit for bit).  With gammas all
 * zero, L = 1 and stop_after = 1 the outputs are those of performMinSum_Symmetric (rework/decoding.py:5-75) with
 * damping = 1.0, `iters` being its currentIter + 1.
 *
 * qbp_relay_configure stores the configuration in the handle (host arrays; uploaded once):
 *   gammas [L][n] memory strengths of leg l (finite, may be negative), leg_iters [L] iterations of leg l (>= 1),
 *   stop_after >= 1 solutions, alpha (min-sum normalisation) and clip_llr as in rework/decoding.py, finite.
 * QBP_E_INVALID: a null pointer, L < 1, a leg_iters[l] < 1, stop_after < 1, anything not finite.  QBP_E_UNSUPPORTED: a
 * matrix whose per-record state -- E messages and three rows of n doubles -- does not fit the 160 KiB of LDS of one
 * workgroup (every code of codes/ and the 864 x 2592 phenomenological matrix fit; 2592 x 7776 does not), unless
 * QBP_OPT_RELAY_MEM allows the other memory layout:
 *
 * Two memory layouts (QBP_OPT_RELAY_MEM, set with qbp_set_option before or after qbp_relay_configure; every launch
 * checks again and refuses, outputs untouched, what its value does not allow):
 *   0 (default)  a record's whole state in LDS: 8 (E + 3 n) bytes + the bookkeeping (+ n in a Monte-Carlo call);
 *   1            the E messages in a per-workgroup global workspace (grid x E doubles, it stays in L2 / Infinity
 *                Cache), the prior and the memory strengths read from global memory; in LDS stay the n posterior
 *                values and the bookkeeping: 8 n bytes + 12 (m / 32) (+ n).  QBP_E_UNSUPPORTED beyond 160 KiB of that:
 *                n of about 20 400, 18 200 in a Monte-Carlo call (2592 x 7776 takes 69 KiB there, the 1008 x 8991
 *                detector error model 79 KiB);
 *   2            automatic: layout 0 where it fits its 160 KiB, else layout 1 (the limit is layout 1's).
 * The outputs do not depend on the layout (same rules, same order of every sum).  QBP_INFO_THREADS, QBP_INFO_GRID and
 * QBP_INFO_LDS_BYTES report the launch.
 *
 * One record (syndrome s, prior P [n] finite):
 *   1. Q = P on the edges, V = P, no best solution, found = 0, total = 0;
 *   2. for leg l = 0 .. L - 1, for t = 0 .. leg_iters[l] - 1:
 *      a. check step of rework/decoding.py:28-56 on Q: signs with 0 -> +1, first minimum by lowest column,
 *         R = alpha * syndrome_sign * r_signs * magnitudes;
 *      b. bias[v] = (1.0 - gammas[l][v]) * P[v] + gammas[l][v] * V[v], every operation rounded on its own;
 *      c. Vn = colsum(R) + bias, the column sum in ascending check order, left to right (QBP_MIN_SUM's default);
 *      d. Q = clip(Vn - R, -clip_llr, clip_llr) on the edges (no damping term);
 *      e. V = Vn, total += 1;
 *      f. hard = V < 0; if H hard == s: w = sum of P[v] over hard[v] = 1, added in ascending v from +0.0; the solution
 *         replaces the best one if there is none yet or w < the best weight (strictly); found += 1; the leg ends;
 *   3. after a leg: stop if found >= stop_after; Q and V carry over into the next leg unchanged, however the leg ended;
 *   4. hard, llr (= V) are those of the best solution, or of the last iteration executed if there is none;
 *      converged = found > 0, iters = total, legs = legs entered, solutions = found.
 * qbp_relay_decode_batch: syndromes [B][m], prior [n] (host entry: a value that is not finite is QBP_E_INVALID) ->
 * hard [B][n], converged [B], iters [B], llr [B][n], legs [B], solutions [B]; any output may be NULL.  QBP_E_INVALID
 * without a configuration.  One workgroup per record, its state in LDS or (layout 1) the messages in global memory
 * (bp_relay_kernel).
 *
 * QBP_FLAG_RELAY in a Monte-Carlo call: the first stage is the call's BP as without the flag; every trial it leaves
 * unconverged is decoded by the rules above from its syndrome and the call's prior (first-stage messages are not
 * carried over) and classified on the result like an OSD output.  counters[10] counts the records Relay leaves without
 * a solution (their hard decision misses the syndrome); [0], [6], [7] are the first stage's.  The record limits of
 * QBP_FLAG_OSD0 apply (QBP_MC_OSD_MAX_TRIALS).  QBP_E_INVALID: together with QBP_FLAG_OSD0 or any OSD bit, or without a
 * configuration.  QBP_E_UNSUPPORTED: in qbp_mc_run_budgets, qbp_mc_run_spectrum, qbp_mc_run_errors_spectrum and
 * qbp_decode_shots, and on matrices qbp_relay_configure refuses under the handle's QBP_OPT_RELAY_MEM (the Monte-Carlo
 * build keeps n more bytes in LDS; the same function chooses the layout).
 */
int qbp_relay_configure(qbp_handle* h, const double* gammas, int32_t L, const int32_t* leg_iters, int32_t stop_after,
                        double alpha, double clip_llr);
int qbp_relay_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, uint8_t* hard,
                           uint8_t* converged, int32_t* iters, double* llr, int32_t* legs, int32_t* solutions);
/* Same, all pointers are DEVICE pointers, enqueued on `stream` (may be NULL), asynchronous. */
int qbp_relay_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                                  uint8_t* d_hard, uint8_t* d_converged, int32_t* d_iters, double* d_llr,
                                  int32_t* d_legs, int32_t* d_solutions, void* stream);

/*
 * Layered (check-serial) BP.  Flooding updates all checks from last iteration's messages, then all variables; here the
 * checks are visited one after another and each sees the posteriors its predecessors of the same iteration just
 * updated.  The reference has no such decoder; the rules below are this build's specification (tests/layered_oracle.py
 * states them in numpy, in the sequential and in the level form, and the kernel reproduces that statement bit for
 * bit).  The row update is the project's own: beliefPropagation.py:114-126 for QBP_SUM_PRODUCT, rework/decoding.py:28-56
 * for QBP_MIN_SUM.
 *
 * One record (syndrome s, prior [n] finite, max_iter >= 1, `order` a permutation of the checks):
 *   state: one check->variable message R per edge, +0.0 at start; the posterior V = prior;
 *   iteration t = 0 .. max_iter - 1, for c in order (checks of weight 0 are skipped):
 *     1. for each edge j of row c in ascending column order: d_j = V[v_j] - R[c,j]; q_j = d_j for QBP_SUM_PRODUCT,
 *        clip(d_j, -clip_llr, clip_llr) for QBP_MIN_SUM;
 *     2. r = the row update of q (sum-product: tanh, sequential product in ascending column order, t_safe, division,
 *        syndrome sign, clip +-0.9999999, 2 arctanh; min-sum: with alpha);
 *     3. R[c,j] = r_j, then V[v_j] = d_j + r_j;
 *   every operation rounded on its own.  After the last check: hard = V < 0; H hard == s: converged at iteration t.
 *   Outputs as qbp_decode_batch: hard and llr = V of the first converged iteration, else of the last; converged;
 *   iters (0-based, max_iter - 1 if none).  Isolated variables keep V = prior.
 * What the kernel runs is the level form: the level of a check is 1 + the largest level of the checks that share a
 * variable with it and come earlier in the order (1 if there are none).  Checks of one level share no variable, and
 * every ordered pair of conflicting checks keeps its order: level after level, all checks of a level at once, is the
 * sequential statement bit for bit.
 *
 * qbp_layered_plan (host only, no device): order_in [m] a permutation of the checks, or NULL for the default order --
 * greedy colouring (checks in ascending index, each the smallest colour no earlier neighbour holds) ordered by (colour,
 * index).  Outputs: order_out [m], the order sorted by level (stable; the default order is its own), level_ptr [m + 1]
 * of which entries 0 .. *n_levels are the level boundaries in order_out (the rest is m).  QBP_E_INVALID: a null
 * pointer, a malformed CSR, an order that is not a permutation.
 *
 * qbp_layered_configure stores the level tables of `order` (host array, NULL = default) in the handle.
 * QBP_E_INVALID: not a permutation.  QBP_E_UNSUPPORTED: a matrix whose per-record state -- E messages, the posterior and
 * the prior -- does not fit the 160 KiB of LDS of one workgroup (864 x 2592 fits; 2592 x 7776 does not), unless
 * QBP_OPT_LAYERED_MEM allows the other memory layout:
 *
 * Two memory layouts (QBP_OPT_LAYERED_MEM, set with qbp_set_option before or after qbp_layered_configure; every call
 * with QBP_FLAG_LAYERED checks again and refuses, host only and outputs untouched, what its value does not allow):
 *   0 (default)  a record's whole state in LDS: per workgroup numpy's tables (counted for both variants at
 *                configuration) and the prior, per slot 8 (E + n) bytes + the bookkeeping: 39 rounds of the [[72,12,6]]
 *                phenomenological matrix (1404 x 4212) fit, 40 do not;
 *   1            the E messages of every slot in a per-workgroup global workspace (grid x S x E doubles, CSR order; a
 *                row's messages are read and written by one thread for the whole launch; it stays in L2 / Infinity
 *                Cache), the prior read from global memory when a slot takes a record; in LDS stay the tables, per
 *                slot the n posterior values, the syndrome bits and the bookkeeping: 8 n + 4 (m / 32) bytes.
 *                QBP_E_UNSUPPORTED beyond 160 KiB of that with one slot: n of about 20 000 (2592 x 7776 takes 64 KiB
 *                there, the 1008 x 8991 detector error model 74 KiB);
 *   2            automatic: layout 0 where a single slot fits its 160 KiB, else layout 1 (the limit is layout 1's).
 * The outputs do not depend on the layout (same rules, same order of every operation).  QBP_OPT_LAYERED_SLOTS and the
 * workgroups per CU follow the layout's own LDS figure; QBP_INFO_THREADS, QBP_INFO_GRID and QBP_INFO_LDS_BYTES report
 * the launch.  Sliding windows (qbp_window_*) take no layered stage in either layout.
 *
 * QBP_FLAG_LAYERED in a call: qbp_decode_batch(_device) decode by the rules above (bp_layered_kernel: one workgroup
 * decodes several records at once, all state in LDS or (layout 1) the messages in global memory;
 * QBP_OPT_LAYERED_SLOTS).  QBP_FLAG_FORCE_FULL runs all iterations
 * and keeps the outputs of the first converged one.  The Monte-Carlo entries run the layered decoder as their first
 * stage on stored errors: qbp_mc_run_errors on the caller's, the sampled entries on the errors
 * qbp_mc_sample_errors[_probs|_weight] return, drawn chunk by chunk (QBP_OPT_MC_WEIGHT_CHUNK) -- counters do not depend
 * on the chunk or on how a trial range is split.  QBP_FLAG_OSD0, the order-w OSD bits and QBP_FLAG_RELAY act on the
 * layered stage's failure records unchanged (llr and hard of the last iteration).  QBP_FLAG_FORCE_FULL changes no
 * count and is dropped there; QBP_FLAG_FAST_MATH is ignored.
 * QBP_E_INVALID: the flag without a configuration, with QBP_DAMPED_SP, with any column-sum order flag (there is no
 * column sum), or a prior that is not finite at a host entry.  QBP_E_UNSUPPORTED: in qbp_mc_run_budgets,
 * qbp_mc_run_spectrum, qbp_mc_run_errors_spectrum, qbp_decode_shots and qbp_check_messages, and on matrices
 * qbp_layered_configure refuses under the handle's QBP_OPT_LAYERED_MEM.
 */
int qbp_layered_plan(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, const int32_t* order_in,
                     int32_t* order_out, int32_t* level_ptr, int32_t* n_levels);
int qbp_layered_configure(qbp_handle* h, const int32_t* order);

/*
 * Fixed-point min-sum BP: messages of q bits, saturating integer arithmetic, what an FPGA or ASIC decoder runs.  The
 * reference has no such decoder; the rules below are this build's specification (tests/quant_oracle.py states them in
 * numpy, and the kernel reproduces that statement bit for bit -- integer sums are exact in any order).
 *
 * qbp_quant_configure stores, per handle: `bits` q, 2 <= q <= 16, with M = 2^(q-1) - 1; `scale`, a finite double > 0,
 * integer units per unit of LLR; the normalisation alpha_num / 2^alpha_shift, 0 <= alpha_shift <= 15 and
 * 1 <= alpha_num <= 2^alpha_shift; the offset beta, 0 <= beta <= M.  QBP_E_INVALID: a parameter out of range.
 * QBP_E_UNSUPPORTED: a column of more than 32767 entries (|V| stays below 2^31), or a matrix whose single-record state
 * -- E messages of 1 byte (q <= 8) or 2, the posterior and the quantised prior as int32 -- does not fit the 160 KiB of
 * LDS of one workgroup.  A later call replaces the configuration.
 *
 * One record (syndrome s, double prior [n], max_iter >= 1):
 *   1. P[v] = 0 if prior[v] is NaN, else clamp(rint(prior[v] * scale), -M, M): one IEEE double multiply, rint rounds
 *      half to even, +-inf clamps to +-M;
 *   2. Q[c,v] = P[v] on every edge;
 *   3. iteration t = 0 .. max_iter - 1, check step, for every edge (c,v):
 *        neg  = s_c XOR (parity of the number of u != v in row c with Q[c,u] < 0; zero counts as positive),
 *        mag  = min over u != v of |Q[c,u]|, M if there is no such u (a row of weight 1),
 *        mag' = max(((mag * alpha_num) >> alpha_shift) - beta, 0),
 *        R[c,v] = neg ? -mag' : mag';
 *   4. variable step: V[v] = P[v] + sum over c of R[c,v], an exact int32 without saturation;
 *      Q[c,v] = clamp(V[v] - R[c,v], -M, M);
 *   5. hard = V < 0; H hard == s: converged at iteration t;
 *   6. outputs: hard and posterior_q = V (int32) of the first converged iteration, else of the last; converged; iters
 *      (0-based, max_iter - 1 if none) as qbp_decode_batch; llr[v] = (double)V[v], an exact conversion without a
 *      division: the LLR in units of 1 / scale, which is what OSD and LSD sort by and add up.  Isolated variables keep
 *      V = P;
 *   7. QBP_FLAG_FORCE_FULL runs all iterations and keeps the outputs of the first converged one.
 *
 * qbp_quant_decode_batch(_device): B records by these rules (bp_quant_kernel: one workgroup decodes several records at
 * once, messages as int8 / int16 and V as int32 in LDS, no FP64 inside the iteration; QBP_OPT_QUANT_SLOTS).  hard is
 * required; converged, iters, posterior_q [B][n] and llr [B][n] may be null.  flags: QBP_FLAG_FORCE_FULL; QBP_FLAG_FAST_MATH
 * is ignored; every other bit is QBP_E_INVALID.  QBP_E_INVALID: no configuration, a NaN prior at the host entry (the
 * device entry applies rule 1).  Outputs do not depend on B, the grid, the slots or the stream.
 *
 * QBP_FLAG_QUANT in qbp_mc_run(_device), qbp_mc_run_errors, qbp_mc_run_probs(_device), qbp_mc_run_weight(_device): the
 * first stage on stored errors -- the caller's, or the errors qbp_mc_sample_errors[_probs|_weight] return, drawn chunk by
 * chunk (QBP_OPT_MC_WEIGHT_CHUNK); counters do not depend on the chunk or on how a trial range is split.  The `prior`
 * argument is quantised by rule 1 (per-column priors of a detector error model included).  QBP_FLAG_OSD0, the order-w
 * OSD bits, QBP_FLAG_RELAY, QBP_FLAG_GD and QBP_FLAG_LSD act on its failure records unchanged, with llr = (double)V and
 * the hard decision of the last iteration (Relay-BP and BPGD start again from the double `prior`).  alpha, damping and
 * clip_llr of the call are ignored, as are QBP_FLAG_FAST_MATH and QBP_FLAG_FORCE_FULL (it cannot change a count).
 * QBP_E_INVALID: the flag without a configuration, with QBP_FLAG_LAYERED, with a variant other than QBP_MIN_SUM, with
 * any column-sum order flag, or a NaN prior at a host entry.  QBP_E_UNSUPPORTED: in qbp_decode_batch(_device),
 * qbp_decode_batch_cond, qbp_mc_run_budgets, qbp_mc_run_spectrum, qbp_mc_run_errors_spectrum, the qbp_mc_run*_llr_hist
 * entries, qbp_decode_shots, qbp_check_messages, and the qbp_window_* and qbp_css_* entries.
 */
int qbp_quant_configure(qbp_handle* h, int32_t bits, double scale, int32_t alpha_num, int32_t alpha_shift, int32_t beta);
int qbp_quant_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, int32_t max_iter,
                           uint32_t flags, uint8_t* hard, uint8_t* converged, int32_t* iters, int32_t* posterior_q,
                           double* llr);
int qbp_quant_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                                  int32_t max_iter, uint32_t flags, uint8_t* d_hard, uint8_t* d_converged,
                                  int32_t* d_iters, int32_t* d_posterior_q, double* d_llr, void* stream);

/*
 * BP guided decimation (BPGD; Yao, Gokduman, Pfister, "Belief propagation decoding of quantum LDPC codes with guided
 * decimation"): flooding BP in rounds of a few iterations; a round that ends without a solution freezes the most
 * reliable variable by overwriting its prior with +-decim_llr, and the next round continues on the same messages.  No
 * elimination and no tables.  The reference has no such decoder; the rules below are this build's specification
 * (tests/gd_oracle.py states them in numpy, and the kernel reproduces that statement bit for bit).  With max_rounds = 0
 * the outputs are those of qbp_decode_batch(max_iter = iters_per_round) -- the plain variant for QBP_SUM_PRODUCT,
 * damping = 1.0 for QBP_MIN_SUM -- `iters` being that call's iters + 1 on converged records and iters_per_round
 * otherwise.
 *
 * qbp_gd_configure stores the configuration in the handle:
 *   iters_per_round T >= 1, max_rounds >= 0, decim_llr > 0 and finite, variant QBP_SUM_PRODUCT or QBP_MIN_SUM, alpha
 *   and clip_llr finite (used by QBP_MIN_SUM only, as in rework/decoding.py).
 * QBP_E_INVALID: a value out of range or not finite, QBP_DAMPED_SP.  QBP_E_UNSUPPORTED: a matrix whose per-record
 * state -- E messages, two rows of n doubles, and numpy's function tables for sum-product -- does not fit the 160 KiB of
 * LDS of one workgroup (every code of codes/ and the 864 x 2592 phenomenological matrix fit; 2592 x 7776 does not),
 * unless QBP_OPT_GD_MEM allows the other memory layout:
 *
 * Two memory layouts (QBP_OPT_GD_MEM, set with qbp_set_option before or after qbp_gd_configure; every launch checks
 * again and refuses, outputs untouched, what its value does not allow):
 *   0 (default)  a record's whole state in LDS: 8 (E + 2 n) bytes + the bookkeeping (+ 3072 for sum-product's tables);
 *   1            the E messages in a per-workgroup global workspace (grid x E doubles, it stays in L2 / Infinity
 *                Cache), the working prior W not stored -- two bits per variable (decimated, sign) and the prior read
 *                from global memory state it --; in LDS stay the n posterior values, the two bit maps and the
 *                bookkeeping: 8 n + n / 4 + 12 (m / 32) bytes (+ 3072).  QBP_E_UNSUPPORTED beyond 160 KiB of that: n of
 *                about 19 800, 19 400 for sum-product (2592 x 7776 takes 64 KiB, 67 KiB for sum-product; the
 *                1008 x 8991 detector error model 73 KiB and 76 KiB);
 *   2            automatic: layout 0 where it fits its 160 KiB, else layout 1 (the limit is layout 1's).
 * The outputs do not depend on the layout (same rules, same order of every sum, every W[v] the same value).
 * QBP_INFO_THREADS, QBP_INFO_GRID and QBP_INFO_LDS_BYTES report the launch.
 *
 * One record (syndrome s, prior P [n] finite):
 *   1. W = P (the working prior), Q = P on the edges, V = P, D = {} (the decimated set), total = 0, rounds = 0;
 *   2. one round, for t = 0 .. T - 1:
 *      1. check step on Q.  QBP_MIN_SUM: rule 2a of Relay-BP above (signs with 0 -> +1, first minimum by lowest column,
 *         R = alpha * syndrome_sign * r_signs * magnitude).  QBP_SUM_PRODUCT: the exact row update of
 *         beliefPropagation.py:114-126 (numpy's tanh, the sequential product in ascending column order, t_safe, the
 *         division, the syndrome sign, the clip at +-0.9999999, 2 arctanh), as flooding and layered BP use it;
 *      2. Vn = colsum(R) + W, the column sum in ascending check order, left to right from the first entry, + W last;
 *      3. on the edges Q = clip(Vn - R, -clip_llr, clip_llr) for QBP_MIN_SUM, Q = Vn - R for QBP_SUM_PRODUCT (no damping
 *         term);
 *      4. V = Vn, total += 1;
 *      5. hard = V < 0; if H hard == s the record has converged and stops;
 *   3. after a round without a solution: stop if rounds == max_rounds.  Otherwise v* is, among the variables not in D,
 *      of column weight >= 1 and with V[v] not NaN, the one with the largest |V[v]|, equal values going to the lowest
 *      variable index; stop if there is none.  W[v*] = -decim_llr if V[v*] < 0, else +decim_llr; v* joins D;
 *      rounds += 1; go to 2 -- Q and V carry over unchanged;
 *   4. hard and llr (= V) are those of the last iteration executed; converged; iters = total; rounds.  Isolated
 *      variables keep V = W = P.
 *   Every floating-point operation is rounded on its own; nothing is fused or reordered.
 * qbp_gd_decode_batch: syndromes [B][m], prior [n] (host entry: a value that is not finite is QBP_E_INVALID) ->
 * hard [B][n], converged [B], iters [B], llr [B][n], rounds [B]; any output may be NULL.  QBP_E_INVALID without a
 * configuration.  One workgroup per record, its state in LDS or (layout 1) the messages in global memory
 * (bp_gd_kernel).
 *
 * QBP_FLAG_GD in a Monte-Carlo call: the first stage is the call's BP as without the flag (any variant, flooding or
 * QBP_FLAG_LAYERED); every trial it leaves unconverged is decoded by the rules above from its syndrome and the call's
 * prior (first-stage messages are not carried over) and classified on the result like an OSD output.  counters[10]
 * counts the records BPGD leaves unsolved (their hard decision misses the syndrome); [0], [6], [7] are the first
 * stage's.  The record limits of QBP_FLAG_OSD0 apply (QBP_MC_OSD_MAX_TRIALS).  QBP_E_INVALID: together with
 * QBP_FLAG_OSD0, any OSD bit or QBP_FLAG_RELAY, or without a configuration.  QBP_E_UNSUPPORTED: in qbp_mc_run_budgets,
 * qbp_mc_run_spectrum, qbp_mc_run_errors_spectrum and qbp_decode_shots, and on matrices qbp_gd_configure refuses under
 * the handle's QBP_OPT_GD_MEM (the same function chooses the layout).
 */
int qbp_gd_configure(qbp_handle* h, int32_t iters_per_round, int32_t max_rounds, double decim_llr, int32_t variant,
                     double alpha, double clip_llr);
int qbp_gd_decode_batch(qbp_handle* h, const uint8_t* syndromes, const double* prior, int64_t B, uint8_t* hard,
                        uint8_t* converged, int32_t* iters, double* llr, int32_t* rounds);
/* Same, all pointers are DEVICE pointers, enqueued on `stream` (may be NULL), asynchronous. */
int qbp_gd_decode_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                               uint8_t* d_hard, uint8_t* d_converged, int32_t* d_iters, double* d_llr, int32_t* d_rounds,
                               void* stream);

/*
 * Localized statistics decoding (BP+LSD; Hillmann, Berent, Di Matteo, Eisert, Wille, Roffe, "Localized statistics
 * decoding: a parallel decoding algorithm for quantum low-density parity-check codes", 2024): a drop-in alternative to
 * OSD-0 with the inputs of qbp_osd_batch.  Clusters grow around the unsatisfied checks in the order of BP's
 * reliabilities; only the small systems inside the clusters are solved, and growth stops as soon as every cluster
 * explains its own syndrome.  The reference has no such decoder; the rules below are this build's specification
 * (tests/lsd_oracle.py states them in numpy, and lsd_kernel reproduces that statement bit for bit).
 *
 * qbp_lsd_configure stores bits_per_step = g >= 0 in the handle (QBP_E_INVALID otherwise).  QBP_E_UNSUPPORTED: a matrix
 * of more than 2048 rows or 65535 columns, or whose per-record state -- the bit-packed rows of [H | syndrome] and the
 * cluster tables -- exceeds the 160 KiB of LDS of one workgroup (the codes of codes/ and 432 x 1296 fit; 864 x 2592
 * does not), unless QBP_OPT_LSD_MEM allows the other memory layout:
 *
 * Two memory layouts (QBP_OPT_LSD_MEM, set with qbp_set_option before or after qbp_lsd_configure; every call checks
 * it again; a value outside 0..2 is QBP_E_INVALID):
 *   0 (default)  lsd_kernel only: one wavefront per record, all m rows and the cluster tables in LDS, the limits above;
 *   1            lsd_large_kernel always: one workgroup of 256 threads per record, the rows in a per-workgroup global
 *                workspace owned by the handle ((W + 1) 32-bit words per check, W = ceil(n / 32), row-major), the
 *                cluster tables alone in LDS.  Only the rows of active checks exist: a row that was never changed equals
 *                its original row of [H | r], and rules 4-6 change a row only while it has a 1 in an active column,
 *                whose checks are all active -- so a check's row is written from the CSR when the check turns active,
 *                and the pivot search and the XORs of rule 6 look at the active checks alone.  The work of a record
 *                scales with its clusters, not with m x n.  Limits: n <= 65535 (rank and column share a 32-bit key)
 *                and lsd_large_lds_bytes(m, n, NP) = 64 + max(8 NP while that fits, 20 m) + 2 NP + 4 n + m bytes,
 *                rounded up to 16 (NP: the power of two >= n), <= 160 KiB -- 2592 x 7776 and 1008 x 8991 fit; m is
 *                bounded by nothing else.  At most two workgroups per CU (the workspace: grid x m x (W + 1) words, plus
 *                the sort keys where they do not fit the LDS -- 650 MB on 2592 x 7776 with 256 CUs);
 *   2            lsd_large_kernel where lsd_kernel is refused (by bytes or by its 2048 rows), lsd_kernel elsewhere.
 * The outputs do not depend on the layout (same rules, same bits).  Refusals are host only, before any GPU work, with
 * the byte count in the message; QBP_INFO_THREADS, QBP_INFO_GRID and QBP_INFO_LDS_BYTES report the launch.
 *
 * One record (syndrome s [m], posterior llr [n], hard decision hard [n]):
 *   1. rank[v] = position of column v in the ascending order of (|llr[v]| by bit pattern, NaN last, v): OSD-0's order;
 *   2. r = s ^ (H hard mod 2); the rows are A = [H | r], all m rows and n columns; no row is a pivot row, no column
 *      is active;
 *   3. every check c with r[c] = 1 is active (a seed);
 *   4. at any time the active checks are the seeds and every check adjacent to an active variable; the clusters are the
 *      connected components of the Tanner graph induced on the active checks and variables (a seed without active
 *      neighbour is a cluster of one check).  A cluster is invalid when it holds a row that is no pivot row and whose
 *      reduced syndrome bit is 1;
 *   5. round t = 1, 2, ... (clusters and validity as at its start): the candidates of an invalid cluster are the
 *      inactive variables adjacent to one of its checks; g = 0: all of them become active; g >= 1: its g candidates of
 *      lowest rank (all, if fewer).  A variable two clusters claim is activated once (the clusters merge); valid
 *      clusters add nothing; a round that activates nothing ends the loop;
 *   6. the columns activated in the round are eliminated in ascending rank, on the same rows: the pivot of column c is
 *      the lowest row that is no pivot row yet and has a 1 in c; without one the column is skipped (it stays active);
 *      otherwise the pivot row is XORed, over the full width and the syndrome bit, into every other row with a 1 in c,
 *      and pivcol[row] = c.  Every activated column is processed;
 *   7. the loop ends when every cluster is valid or nothing more can be activated (at most n rounds);
 *   8. e[pivcol[row]] = reduced syndrome bit of every pivot row, 0 elsewhere; solution = hard ^ e;
 *      stats = {rounds that activated something, active variables, clusters at the end, valid}, valid = 1 iff no cluster
 *      is invalid -- the solution then satisfies s.  With valid = 0 the solution is still the readout above.
 * Row operations never cross clusters, so diag(H1, H2) decodes to the concatenation of the separate solutions; a record
 * with r = 0 returns hard with stats {0, 0, 0, 1}.
 *
 * qbp_lsd_batch: syndromes [B][m], llr [B][n], hard [B][n] -> solution [B][n], stats [B][4] (may be NULL).
 * QBP_E_INVALID without a configuration.  One wavefront per record, all of its state in LDS (lsd_kernel), or the build
 * QBP_OPT_LSD_MEM selects.
 *
 * QBP_FLAG_LSD in a Monte-Carlo call: the first stage is the call's BP as without the flag (any variant, flooding or
 * QBP_FLAG_LAYERED); every trial it leaves unconverged is decoded by the rules above from its syndrome and the first
 * stage's posterior and hard decision, and classified on the result like an OSD output: the counters OSD-0 fills.
 * counters[10] counts the records with valid = 0 (their solution misses the syndrome); [0], [6], [7] are the first
 * stage's.  The second stage is the build QBP_OPT_LSD_MEM selects (QBP_E_UNSUPPORTED where qbp_lsd_configure would
 * refuse under the handle's option).  The record limits of QBP_FLAG_OSD0 apply (QBP_MC_OSD_MAX_TRIALS).
 * QBP_E_INVALID: together with QBP_FLAG_OSD0, any OSD bit, QBP_FLAG_RELAY or QBP_FLAG_GD, or without a configuration.
 * QBP_E_UNSUPPORTED: in qbp_mc_run_budgets, qbp_mc_run_spectrum, qbp_mc_run_errors_spectrum, qbp_decode_shots and the
 * window entries.
 */
int qbp_lsd_configure(qbp_handle* h, int32_t bits_per_step);
int qbp_lsd_batch(qbp_handle* h, const uint8_t* syndromes, const double* llr, const uint8_t* hard, int64_t B,
                  uint8_t* solution, int32_t* stats);
/* Same, all pointers are DEVICE pointers, enqueued on `stream` (may be NULL), asynchronous. */
int qbp_lsd_batch_device(qbp_handle* h, const uint8_t* d_syndromes, const double* d_llr, const uint8_t* d_hard,
                         int64_t B, uint8_t* d_solution, int32_t* d_stats, void* stream);

/* Errors the sampler of qbp_mc_run draws for trials [trial_begin, trial_begin + T):
 * errors [T][n] host bytes.  For tests (compared bit for bit with the oracle's restatement). */
int qbp_mc_sample_errors(qbp_handle* h, double p, int32_t draws, uint64_t seed,
                         int64_t trial_begin, int64_t T, uint8_t* errors);

/*
 * Monte-Carlo on a detector error model: qbp_mc_run with a probability per column (error mechanism) instead of
 * one p.  probs [n] (host; NaN, < 0, > 1 or a null pointer: QBP_E_INVALID before any GPU work).  Trial t,
 * column v: bit = XOR over d < draws of [word v % 4 of Philox4x32-10(counter (t lo, t hi, v / 4, d), key seed)
 * < thr[v]], thr[v] = floor(probs[v] 2^32) clamped to [0, 2^32 - 1] -- with every probs[v] == p exactly the bits
 * of qbp_mc_run(p).  The thresholds are uploaded once per handle and re-uploaded only when probs changes.
 * A column no check touches (an undetectable logical mechanism) is drawn like any other: with Lx it counts as a
 * logical error.  Flags, OSD bits, limits and QBP_E_UNSUPPORTED cases are those of qbp_mc_run.
 */
int qbp_mc_run_probs(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                     int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                     const double* prior, int32_t max_iter, int32_t variant, double alpha,
                     double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form (as qbp_mc_run_device): d_prior and d_counters (ADDED to) are device pointers; Lx and probs
 * stay host pointers. */
int qbp_mc_run_probs_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                            const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                            int64_t trial_end, const double* d_prior, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr,
                            uint32_t flags, int64_t* d_counters, void* stream);
/*
 * Monte-Carlo over a ladder of BP iteration budgets in one pass: the sweep of BP_per_Iteration.py:40-81 (maxIter =
 * 10, 20, ... 90; logical errors, degeneracies and OSD invocations per limit) without sampling and decoding the
 * same trials once per limit.  budgets [n_budgets] (host): 1 <= n_budgets <= QBP_MC_MAX_BUDGETS values >= 1,
 * strictly ascending.  counters is [n_budgets][QBP_NUM_COUNTERS] (ADDED to), and row j equals, digit for digit, what
 * qbp_mc_run_probs adds for the same arguments with max_iter = budgets[j] -- flooding BP does not know its limit,
 * so a trial's state after b iterations of a longer run is the output of a b-iteration run.  One trial whose
 * syndrome is first satisfied in (0-based) iteration k:
 *   rows with budgets[j] > k: converged, k added to [7], classified on the hard decision of iteration k;
 *   rows with budgets[j] <= k: not converged, budgets[j] - 1 added to [7]; what is classified -- or, with
 *   QBP_FLAG_OSD0, handed to OSD -- is the posterior of iteration budgets[j] - 1.
 * The trial stops at min(k, budgets[n_budgets - 1] - 1) (QBP_FLAG_FORCE_FULL: as in qbp_mc_run).  A uniform error
 * rate p is probs filled with p (then the rows are also those of qbp_mc_run(p)).  Kernels of their own checkpoint
 * the running trial (bp_fused_budgets_kernel, bp_generic_budgets_kernel); every matrix qbp_mc_run_probs takes.
 * QBP_E_INVALID, before any GPU work and with the counters untouched: a null pointer, n_budgets out of range, a
 * budget < 1, budgets not strictly ascending, and whatever qbp_mc_run refuses.  Flags, OSD bits and
 * QBP_E_UNSUPPORTED cases are those of qbp_mc_run_probs; with QBP_FLAG_OSD0 the per-trial records are kept per
 * budget, so a call covers at most QBP_MC_OSD_MAX_TRIALS / n_budgets trials (and 16 GiB / n_budgets of records).
 */
#define QBP_MC_MAX_BUDGETS 16
int qbp_mc_run_budgets(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                       int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                       const double* prior, const int32_t* budgets, int32_t n_budgets, int32_t variant,
                       double alpha, double damping, double clip_llr, uint32_t flags, int64_t* counters);
/* Asynchronous form (as qbp_mc_run_probs_device): d_prior and d_counters ([n_budgets][QBP_NUM_COUNTERS], ADDED to)
 * are device pointers; Lx, probs and budgets stay host pointers. */
int qbp_mc_run_budgets_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                              const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                              int64_t trial_end, const double* d_prior, const int32_t* budgets, int32_t n_budgets,
                              int32_t variant, double alpha, double damping, double clip_llr,
                              uint32_t flags, int64_t* d_counters, void* stream);

/*
 * Monte-Carlo with posterior-LLR histograms per iteration budget: qbp_mc_run_budgets -- the same trials, sampler,
 * decoder, OSD and counters [n_budgets][QBP_NUM_COUNTERS], digit for digit -- plus the binned form of the lists
 * BP_per_Iteration.py:46-60, 82-90 (llrs_per_iter, llrs_per_iter_after_OSD) and rework/Alvarado.py:122, 159-162
 * (llr_data[...]["true_0"] / ["true_1"]) collect value by value.
 *   hist [n_budgets][QBP_LLR_HIST_ROWS][bins + 3], int64, ADDED to.  For budget row j let (hard, conv, it, llr) be what
 *   qbp_decode_batch returns for the trial's syndrome with max_iter = budgets[j].  Every one of the trial's n values
 *   llr[v] -- the columns without a check too, whose value is the prior -- adds 1 to
 *       hist[j][2 * !conv + error[v]][col(llr[v])].
 *   The histograms are of BP's output: no OSD bit changes them.
 *   Columns of a row, for edges = np.linspace(llr_lo, llr_hi, bins + 1), which the host computes:
 *       0             x < llr_lo (-inf included)
 *       1 .. bins     the bin np.histogram(x, bins, range=(llr_lo, llr_hi)) puts x in: left-closed, the last bin closed
 *                     on both sides
 *       bins + 1      x > llr_hi (+inf included)
 *       bins + 2      NaN
 *   llrs_per_iter[j] is the sum of the four rows of budget j, llrs_per_iter_after_OSD[j] rows 2 + 3; Alvarado's true_0 /
 *   true_1 are rows 0 + 2 / rows 1 + 3 with one budget.  Identities: sum(hist[j]) = n counters[j][0]; rows 2 + 3 sum to
 *   n counters[j][6]; rows 1 + 3 sum to the total weight of the errors, whatever j.
 * Kernels of their own (bp_fused_llrhist_kernel, bp_generic_llrhist_kernel: the budgets builds, binning every emission
 * into a table the workgroup keeps in LDS as 32-bit counts); every matrix qbp_mc_run_budgets takes.  A count stays
 * below 2^32 because the host launches at most (2^32 - 1) / n trials at a time (QBP_OPT_LLR_HIST_CHUNK lowers that;
 * results do not depend on it).  The table has to fit beside the decoder's state: QBP_LLR_HIST_WORDS(n_budgets, bins)
 * <= QBP_LLR_HIST_MAX_WORDS, which admits 9 budgets x 128 bins, 1 budget x 1024 bins and up to 2045 bins.
 * QBP_E_INVALID, before any GPU work and with both outputs untouched: a null hist, bins < 1, llr_lo or llr_hi not
 * finite or llr_lo >= llr_hi, a table beyond the cap, and whatever qbp_mc_run_budgets refuses.  Flags, OSD bits, the
 * records-per-budget rule and QBP_E_UNSUPPORTED cases are those of qbp_mc_run_budgets.
 */
#define QBP_LLR_HIST_ROWS 4
#define QBP_LLR_HIST_MAX_WORDS 8192
#define QBP_LLR_HIST_WORDS(n_budgets, bins) ((int64_t)(n_budgets) * QBP_LLR_HIST_ROWS * ((int64_t)(bins) + 3))
int qbp_mc_run_llr_hist(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                        int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* prior,
                        const int32_t* budgets, int32_t n_budgets, int32_t variant, double alpha, double damping,
                        double clip_llr, uint32_t flags, double llr_lo, double llr_hi, int32_t bins, int64_t* counters,
                        int64_t* hist);
/* Asynchronous form (as qbp_mc_run_budgets_device): d_prior, d_counters and d_hist are device pointers, both outputs
 * ADDED to; Lx, probs and budgets stay host pointers.  The handle keeps ONE set of edges (and one table of sampler
 * thresholds) on the device, rewritten -- and possibly reallocated -- on the calling stream when a call brings others:
 * calls with different edges or probs on different streams must not be in flight on one handle at the same time. */
int qbp_mc_run_llr_hist_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance, const double* probs,
                               int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                               const double* d_prior, const int32_t* budgets, int32_t n_budgets, int32_t variant,
                               double alpha, double damping, double clip_llr, uint32_t flags, double llr_lo,
                               double llr_hi, int32_t bins, int64_t* d_counters, int64_t* d_hist, void* stream);
/* The same on T GIVEN error patterns (as qbp_mc_run_errors: counters [n_budgets][QBP_NUM_COUNTERS] SET, not added to);
 * hist is ADDED to.  This is how a fixture made by the reference's own loop goes through the product path. */
int qbp_mc_run_errors_llr_hist(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                               int64_t T, const double* prior, const int32_t* budgets, int32_t n_budgets,
                               int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                               double llr_lo, double llr_hi, int32_t bins, int64_t* counters, int64_t* hist);

/*
 * Monte-Carlo with two distributions per call: qbp_mc_run_probs -- the same trials, sampler, decoder, OSD and
 * counters, digit for digit -- plus two tables, both ADDED to like the counters (rework/main.py:65-112,
 * spectrum.py:37-54).
 *   spectrum [QBP_SPECTRUM_ROWS][n + 1].  Per trial: detection = BP's hard decision if BP converged or no OSD flag
 *   is set, else the OSD output; residual = detection ^ error, w = its weight, logical = any(Lx residual), found =
 *   BP's converged flag.  w == 0 adds nothing; otherwise spectrum[row][w] += 1 with
 *     row 0 (weights_found_BP)        found, not logical      row 2 (weights_found_BP_error)   found, logical
 *     row 1 (weights_found_OSD)       not found, not logical  row 3 (weights_found_OSD_error)  not found, logical
 *   -- by `found` alone, never by whether OSD ran or its output is valid (rework/main.py:96-110).  Bins are exact
 *   weights 0 .. n; column 0 stays zero.  spectrum.py's list is row 0 + row 1.
 *   iter_hist [max_iter + 1], may be null: bin k < max_iter counts the trials whose syndrome was first satisfied in
 *   0-based iteration k, bin max_iter those BP did not converge on: sum = [0], last bin = [6],
 *   sum k bin_k + (max_iter - 1) bin_max_iter = [7].
 * Kernels of their own (bp_fused_spectrum_kernel, bp_generic_spectrum_kernel, osd*_spectrum_kernel); every matrix
 * qbp_mc_run_probs takes.  QBP_E_INVALID, before any GPU work and with counters and tables untouched: a null
 * spectrum, max_iter > QBP_MC_SPECTRUM_MAX_ITER (the workgroups keep the iteration histogram on chip), and
 * whatever qbp_mc_run_probs refuses.  Flags, OSD bits, the QBP_MC_OSD_MAX_TRIALS rule and QBP_E_UNSUPPORTED cases
 * are those of qbp_mc_run_probs.
 */
#define QBP_SPECTRUM_ROWS 4
#define QBP_MC_SPECTRUM_MAX_ITER 1024
int qbp_mc_run_spectrum(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                        int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                        const double* prior, int32_t max_iter, int32_t variant, double alpha,
                        double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS],
                        int64_t* spectrum, int64_t* iter_hist);
/* Asynchronous form (as qbp_mc_run_probs_device): d_prior, d_counters, d_spectrum and d_iter_hist (may be null) are
 * device pointers, all three outputs ADDED to; Lx and probs stay host pointers. */
int qbp_mc_run_spectrum_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance,
                               const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                               int64_t trial_end, const double* d_prior, int32_t max_iter,
                               int32_t variant, double alpha, double damping, double clip_llr,
                               uint32_t flags, int64_t* d_counters, int64_t* d_spectrum, int64_t* d_iter_hist,
                               void* stream);
/* The same on T GIVEN error patterns (as qbp_mc_run_errors, whose counters these are: SET, not added to); spectrum
 * and iter_hist are ADDED to.  This is how a fixture made by the reference's own loop goes through the product path. */
int qbp_mc_run_errors_spectrum(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                               int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                               double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS],
                               int64_t* spectrum, int64_t* iter_hist);

/* Errors the sampler of qbp_mc_run_probs draws for trials [trial_begin, trial_begin + T): errors [T][n] host
 * bytes (tests). */
int qbp_mc_sample_errors_probs(qbp_handle* h, const double* probs, int32_t draws, uint64_t seed,
                               int64_t trial_begin, int64_t T, uint8_t* errors);

/*
 * Monte-Carlo on errors of a FIXED weight: every trial's error is a subset of exactly `weight` of the n columns,
 * uniform among the C(n, weight) patterns, instead of n Bernoulli draws.  The failure fractions f_w of a few weights
 * give the logical error rate at every p of uniform noise from one set of runs,
 * LER(p) = sum_w C(n, w) p^w (1 - p)^(n - w) f_w (qldpc_amd/mc.py: run_weights, ler_from_weights), also where it is
 * far below 1 / trials of a Bernoulli run; the reference splits its counters by sum(error) < distance // 2 already
 * (paperResults_GPU.py:140-144).
 * The sampler is this build's own specification, as the Philox Bernoulli sampler of qbp_mc_run is.  For global trial
 * index t, weight w, n columns and seed, start with S empty and run Floyd's subset sampling: for i = 0 .. w - 1
 *   j = n - w + i
 *   r = word i % 4 of Philox4x32-10(counter = (t lo, t hi, i / 4, 2), key = (seed lo, seed hi))
 *   u = (uint64(r) * (j + 1)) >> 32
 *   add j to S if u is already in S, else add u.
 * Counter word 3 is 2: the Bernoulli samplers use 0 and 1 there for their draws, so the streams never coincide.
 * errors[t][v] = 1 iff v in S.  The rows are exactly weight w; they are uniform over subsets up to the multiply-shift
 * bias, at most (j + 1) / 2^32 per step; and they are independent of how [trial_begin, trial_end) is split over calls,
 * chunks or GPUs (tests/weight_oracle.py restates the sampler in numpy).
 * Two stages: a chunk of trials is sampled into a device buffer the handle owns (mc_sample_weight_kernel, one lane per
 * trial), then decoded and classified by the pipeline of qbp_mc_run_errors -- no BP or OSD kernel is built for this.
 * A chunk is QBP_OPT_MC_WEIGHT_CHUNK trials; the default (option 0) is 2^28 / n trials, at least 1 and at most 2^20:
 * a buffer of at most 256 MiB.  The result does not depend on the chunk.
 * counters (ADDED to), flags, OSD bits, the QBP_MC_OSD_MAX_TRIALS rule (for the whole call, not per chunk) and the
 * QBP_E_UNSUPPORTED cases are those of qbp_mc_run.  prior [n] is an input, as there, and fixes the decoder the f_w
 * are measured for; `ew < distance / 2` ([3] against [4]) is evaluated with the actual weight.
 * QBP_E_INVALID, before any GPU work and with the counters untouched: weight < 0 or weight > n, a null prior or
 * counters, trial_begin < 0, trial_end < trial_begin, and whatever qbp_mc_run refuses.
 */
int qbp_mc_run_weight(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, int32_t weight, uint64_t seed,
                      int64_t trial_begin, int64_t trial_end, const double* prior, int32_t max_iter,
                      int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                      int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form (as qbp_mc_run_device): d_prior and d_counters (ADDED to) are device pointers; Lx stays a host
 * pointer.  Every chunk is enqueued on `stream`, in order, on the handle's one buffer. */
int qbp_mc_run_weight_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance, int32_t weight,
                             uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* d_prior,
                             int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                             uint32_t flags, int64_t* d_counters, void* stream);
/* Errors the sampler of qbp_mc_run_weight draws for trials [trial_begin, trial_begin + T): errors [T][n] host
 * bytes (tests). */
int qbp_mc_sample_errors_weight(qbp_handle* h, int32_t weight, uint64_t seed, int64_t trial_begin, int64_t T,
                                uint8_t* errors);

/*
 * EXHAUSTIVE enumeration of the errors of one weight: every pattern of a class instead of a sample of it.  The lowest
 * weights dominate LER(p) at small p and are where sampling works worst (the first non-zero f_w is tiny); their classes
 * are small enough to decode completely -- 59 640 patterns of weight 3 on [[72,12,6]], 17 178 876 of weight 4 on
 * [[144,12,12]] -- which gives f_w exactly and the decoder's real minimum failing weight.
 * The order (this build's specification; qldpc_amd/enumerate.py states it in Python integers): for n columns and weight
 * w, rank r in [0, C(n, w)) is the r-th tuple of itertools.combinations(range(n), w), i.e. lexicographic order of the
 * ascending column tuple.  w = 0 has one pattern, the zero row; w = n has one pattern.  Ranks are int64 and a call is
 * valid only if C(n, w) <= 2^62.  The rank is the trial index: seed-free, and one int64 names a pattern.
 * Unranking: for i = 0 .. w - 1, with lo = previous column + 1 (0 at first), take the smallest column c >= lo for which
 * the remaining rank is below sum_{c' = lo .. c} C(n - 1 - c', w - 1 - i); subtract the sum up to c - 1.  By the
 * hockey-stick identity that is a search on one monotone row of a binomial table: with D = C(n, w) - 1 - r, for
 * t = w .. 1 the largest j below the previous one with C(j, t) <= D, column n - 1 - j, D -= C(j, t).  The host builds
 * C(j, t) for 0 <= j <= n, 0 <= t <= w as uint64, entries above 2^63 - 1 saturated (harmless: every compared value is
 * below 2^62); the handle owns the table and keeps it per (n, w).
 * Two stages as qbp_mc_run_weight: a chunk of QBP_OPT_MC_WEIGHT_CHUNK ranks is written into the same handle buffer
 * (mc_enum_weight_kernel, one lane per pattern, w searches and w byte stores), then decoded and classified by the
 * pipeline of qbp_mc_run_errors.  Everything is as in qbp_mc_run_weight -- counters ADDED to, every flag it takes (OSD-0,
 * order-w OSD, Relay, GD, LSD, layered, fixed-point, the large builds), the QBP_MC_OSD_MAX_TRIALS rule for the whole
 * call -- except that there is no seed and the trial range is the rank range [rank_begin, rank_end).  The result does
 * not depend on the chunk or on how the range is split; [0] of a whole class is C(n, weight).
 * QBP_E_INVALID, before any GPU work and with the outputs untouched: weight outside [0, n], C(n, weight) > 2^62,
 * rank_begin < 0, rank_end < rank_begin, rank_end > C(n, weight), and whatever qbp_mc_run_weight refuses.
 */
int qbp_mc_run_enum(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t distance, int32_t weight, int64_t rank_begin,
                    int64_t rank_end, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                    double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form (as qbp_mc_run_weight_device). */
int qbp_mc_run_enum_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t distance, int32_t weight,
                           int64_t rank_begin, int64_t rank_end, const double* d_prior, int32_t max_iter,
                           int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                           int64_t* d_counters, void* stream);
/* The patterns of ranks [rank_begin, rank_begin + T) as qbp_mc_run_enum fills them: errors [T][n] host bytes (tests). */
int qbp_mc_sample_errors_enum(qbp_handle* h, int32_t weight, int64_t rank_begin, int64_t T, uint8_t* errors);
/* count[0] = C(n, weight).  Host only, no device needed.  QBP_E_INVALID (count untouched): n < 0, weight outside [0, n],
 * C(n, weight) > 2^62. */
int qbp_enum_count(int32_t n, int32_t weight, int64_t* count);

/*
 * WHICH patterns of an enumerated class the decoder fails on.  Per pattern e of ranks [rank_begin, rank_end): s = H e,
 * actual = Lx e; (x, conv) is what qbp_decode_shots computes for s (BP, then the OSD bits of `flags` where BP did not
 * converge); kind = (Lx x != actual) | 2 (!conv).  The pattern is captured when kind & what != 0, what in 1 .. 3
 * (1 logical failures, 2 patterns BP did not converge on, 3 either).
 *   found[0]: the number captured; it may exceed cap.  ranks [cap], kinds [cap] (null allowed with cap = 0): the first
 *   min(found, cap) entries hold captured patterns, sorted by ascending rank when found <= cap; when found > cap which
 *   cap of them are kept, and their order, is unspecified.  Entries beyond min(found, cap) are not written.
 *   counters (ADDED to): those of qbp_decode_shots -- [0], [1], [6], [7], [8], [10].
 * Flags are those qbp_decode_shots accepts (a second stage it does not take: QBP_E_UNSUPPORTED, as there); k in 1 .. 64.
 * Chunk by chunk on the device, nothing returning to the host in between: mc_enum_weight_kernel fills a chunk of
 * QBP_OPT_MC_WEIGHT_CHUNK rows (with OSD at most the records of one qbp_decode_shots call), enum_pack_kernel computes
 * every row's b8 det_bits row and its actual word through the CSR arrays and the Lx columns, the launches of
 * qbp_decode_shots run unchanged, enum_capture_kernel compares and compacts the hits (a ballot per wavefront, one atomic
 * per wavefront, entries past cap dropped).  The result does not depend on the chunk or on how the range is split.
 * QBP_E_INVALID, before any GPU work and with every output untouched: what qbp_mc_run_enum refuses of weight and ranks,
 * what outside 1 .. 3, cap < 0, a null found, null ranks or kinds with cap > 0, and whatever qbp_decode_shots refuses.
 */
int qbp_enum_failures(qbp_handle* h, const uint8_t* Lx, int32_t k, int32_t weight, int64_t rank_begin, int64_t rank_end,
                      const double* prior, int32_t max_iter, int32_t variant, double alpha, double damping,
                      double clip_llr, uint32_t flags, int32_t what, int64_t cap, int64_t* ranks, uint8_t* kinds,
                      int64_t found[1], int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form: device pointers but Lx; the order of the entries is always unspecified; d_found [1] is ADDED to
 * (the caller zeroes it), as d_counters is. */
int qbp_enum_failures_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, int32_t weight, int64_t rank_begin,
                             int64_t rank_end, const double* d_prior, int32_t max_iter, int32_t variant, double alpha,
                             double damping, double clip_llr, uint32_t flags, int32_t what, int64_t cap,
                             int64_t* d_ranks, uint8_t* d_kinds, int64_t* d_found, int64_t* d_counters, void* stream);

/*
 * Monte-Carlo on circuit faults of a FIXED number: every trial has exactly `weight` firing fault SITES of a circuit,
 * uniform among the C(N, weight) site sets, each with one of its K codes, uniform -- the circuit-level counterpart of
 * qbp_mc_run_weight.  When every active site of a circuit fires independently with the same rate p and then takes one
 * of its K codes uniformly (the frame sampler's own model, qbp_frame_sample, with one rate), the number of firing sites
 * is Binomial(N, p), and given w of them the site set and the codes are uniform; so
 * LER(p) = sum_w C(N, w) p^w (1 - p)^(N - w) f_w with N the ACTIVE sites (qldpc_amd/mc.py: run_circuit_weights, and
 * ler_from_weights with n := N).  The strata are sites, not columns of the detector error model: a merged column's
 * probability depends on how many faults of which (class, K) went into it, so column patterns of one weight are not
 * equiprobable.  Propagation is linear: the detectors and observables of a fault set are the XOR of the columns of its
 * faults, so a trial is an error row over the model's columns and everything behind the sampler is the stored-errors
 * pipeline of qbp_mc_run_weight.
 * The fault table (qbp_fault_table_set) names the N active sites -- first_fault [N], the site's first fault in the
 * circuit's fault numbering (faults are numbered by site, then code), and K [N] in {1, 3, 15} -- and maps every fault
 * to a column of H: fault_column [n_faults], -1 for a fault that flips nothing.
 * The sampler (this build's specification; tests/fault_weight_oracle.py restates it in numpy).  For global trial index
 * t, weight w, seed: Philox4x32-10 with the key (lo32(seed), hi32(seed)); counter word 3 is QBP_FAULT_PHILOX_STREAM
 * (streams 0 to 5 are taken, see QBP_DISTANCE_PHILOX_STREAM and QBP_FRAME_PHILOX_STREAM).
 *   Sites, by Floyd's algorithm exactly as qbp_mc_run_weight over N instead of n: for i = 0 .. w - 1
 *     j = N - w + i
 *     r = word i % 4 of the block at counter (lo32(t), hi32(t), i / 4, 6)
 *     u = (uint64(r) * (j + 1)) >> 32
 *     s_i = j if u is one of s_0 .. s_(i-1), else u.
 *   Codes: for i = 0 .. w - 1
 *     r' = word i % 4 of the block at counter (lo32(t), hi32(t), 0x80000000 | i / 4, 6)
 *     c_i = (uint64(r') * K[s_i]) >> 32,  fault f_i = first_fault[s_i] + c_i.
 *   Row: errors[t][v] = parity of the number of i with fault_column[f_i] == v.  Faults mapped to -1 contribute nothing;
 *   two faults in one column cancel, which is the physics.  A row has at most w ones.
 * Rows depend on (t, w, seed, table) only: not on how [trial_begin, trial_end) is split over calls, chunks, streams or
 * GPUs.  Limits: 0 <= w <= min(N, QBP_FAULT_WEIGHT_MAX); N <= 2^32 - 4, the frame simulator's own site limit.
 * Two stages as qbp_mc_run_weight: a chunk of QBP_OPT_MC_WEIGHT_CHUNK trials is sampled into the same handle buffer
 * (mc_sample_fault_weight_kernel, one lane per trial; the lane's sites go to a workspace the handle owns, which is how a
 * step sees the earlier ones), then decoded and classified by the pipeline of qbp_mc_run_errors -- no BP or OSD kernel
 * is built for this.  `ew < distance / 2` is evaluated with the weight of the ROW, which may be below w.
 */
#define QBP_FAULT_PHILOX_STREAM 6
#define QBP_FAULT_WEIGHT_MAX 256
/* Validates on the host, uploads, and keeps the table on the handle; a second call replaces the first, n_sites = 0
 * clears it (the arrays may then be null).  QBP_E_INVALID, with the handle's table as it was: a null array, n_sites < 0
 * or > 2^32 - 4, n_faults < 0, K outside {1, 3, 15}, first_fault[s] < 0 or first_fault[s] + K[s] > n_faults, or a column
 * outside [-1, n). */
int qbp_fault_table_set(qbp_handle* h, int64_t n_sites, const int64_t* first_fault, const uint8_t* K, int64_t n_faults,
                        const int32_t* fault_column);
/* counters (ADDED to), flags, OSD bits, the QBP_MC_OSD_MAX_TRIALS rule and the QBP_E_UNSUPPORTED cases: those of
 * qbp_mc_run_weight, as is every QBP_E_INVALID of it; additionally QBP_E_INVALID, before any GPU work and with the
 * counters untouched, without a table or with weight > min(N, QBP_FAULT_WEIGHT_MAX). */
int qbp_mc_run_fault_weight(qbp_handle* h, const uint8_t* L, int32_t k, int32_t distance, int32_t weight, uint64_t seed,
                            int64_t trial_begin, int64_t trial_end, const double* prior, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                            int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form (as qbp_mc_run_weight_device). */
int qbp_mc_run_fault_weight_device(qbp_handle* h, const uint8_t* L_host, int32_t k, int32_t distance, int32_t weight,
                                   uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* d_prior,
                                   int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                                   uint32_t flags, int64_t* d_counters, void* stream);
/* The rows the sampler of qbp_mc_run_fault_weight fills for trials [trial_begin, trial_begin + T): errors [T][n] host
 * bytes (tests). */
int qbp_mc_sample_errors_fault_weight(qbp_handle* h, int32_t weight, uint64_t seed, int64_t trial_begin, int64_t T,
                                      uint8_t* errors);
/* WHICH trials of a fixed-weight fault run the decoder fails on: qbp_enum_failures with the filler swapped --
 * mc_sample_fault_weight_kernel fills the chunk, then enum_pack_kernel, the launches of qbp_decode_shots and
 * enum_capture_kernel run unchanged.  The captured int64 is the TRIAL INDEX; with the statement above it names the fault
 * set (qldpc_amd/circuit.py: fault_sets).  kinds, what, cap, found, counters, the unwritten entries and the order are as
 * in qbp_enum_failures.  QBP_E_INVALID, before any GPU work and with every output untouched: what
 * qbp_mc_run_fault_weight refuses of the table, weight and trials, and what qbp_enum_failures refuses of the rest. */
int qbp_fault_weight_failures(qbp_handle* h, const uint8_t* L, int32_t k, int32_t weight, uint64_t seed,
                              int64_t trial_begin, int64_t trial_end, const double* prior, int32_t max_iter,
                              int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                              int32_t what, int64_t cap, int64_t* trials, uint8_t* kinds, int64_t found[1],
                              int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form (as qbp_enum_failures_device). */
int qbp_fault_weight_failures_device(qbp_handle* h, const uint8_t* L_host, int32_t k, int32_t weight, uint64_t seed,
                                     int64_t trial_begin, int64_t trial_end, const double* d_prior, int32_t max_iter,
                                     int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                                     int32_t what, int64_t cap, int64_t* d_trials, uint8_t* d_kinds, int64_t* d_found,
                                     int64_t* d_counters, void* stream);

/*
 * Decode T RECORDED shots of a detector error model to observable predictions: the loop of
 * studies/studyComplete.py:91-109 (sampler.sample(shots, separate_observables=True); BP per shot;
 * L_matrix @ prediction % 2 != actual_observables[i]) for data that comes from stim's circuit sampler or from an
 * experiment -- detection events and, if known, the observable flips that really happened; no error pattern.
 *   det_bits [T][ceil(m / 8)]: stim's b8 layout, detector c of shot t is bit c % 8 of byte t * ceil(m / 8) + c / 8;
 *   rows are not padded to words (any alignment), padding bits are ignored.
 *   actual [T] (may be null) and predictions [T] (may be null): bit l = observable l, 1 <= k <= 64; Lx [k][n] 0/1
 *   bytes as in qbp_mc_run.  converged [T] (may be null).
 * One shot: let (hard, conv, it, llr) be what qbp_decode_batch returns for its syndrome with the same prior, max_iter,
 * variant, alpha, damping, clip_llr and the same column-sum and QBP_FLAG_FORCE_FULL bits.  x = hard if conv is set or
 * no OSD flag is; otherwise x = the solution of qbp_osd_batch(OSD bits of flags) on (syndrome, llr, hard).
 * predictions[t] = Lx x mod 2, converged[t] = conv.  Nothing but the shot's bit row is read and nothing but those
 * nine bytes written per shot BP converges on: messages, posteriors and hard decisions stay on chip.
 * counters (ADDED to, indices of qbp_mc_run):
 *   [0] shots  [1] predictions[t] != actual[t]  [6] shots BP did not converge on  [7] sum of `it`
 *   [8] the [1] shots among [6]  [10] shots handed to OSD whose x misses the syndrome (H x != s: a recorded
 *   syndrome need not lie in the column space of H); all others stay 0; with actual == NULL [1] and [8] are untouched.
 * Flags, OSD bits, the QBP_MC_OSD_MAX_TRIALS rule and QBP_E_UNSUPPORTED cases are those of qbp_mc_run.  Kernels of
 * their own (bp_fused_shots_kernel, bp_generic_shots_kernel, osd*_shots_kernel); every matrix qbp_mc_run takes.
 * QBP_E_INVALID, before any GPU work and with every output untouched: a null Lx, det_bits, prior or counters, k
 * outside 1..64, T < 0, a NaN prior (host entry), and whatever qbp_mc_run refuses.  T = 0 succeeds and changes nothing.
 */
int qbp_decode_shots(qbp_handle* h, const uint8_t* Lx, int32_t k, const uint8_t* det_bits, const uint64_t* actual,
                     int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha, double damping,
                     double clip_llr, uint32_t flags, uint64_t* predictions, uint8_t* converged,
                     int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form: Lx stays a host pointer (uploaded once per handle and cached), every other pointer is a device
 * pointer (d_actual, d_predictions, d_converged may be null; d_counters ADDED to), enqueued on `stream`. */
int qbp_decode_shots_device(qbp_handle* h, const uint8_t* Lx_host, int32_t k, const uint8_t* d_det_bits,
                            const uint64_t* d_actual, int64_t T, const double* d_prior, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                            uint64_t* d_predictions, uint8_t* d_converged, int64_t* d_counters, void* stream);

/*
 * Sliding-window decoding of a multi-round matrix (space-time matrices in the style of spaceTime.py, detector error
 * models): instead of one decode of the whole history, overlapping windows of W rounds are decoded one after another,
 * each commits its first F rounds, and the committed correction is folded into the syndrome the later windows see.  The
 * 2592 x 7776 phenomenological matrix of [[288,12,18]] over 18 rounds becomes five 864 x 2592 problems at (W, F) = (6, 3),
 * which the on-chip BP kernel and the one-launch OSD kernels take.  The reference has no such decoder; the rules below are
 * this build's specification (tests/window_oracle.py states them in numpy, and the device path reproduces that statement
 * composed from qbp_decode_batch and qbp_osd_batch bit for bit).
 *
 * Inputs: H [m][n] in CSR form; check_round [m], integers in [0, R) with R = 1 + the largest of them, in any order, not
 * necessarily contiguous, a round may have no check; the window size W >= 1 and the commit size 1 <= F <= W.
 *   var_round[v] = the smallest check_round over column v, 0 for an empty column.
 *   Window k covers rounds [kF, min(kF + W, R)).  The last window is the first k with kF + W >= R (window 0 when
 *   W >= R); there are K = k_last + 1 windows.  For window k:
 *     C_k = the checks whose round lies in the window, ascending;  U_k = the variables whose var_round does, ascending;
 *     H_k = H[C_k, U_k] (column entries in later rounds are cut off);
 *     M_k = {v in U_k : var_round[v] < kF + F}, in the last window all of U_k.  Every variable is in exactly one M_k.
 * One record (syndrome s, prior [n]; only bit 0 of a syndrome byte counts): r = s & 1, x = 0, iters = 0,
 * window_fails = 0; for k = 0 .. K - 1
 *   0. a window without a check or without a variable (a round may have no check) is skipped: nothing is decoded or
 *      counted; for v in M_k -- columns no check touches, the only variables such a window can hold -- x[v] = 0 and
 *      llr_out[v] = prior[v];
 *   1. (hard, conv, it, llr) = qbp_decode_batch(H_k, r[C_k], prior[U_k], max_iter, variant, alpha, damping, clip_llr):
 *      flooding BP, any of the three variants, the default column-sum order;
 *   2. if !conv and OSD bits are set: hard = qbp_osd_batch(H_k, OSD bits)(r[C_k], llr, hard);
 *   3. for v in M_k: x[v] = hard[v], llr_out[v] = llr[v];
 *   4. for every check c of H (also beyond the window): r[c] ^= XOR of x[v] over v in M_k and row c;
 *   5. iters += it, window_fails += !conv.
 * Outputs (any may be NULL): correction [B][n], converged [B] (1 when r == 0 at the end, i.e. H x == s), iters [B],
 * llr [B][n], window_fails [B].  With W >= R and no OSD bits correction, iters and llr are those of qbp_decode_batch on
 * H, bit for bit, and converged is its flag.
 *
 * qbp_window_plan (host only, no device): sizes[3] = {K, sum of |C_k|, sum of |U_k|}; the other outputs may be NULL (call
 * once for the sizes; K <= R, and a check or a variable is in at most ceil(W / F) windows): win_check_ptr [K + 1] into
 * win_checks, win_var_ptr [K + 1] into win_vars, win_commit (0/1 per entry of win_vars), win_class [K] -- windows whose
 * local CSR (H_k in the indices of C_k and U_k) is identical share a class id, numbered in order of first appearance;
 * a skipped window (rule 0) has class -1.
 * QBP_E_INVALID: a null row_ptr, col_idx, check_round or sizes, a malformed CSR, a negative round, W < 1, F outside 1..W,
 * a round of 2^20 or more (rounds need not be contiguous, but K grows with the largest), and windows that hold more than
 * 2^28 checks or variables in all.
 *
 * qbp_window_create builds the decoder: one ordinary qbp_handle per window class (one on a phenomenological matrix, a
 * second if the last window is shorter), the window tables and the rows of H restricted to each M_k on the device, and
 * its batch workspaces.  It is bound to one device and has the thread and stream rules of a handle.  QBP_E_INVALID as
 * qbp_window_plan.
 *
 * qbp_window_decode_batch (host pointers; a NaN prior is QBP_E_INVALID) and qbp_window_decode_batch_device (device
 * pointers, enqueued on `stream`, asynchronous): one call enqueues the whole chain of launches -- per window a gather
 * of the syndrome rows (window_gather_kernel), the sub-handle's BP launch, with OSD bits the list of its failures
 * (window_fail_list_kernel) and the sub-handle's OSD launch on those records only, and the commit of rules 3-5
 * (window_commit_kernel) -- and nothing returns to the host in between.  flags: QBP_FLAG_FORCE_FULL, and the OSD bits as
 * qbp_osd_batch reads them (QBP_FLAG_OSD0 alone: OSD-0; QBP_FLAG_OSD_CS / _E with QBP_OSD_ORDER_FLAGS(w), QBP_FLAG_OSD_LARGE);
 * any other bit is QBP_E_INVALID.  What a sub-handle would refuse (an OSD order its matrix does not take:
 * QBP_E_UNSUPPORTED) is refused before any GPU work, with every output untouched.
 *
 * qbp_window_mc_run_probs(_device): trials [trial_begin, trial_end) drawn by the sampler of qbp_mc_run_probs (the rows of
 * qbp_mc_sample_errors_probs), syndrome = H e (window_syndrome_kernel), the window decoder, classification on the device
 * (window_classify_kernel); chunk by chunk (QBP_OPT_MC_WEIGHT_CHUNK through qbp_window_set_option; default 2^28 / n
 * trials, at most 2^20): counters do not depend on the chunk or on how the range is split.  counters[QBP_NUM_COUNTERS]
 * are ADDED to and mean what qbp_mc_run's mean with detection = correction and "converged" = (window_fails == 0):
 * [6] trials with a window BP did not converge on, [7] the sum of iters, [5] asks H x == s itself, and [10] counts the
 * trials whose correction misses the syndrome.  qbp_window_mc_run_errors: the same pipeline on T stored error patterns
 * (host), counters SET.
 *
 * Out of scope: Relay-BP, BPGD and the layered schedule inside a window (they need per-window configuration), the
 * column-sum order flags, QBP_FLAG_FAST_MATH, budget ladders and spectra, bit-packed shot files (unpack them to bytes),
 * and reading rounds out of a detector error model's coordinates -- the caller supplies check_round.
 */
typedef struct qbp_window qbp_window;
int qbp_window_plan(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, const int32_t* check_round,
                    int32_t W, int32_t F, int32_t sizes[3], int32_t* win_check_ptr, int32_t* win_checks,
                    int32_t* win_var_ptr, int32_t* win_vars, uint8_t* win_commit, int32_t* win_class);
int qbp_window_create(const int32_t* row_ptr, const int32_t* col_idx, int32_t m, int32_t n, const int32_t* check_round,
                      int32_t W, int32_t F, int32_t device, qbp_window** out);
void qbp_window_destroy(qbp_window* w);
int qbp_window_decode_batch(qbp_window* w, const uint8_t* syndromes, const double* prior, int64_t B, int32_t max_iter,
                            int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                            uint8_t* correction, uint8_t* converged, int32_t* iters, double* llr, int32_t* window_fails);
int qbp_window_decode_batch_device(qbp_window* w, const uint8_t* d_syndromes, const double* d_prior, int64_t B,
                                   int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                                   uint32_t flags, uint8_t* d_correction, uint8_t* d_converged, int32_t* d_iters,
                                   double* d_llr, int32_t* d_window_fails, void* stream);
int qbp_window_mc_run_probs(qbp_window* w, const uint8_t* Lx, int32_t k, int32_t distance, const double* probs,
                            int32_t draws, uint64_t seed, int64_t trial_begin, int64_t trial_end, const double* prior,
                            int32_t max_iter, int32_t variant, double alpha, double damping, double clip_llr,
                            uint32_t flags, int64_t counters[QBP_NUM_COUNTERS]);
/* Asynchronous form: d_prior and d_counters (ADDED to) are device pointers; Lx and probs stay host pointers. */
int qbp_window_mc_run_probs_device(qbp_window* w, const uint8_t* Lx_host, int32_t k, int32_t distance,
                                   const double* probs, int32_t draws, uint64_t seed, int64_t trial_begin,
                                   int64_t trial_end, const double* d_prior, int32_t max_iter, int32_t variant,
                                   double alpha, double damping, double clip_llr, uint32_t flags, int64_t* d_counters,
                                   void* stream);
int qbp_window_mc_run_errors(qbp_window* w, const uint8_t* Lx, int32_t k, int32_t distance, const uint8_t* errors,
                             int64_t T, const double* prior, int32_t max_iter, int32_t variant, double alpha,
                             double damping, double clip_llr, uint32_t flags, int64_t counters[QBP_NUM_COUNTERS]);
/* what: QBP_WINDOW_INFO_* below, or a QBP_INFO_* of the sub-handle of window class `index`; -1 if unknown. */
enum { QBP_WINDOW_INFO_WINDOWS = 1, QBP_WINDOW_INFO_CLASSES = 2, QBP_WINDOW_INFO_ROUNDS = 3 };
int64_t qbp_window_get_info(qbp_window* w, int32_t what, int32_t index);
/* QBP_OPT_MC_WEIGHT_CHUNK: trials per chunk of qbp_window_mc_run_* (0 = default); any other option goes to every sub-handle. */
int qbp_window_set_option(qbp_window* w, int32_t option, int64_t value);

/*
 * BP with a prior that differs per record.  Record b decodes syndromes[b] with the prior
 *   prior_b[v] = (sel[b][v] & 1) ? prior1[v] : prior0[v]          (sel [B][n] bytes, only bit 0 counts)
 * and is, bit for bit, qbp_decode_batch on that one syndrome with that prior vector: flooding schedule, QBP_SUM_PRODUCT or
 * QBP_MIN_SUM (alpha the normalisation, clip_llr the clip, damping = 1: there is no damping argument).  Outputs (any may
 * be NULL) have qbp_decode_batch's meaning: hard [B][n], converged [B], iters [B] (0-based iteration of the first
 * syndrome match, max_iter - 1 if none), llr [B][n].  One workgroup per record with the record's whole state in LDS
 * (bp_cond_kernel, qbp_cond.hpp).
 *   QBP_E_INVALID      a null input, a NaN in prior0 or prior1 (host entry; +-inf are legal), max_iter < 1, an unknown
 *                      variant, an OSD bit -- before any GPU work, outputs untouched;
 *   QBP_E_UNSUPPORTED  QBP_DAMPED_SP; a column-sum order flag, QBP_FLAG_LAYERED, _RELAY, _GD, _LSD or _FAST_MATH; a matrix
 *                      whose record state exceeds 160 KiB of LDS (as Relay-BP and BPGD) -- the same;
 *   B = 0 succeeds and changes nothing.  QBP_FLAG_FORCE_FULL is accepted and changes no output.
 */
int qbp_decode_batch_cond(qbp_handle* h, const uint8_t* syndromes, const uint8_t* sel, const double* prior0,
                          const double* prior1, int64_t B, int32_t max_iter, int32_t variant, double alpha,
                          double clip_llr, uint32_t flags, uint8_t* hard, uint8_t* converged, int32_t* iters, double* llr);
/* Same, all pointers are DEVICE pointers, enqueued on `stream`, asynchronous (no NaN check). */
int qbp_decode_batch_cond_device(qbp_handle* h, const uint8_t* d_syndromes, const uint8_t* d_sel, const double* d_prior0,
                                 const double* d_prior1, int64_t B, int32_t max_iter, int32_t variant, double alpha,
                                 double clip_llr, uint32_t flags, uint8_t* d_hard, uint8_t* d_converged, int32_t* d_iters,
                                 double* d_llr, void* stream);

/*
 * Two-stage decoding of a CSS code under Pauli noise (X/Z-correlated BP).  Sector A is the matrix `ha` with the part
 * e_a of the error it detects, sector B the matrix `hb` with e_b; for the codes of codes/: ha = Hx detects Z and Y,
 * hb = Hz detects X and Y, and a Y error flips the qubit's bit in both.  Per trial:
 *   A.  qbp_decode_batch on ha with prior_a; with QBP_FLAG_OSD0 (| a method bit and an order) in `flags` the trials BP
 *       leaves unconverged go through qbp_osd_batch.  x_a = the OSD solution where BP failed and OSD ran, else `hard`.
 *   B.  qbp_decode_batch_cond on hb with sel = x_a, prior0 = prior_b0, prior1 = prior_b1; the same OSD rule gives x_b.
 * For depolarizing noise of strength p (px = py = pz = p / 3) the conditional priors are prior_b0 = log(3 (1 - p) / p)
 * and prior_b1 = log(pz / py) = 0 exactly; prior_b1 = prior_b0 = the marginal of sector B decodes the sectors
 * independently.  variant: QBP_SUM_PRODUCT or QBP_MIN_SUM, for both stages; damping reaches stage A only (stage B has
 * none).  flags: QBP_FLAG_FORCE_FULL and the OSD bits, as in qbp_mc_run.
 *   QBP_E_INVALID      null pointers, NaN priors, probabilities outside [0, 1] or px + py + pz > 1, k outside 0..64;
 *   QBP_E_UNSUPPORTED  QBP_DAMPED_SP, what qbp_decode_batch_cond refuses, and Relay-BP, BPGD, LSD or the layered
 *                      schedule as a stage (out of scope) -- all before any GPU work.
 *
 * qbp_css_create borrows two handles the caller owns (same device, same n, else QBP_E_INVALID); qbp_css_destroy frees
 * the object and leaves them alone.  They must outlive it, and no other call may use them while a qbp_css_* call runs.
 *
 * The sampler: Philox4x32-10 keyed by the seed on the counter (trial lo, trial hi, qubit / 4, QBP_CSS_PHILOX_STREAM),
 * word qubit % 4 = u.  Counter word 3 is the sampler's stream: the Bernoulli draws of qbp_mc_run use 0 and 1, the
 * fixed-weight sampler 2, this one 3.  With t1 = floor(pz 2^32), t2 = floor((pz + px) 2^32), t3 = floor(((pz + px) + py)
 * 2^32), each at most 2^32 - 1: u < t1 is Z, else u < t2 is X, else u < t3 is Y, else no error.  errors_a = Z or Y,
 * errors_b = X or Y, both [T][n] 0/1 bytes.  The rows do not depend on how a trial range is split.
 *
 * Monte-Carlo: counters [3][QBP_NUM_COUNTERS].  Rows 0 and 1 are the sectors, (e_a, x_a, La) and (e_b, x_b, Lb), in
 * qbp_mc_run's layout with the sliding-window decoder's two rules: [5] also counts a correction OSD made valid, [10]
 * counts the corrections that miss their syndrome (without OSD: the unconverged ones).  [6], [7] and [8] follow the BP
 * stage of the sector.  Row 2 is the trial: [0] trials, [1] a logical error in either sector, [6] either BP
 * unconverged, [8] the [1] among the [6], [9] both corrections equal to the errors, [10] either correction misses its
 * syndrome; its other counters are 0.  qbp_css_mc_run ADDS to counters, qbp_css_mc_run_errors SETS them.  A call works
 * in chunks of at most QBP_MC_OSD_MAX_TRIALS trials, each one chain of launches on the stream (sample or copy,
 * syndromes, A, B, classify); counters do not depend on the chunk size (QBP_OPT_MC_WEIGHT_CHUNK through
 * qbp_css_set_option) or on how the range is split.
 */
#define QBP_CSS_PHILOX_STREAM 3
typedef struct qbp_css qbp_css;
int qbp_css_create(qbp_handle* ha, qbp_handle* hb, qbp_css** out);
void qbp_css_destroy(qbp_css* css);
int qbp_css_set_option(qbp_css* css, int32_t option, int64_t value);
int qbp_css_sample_errors(qbp_css* css, double px, double py, double pz, uint64_t seed, int64_t trial_begin, int64_t T,
                          uint8_t* errors_a, uint8_t* errors_b);
/* x_a, x_b [B][n], conv_a, conv_b [B] (the BP stages' converged flags); any output may be NULL. */
int qbp_css_decode_batch(qbp_css* css, const uint8_t* syn_a, const uint8_t* syn_b, int64_t B, const double* prior_a,
                         const double* prior_b0, const double* prior_b1, int32_t max_iter, int32_t variant, double alpha,
                         double damping, double clip_llr, uint32_t flags, uint8_t* x_a, uint8_t* x_b, uint8_t* conv_a,
                         uint8_t* conv_b);
int qbp_css_mc_run(qbp_css* css, const uint8_t* La, int32_t ka, const uint8_t* Lb, int32_t kb, int32_t distance,
                   double px, double py, double pz, uint64_t seed, int64_t trial_begin, int64_t trial_end,
                   const double* prior_a, const double* prior_b0, const double* prior_b1, int32_t max_iter,
                   int32_t variant, double alpha, double damping, double clip_llr, uint32_t flags,
                   int64_t counters[3 * QBP_NUM_COUNTERS]);
int qbp_css_mc_run_errors(qbp_css* css, const uint8_t* La, int32_t ka, const uint8_t* Lb, int32_t kb, int32_t distance,
                          const uint8_t* errors_a, const uint8_t* errors_b, int64_t T, const double* prior_a,
                          const double* prior_b0, const double* prior_b1, int32_t max_iter, int32_t variant, double alpha,
                          double damping, double clip_llr, uint32_t flags, int64_t counters[3 * QBP_NUM_COUNTERS]);

/* ---- Distance upper bound: randomized information-set search over ker H --------------------------------------------
 * QDistRnd's algorithm (Pryadko, Shabashov, Kozin 2022): an upper bound on the weight of the lightest vector of ker H
 * that a row of L detects -- the distance of one sector of a CSS code (H = Hx, L = Lx, or H = Hz, L = Lz), or the weight
 * of the lightest undetectable logical fault of a detector error model (its H and L).  tests/distance_oracle.py states
 * the same rules in numpy; the kernel (qbp_distance.hpp) reproduces them bit for bit.
 *
 * Inputs: H is the handle's matrix [m][n].  G [r][n] 0/1 bytes: every row in ker H, rows may be dependent (a basis of
 * ker H makes the search complete; any subset still gives a valid bound).  L [k][n] 0/1 bytes, 1 <= k <= 64.  A 64-bit
 * seed.  Global trial indices [trial_begin, trial_end).
 *
 * Trial t:
 *   1. Column order.  key[v] = word v & 3 of Philox4x32-10 on the counter (lo32(t), hi32(t), v >> 2,
 *      QBP_DISTANCE_PHILOX_STREAM) with the key (lo32(seed), hi32(seed)).  Counter word 3 is the stream: the Bernoulli
 *      draws use 0 and 1, qbp_mc_run_weight 2, the Pauli sampler 3, this search 4.  The order is the columns sorted
 *      ascending by (key[v], v).
 *   2. Elimination.  Gauss-Jordan on a copy of G, columns in that order: the pivot of a column is the lowest not yet
 *      used row with a 1 in it; if there is none the column is skipped; otherwise the pivot row is XORed into every
 *      other row that has a 1 there and is marked used.  It stops when every row is used or the columns are exhausted.
 *   3. Candidates.  For every row i of the reduced matrix: w_i its weight, lm_i the 64-bit mask whose bit l is
 *      parity(L[l] & row_i).  The row is a candidate when lm_i != 0 (a zero row never is).
 *   4. The trial's result is the candidate with the smallest (w_i, i); without a candidate the trial has no result.
 *
 * Call result: hist [n + 1] is ADDED to: hist[w] += 1 for every trial with a result.  result[4] is SET: the trials run,
 * the smallest w (-1 if no trial had a result), the smallest trial index that reached it (-1), that trial's row i (-1).
 * codeword [n]: that row as 0/1 bytes; logical_mask: its lm.  Either may be NULL; both are untouched when there is no
 * result.  Results do not depend on the grid, the stream or how a range is split: the hist of two adjacent ranges adds
 * up to the hist of their union, and the best of the union is the smaller (w, trial) of the two.
 *
 * Host pointers only; the call synchronises before it returns, like qbp_mc_run.  There is no _device form.  Before any
 * GPU work the library checks through the handle's CSR that every row of G satisfies H g = 0, so the returned weight
 * is a valid upper bound whatever the caller passed.
 * QBP_E_INVALID, with every output untouched: a null h, G, L, result or hist; r < 1; k outside 1..64;
 * trial_end < trial_begin, or more than 2^47 trials in one call; a row of G outside ker H.
 * QBP_E_UNSUPPORTED, before any GPU work and with every output untouched: r > 2048 (a lane tracks its rows in a
 * 32-bit mask, as in the LSD kernel), n > 65535 (16-bit column indices), or a trial state -- the sort keys, 8 bytes
 * for each of the columns rounded up to a power of two, overlaid with the rows, 4 (n / 32 + 1) bytes each, plus two
 * bytes per sorted column -- beyond 160 KiB of LDS.  The bytes are what bounds n in effect: 10 bytes per sorted column
 * let at most 16384 of them fit, so n <= 16384 (with at most 63 rows there: exactly 160 KiB), and the 65535 check never
 * is the one that fires.  There is no global-workspace build.
 * trial_begin == trial_end succeeds with result = {0, -1, -1, -1}.
 * One wavefront per trial, a grid-stride loop over the trials; QBP_OPT_BLOCKS_PER_CU sets the workgroups per CU, and
 * QBP_INFO_THREADS, QBP_INFO_GRID and QBP_INFO_LDS_BYTES report the launch.  G and L are bit-packed once per call into
 * buffers the handle owns.  codeword and logical_mask come from a second launch of one wavefront that repeats the
 * best trial.
 */
#define QBP_DISTANCE_PHILOX_STREAM 4
int qbp_distance_search(qbp_handle* h, const uint8_t* G, int32_t r, const uint8_t* L, int32_t k,
                        uint64_t seed, int64_t trial_begin, int64_t trial_end,
                        int64_t result[4], int64_t* hist, uint8_t* codeword, uint64_t* logical_mask);

/* ---- Circuit-level noise: Pauli-frame simulation of CSS circuits ---------------------------------------------------
 * A circuit of resets, CNOTs and measurements in the Z and X bases with Pauli noise is run for T records at once:
 * sampled shots (qbp_frame_sample) or enumerated single faults (qbp_frame_faults), one propagation, two injectors.
 * The outputs have the layout qbp_decode_shots_device reads: b8 detection rows and uint64 observable masks.
 * tests/circuit_oracle.py states the same rules in numpy; the kernels (qbp_frame.hpp) reproduce them bit for bit.
 *
 * The op table: ops [n_ops][4] int32, one row (kind, q0, q1, rate class) per target or pair, in circuit order; q1 is
 * read for QBP_FRAME_CX and QBP_FRAME_DEP2 only, the rate class for the four noise kinds only.  Measurement rows are
 * numbered 0, 1, ... in table order: the measurement record.  Noise rows are numbered 0, 1, ... in table order: the
 * sites.  Site j has K possible faults with codes 1 .. K: K = 1 for QBP_FRAME_XERR (the Pauli X) and QBP_FRAME_ZERR
 * (the Pauli Z), 3 for QBP_FRAME_DEP1 (code = Pauli: 1 X, 2 Z, 3 Y), 15 for QBP_FRAME_DEP2 (code & 3 is the Pauli on
 * q0, code >> 2 the Pauli on q1).  Faults are numbered by site, then by code: site_base[j] = sum of K over the sites
 * before j.  Detector c is the XOR of the record bits det_idx[det_ptr[c] .. det_ptr[c + 1]), observable l that of
 * obs_idx[obs_ptr[l] .. obs_ptr[l + 1]) (CSR, 32-bit; an index listed twice cancels).
 *
 * One record: X and Z frame bits per qubit, all zero at the start; row after row
 *   QBP_FRAME_RZ / _RX   clear both bits of q0;
 *   QBP_FRAME_CX q0->q1  X[q1] ^= X[q0], then Z[q0] ^= Z[q1];
 *   QBP_FRAME_MZ         the next record bit is X[q0];        QBP_FRAME_MX: the next record bit is Z[q0];
 *   a noise row          if the injector puts a fault with Pauli P on qubit q here: X[q] ^= P & 1, Z[q] ^= P >> 1 & 1.
 * Injectors:
 *   sampling    for site j of shot t, u = word j % 4 of Philox4x32-10 on the counter (lo32(t), hi32(t), j / 4,
 *               QBP_FRAME_PHILOX_STREAM) with the key (lo32(seed), hi32(seed)) -- counter word 3 is the stream, 0 to 4
 *               are taken by the other samplers.  The site faults iff u < thr, thr = floor(rates[class] 2^32), and
 *               then its code is 1 + (u K) / thr in 64-bit integer arithmetic.  rates [n_rates] (host, doubles): a
 *               rate per class; a rate that is negative, >= 1 or NaN is refused, and so is a class >= n_rates.
 *   enumeration record f is fault f: exactly that fault happens, at its site, and nothing else.
 * Outputs, either may be NULL: det_bits [T][ceil(m / 8)], detector c of record t is bit c % 8 of byte
 * t * ceil(m / 8) + c / 8 and the padding bits of a row's last byte are zero; obs [T], bit l = observable l.  Record t
 * of a call is shot shot_begin + t or fault fault_begin + t: the rows do not depend on how a range is split into
 * calls, on begin % 32, on the chunk or on the stream.
 *
 * qbp_frame_create checks the tables, numbers records and sites and uploads them; the handle is bound to one device
 * and has the thread and stream rules of a qbp_handle.  The frame bits [2 nq] and the record bits of 32 records are
 * one 32-bit word each, column `lane` of a global workspace the handle owns; records go through it chunk by chunk
 * (QBP_FRAME_OPT_CHUNK_LANES lanes of 32 records, by default as many as 256 MiB hold, at most 2^20), every chunk one
 * launch of frame_sim_kernel and one of frame_assemble_kernel.  The _device forms take device pointers for det_bits
 * and obs and enqueue on `stream` without synchronising; the host forms synchronise before they return.
 * QBP_E_INVALID, host only, before any GPU work and with every output untouched: a null handle, ops (with
 * n_ops > 0), out, rates, or CSR array (with m > 0 or k > 0 respectively); nq < 1; a kind outside 0 .. 8; a qubit
 * outside [0, nq); a QBP_FRAME_CX or QBP_FRAME_DEP2 row with q0 == q1; a rate class outside
 * [0, QBP_FRAME_MAX_CLASSES); m < 0; a CSR pointer array that does not start at 0 or decreases; a record index outside
 * the measurement record; k outside 0 .. 64; T < 0; shot_begin < 0 or shot_begin + T beyond 2^63 - 1; a fault range
 * outside [0, faults]; a bad rate.  QBP_E_UNSUPPORTED: more than 2^32 - 4 sites or 2^31 - 1 measurements.
 * T = 0 succeeds and changes nothing.
 */
#define QBP_FRAME_PHILOX_STREAM 5
#define QBP_FRAME_MAX_CLASSES 16
enum { QBP_FRAME_RZ = 0, QBP_FRAME_RX = 1, QBP_FRAME_CX = 2, QBP_FRAME_MZ = 3, QBP_FRAME_MX = 4, QBP_FRAME_XERR = 5,
       QBP_FRAME_ZERR = 6, QBP_FRAME_DEP1 = 7, QBP_FRAME_DEP2 = 8 };
enum { QBP_FRAME_INFO_QUBITS = 0, QBP_FRAME_INFO_SITES = 1, QBP_FRAME_INFO_FAULTS = 2, QBP_FRAME_INFO_RECORDS = 3,
       QBP_FRAME_INFO_DETECTORS = 4, QBP_FRAME_INFO_OBSERVABLES = 5,
       QBP_FRAME_INFO_CHUNK_LANES = 6,      /* lanes (of 32 records) a chunk holds at the most */
       QBP_FRAME_INFO_WORKSPACE_BYTES = 7,  /* the workspace as the last call left it */
       QBP_FRAME_INFO_CHUNKS = 8,           /* chunks of the last call */
       QBP_FRAME_INFO_CLASSES = 9 };        /* 1 + the largest rate class of the table */
enum { QBP_FRAME_OPT_CHUNK_LANES = 1 };     /* 0 = default; rounded up to a multiple of 64 (tests force several chunks) */
typedef struct qbp_frame qbp_frame;
int qbp_frame_create(int32_t nq, const int32_t* ops, int64_t n_ops, const int32_t* det_ptr, const int32_t* det_idx,
                     int32_t m, const int32_t* obs_ptr, const int32_t* obs_idx, int32_t k, int32_t device,
                     qbp_frame** out);
void qbp_frame_destroy(qbp_frame* f);
int qbp_frame_sample(qbp_frame* f, const double* rates, int32_t n_rates, uint64_t seed, int64_t shot_begin, int64_t T,
                     uint8_t* det_bits, uint64_t* obs);
int qbp_frame_sample_device(qbp_frame* f, const double* rates, int32_t n_rates, uint64_t seed, int64_t shot_begin,
                            int64_t T, uint8_t* d_det_bits, uint64_t* d_obs, void* stream);
int qbp_frame_faults(qbp_frame* f, int64_t fault_begin, int64_t T, uint8_t* det_bits, uint64_t* obs);
int qbp_frame_faults_device(qbp_frame* f, int64_t fault_begin, int64_t T, uint8_t* d_det_bits, uint64_t* d_obs,
                            void* stream);
int qbp_frame_set_option(qbp_frame* f, int32_t option, int64_t value);
int64_t qbp_frame_get_info(qbp_frame* f, int32_t what);

/* Tuning / introspection. */
enum {
    QBP_OPT_SLOTS_PER_BLOCK = 1, /* syndromes decoded concurrently by one workgroup (0 = auto) */
    QBP_OPT_BLOCKS_PER_CU = 2,   /* persistent workgroups per CU (0 = auto)                    */
    QBP_OPT_FORCE_GENERIC = 4,   /* 1 = use the general-H kernel even where the on-chip one fits */
    QBP_OPT_KERNEL = 5,          /* 0 auto, 1 on-chip, 2 general-H (workgroup per syndrome),
                                    3 streaming (lane per syndrome, messages in HBM)          */
    QBP_OPT_GENERAL_THREADS = 6, /* general-H kernel: threads per workgroup (0 = auto)        */
    QBP_OPT_GENERAL_MEM = 10,          /* general-H kernel, where the messages live: 0 auto (LDS when they fit),
                                          1 global workspace, 2 Q global + half of R in LDS (tests) */
    QBP_OPT_GENERAL_NO_R_SPLIT = 9,    /* 1 = general-H kernel keeps all of R in its global workspace (A/B) */
    QBP_OPT_GENERAL_NO_LDS_TABLES = 8, /* 1 = general-H kernel reads its variable-step tables from L2 (A/B) */
    QBP_OPT_EARLY_EXIT_FULL_WG = 13,  /* 1 = early-exit launches use workgroups of 16 wavefronts like forced ones
                                         (default: two of 8 per CU; A/B) */
    QBP_OPT_NO_FIRST_STEP_TABLE = 12, /* 1 = early-exit launches of the on-chip kernel compute a syndrome's first
                                         check step like every other (default: from a per-workgroup LDS table of
                                         its messages, which depend on the priors and the syndrome bit only; A/B, tests) */
    QBP_OPT_FORCED_TWO_BARRIERS = 11, /* 1 = QBP_FLAG_FORCE_FULL launches keep both barriers of the iteration
                                         (default: one barrier, two copies of the messages in LDS; A/B, tests) */
    QBP_OPT_OSD_BIG = 7,         /* tests: OSD through a workgroup-per-syndrome kernel (matrix in global memory) even
                                    where the one-wavefront kernel fits.  1 = the kernel such matrices get (eight
                                    pivots at a time up to 8192 rows), 2 = the one-pivot-at-a-time kernel (larger
                                    matrices), 3 = as 1 with a first sweep over too few sorted columns, so that
                                    the full-width second sweep runs.  Order w: only with QBP_FLAG_OSD_LARGE and
                                    values 1 or 3, which are one path there (osd_order_blocked_kernel always sweeps
                                    the full width); 2 is QBP_E_UNSUPPORTED */
    QBP_OPT_MC_WEIGHT_CHUNK = 14, /* qbp_mc_run_weight*: trials sampled and decoded per chunk (0 = default, see there;
                                    at most 2^20).  Results do not depend on it (tests force several chunks) */
    QBP_OPT_LAYERED_SLOTS = 15,  /* layered BP: records decoded at once by one workgroup (0 = auto, at most 32; fewer
                                    where the LDS holds fewer).  Results do not depend on it (tests force 1 and 2) */
    QBP_OPT_RELAY_MEM = 16,      /* Relay-BP, where a record's messages live (qbp_relay_configure): 0 LDS only, 1 a global
                                    workspace always (tests reach it on small matrices), 2 automatic.  Results do not
                                    depend on it */
    QBP_OPT_LAYERED_MEM = 17,    /* layered BP, where a record's messages live (qbp_layered_configure): 0 LDS only, 1 a
                                    global workspace always (tests reach it on small matrices), 2 automatic.  Results do
                                    not depend on it */
    QBP_OPT_GD_MEM = 18,         /* BP guided decimation, where a record's messages live (qbp_gd_configure): 0 LDS only, 1 a
                                    global workspace always (tests reach it on small matrices), 2 automatic.  Results do
                                    not depend on it */
    QBP_OPT_LSD_MEM = 19,        /* localized statistics decoding, where a record's rows of [H | syndrome] live
                                    (qbp_lsd_configure): 0 LDS only, 1 a global workspace always (tests reach it on small
                                    matrices), 2 automatic.  Results do not depend on it */
    QBP_OPT_DEBUG_THROW = 99,    /* tests (null handle allowed): raise inside the entry point -- 1 std::bad_alloc
                                    (-> QBP_E_NOMEM), 2 std::runtime_error, 3 a non-standard exception
                                    (-> QBP_E_INVALID): no exception crosses the ABI */
    QBP_OPT_QUANT_SLOTS = 121,   /* fixed-point min-sum: records decoded at once by one workgroup (0 = auto, at most 32;
                                    fewer where the LDS holds fewer).  Results do not depend on it (tests force 1 and 3) */
    QBP_OPT_LLR_HIST_CHUNK = 120, /* tests: qbp_mc_run_llr_hist* launches at most this many trials at a time (0 = default,
                                    the most that keeps the 32-bit counts of a workgroup below 2^32: (2^32 - 1) / n; larger
                                    values mean that too).  Results do not depend on it.  Not 20: tests/test_lsd_large_cpu.py
                                    pins 19 as the last option number below 99, and 100 .. 111 are the QBP_INFO_* values */
    QBP_INFO_M = 100, QBP_INFO_N = 101, QBP_INFO_EDGES = 102, QBP_INFO_MAX_ROW_DEG = 103,
    QBP_INFO_MAX_COL_DEG = 104, QBP_INFO_KERNEL_KIND = 105, /* 1 on-chip, 2 general-H, 3 streaming */
    QBP_INFO_THREADS = 106, QBP_INFO_LDS_BYTES = 107, QBP_INFO_GRID = 108, QBP_INFO_NUM_CU = 109,
    QBP_INFO_LAST_KERNEL = 110, /* kernel of the last decode launch: 1 on-chip, 2 general-H, 3 streaming, 4 layered,
                                   5 fixed-point min-sum */
    QBP_INFO_ONE_BARRIER = 111  /* 1 if the last on-chip launch geometry used the one-barrier forced kernel */
};
int qbp_set_option(qbp_handle* h, int32_t option, int64_t value);
int64_t qbp_get_info(qbp_handle* h, int32_t what);

/* Device evaluation of the kernels' FP64 elementary functions, for tests:
 * kind 0: np.tanh(x * 0.5), 1: 2.0 * np.arctanh(x) as the kernels compute them (numpy's bits: qbp_math.hpp),
 * 2: raw v_rcp_f64(x), 3: div_nr(1, x), 4 / 5: the round-1/2 forms of 0 / 1 (QBP_MATH_FAST builds).
 * Host buffers. */
int qbp_debug_math(qbp_handle* h, int32_t kind, const double* x, double* y, int64_t count);

const char* qbp_last_error(void);
const char* qbp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QBP_H */
