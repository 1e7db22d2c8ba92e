"""numpy statement of the two-stage CSS decoder (include/qbp.h, qbp_css_*) -- TEST INFRASTRUCTURE, composed from the
CPU oracle's pieces: the Pauli sampler (Philox in numpy, as tests/weight_oracle.py), the conditional prior per record,
the chain (oracle.decode_batch record by record with the record's own prior vector, oracle.osd0 or
tests/osd_order_oracle.py on what BP leaves unconverged) and the three counter rows (oracle.classify_trials per sector
plus the joint row).  Also the hypergraph product of two classical matrices: the Steane matrix with itself, a CSS pair
with irregular columns and k = 16, and with a 4 x 5 chain, a pair whose sectors differ (15 x 47 and 28 x 47, k = 4),
with per-qubit biased priors for it."""
import numpy as np

import osd_order_oracle
from dem_sampler import philox4x32_10, thresholds
from lsd_util import STEANE as STEANE_H
from oracle import oracle

_MASK = np.uint64(0xFFFFFFFF)
PHILOX_STREAM = 3                # counter word 3 (QBP_CSS_PHILOX_STREAM)


def pauli_thresholds(px, py, pz):
    """Cumulative: Z below t1, X below t2, Y below t3 (the sums in this order, in double)."""
    return thresholds([pz, pz + px, (pz + px) + py])


def sample_pauli(n, px, py, pz, seed, trial_begin, T):
    """-> (e_a, e_b) uint8[T, n]: e_a = Z or Y (what Hx detects), e_b = X or Y (what Hz detects)."""
    t1, t2, t3 = pauli_thresholds(px, py, pz)
    n4 = (n + 3) // 4
    t = (np.uint64(trial_begin) + np.arange(T, dtype=np.uint64))[:, None]
    t_lo, t_hi = np.broadcast_to(t & _MASK, (T, n4)), np.broadcast_to(t >> np.uint64(32), (T, n4))
    g = np.broadcast_to(np.arange(n4, dtype=np.uint64)[None, :], (T, n4))
    seed = int(seed)
    words = philox4x32_10((t_lo, t_hi, g, np.full((T, n4), PHILOX_STREAM, np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.stack(words, axis=-1).reshape(T, 4 * n4)[:, :n]
    z = u < t1
    x = ~z & (u < t2)
    y = ~z & ~x & (u < t3)
    return (z | y).astype(np.uint8), (x | y).astype(np.uint8)


def conditional_prior(sel, prior0, prior1):
    """The prior of every record: float64[B, n]."""
    return np.where((np.asarray(sel) & 1).astype(bool), np.asarray(prior1, np.float64)[None, :],
                    np.asarray(prior0, np.float64)[None, :])


def decode_cond(H, syndromes, sel, prior0, prior1, max_iter=50, variant=0, alpha=1.0, clip_llr=20.0):
    """qbp_decode_batch_cond: oracle.decode_batch record by record (damping = 1)."""
    pr = conditional_prior(sel, prior0, prior1)
    outs = [oracle.decode_batch(H, syndromes[b:b + 1], pr[b], max_iter, variant, alpha, 1.0, clip_llr)
            for b in range(len(syndromes))]
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(4))


def _osd(H, syn, llr, hard, conv, osd):
    """osd: None, 0 (OSD-0) or ("cs" | "e", order)."""
    x = np.array(hard, np.uint8)
    if osd is None:
        return x
    for i in np.flatnonzero(~conv):
        x[i] = (oracle.osd0(H, syn[i], llr[i], hard[i]) if osd == 0
                else osd_order_oracle.osd_order(H, syn[i], llr[i], hard[i], osd[1], osd[0]))
    return x


def decode(Hx, Hz, syn_a, syn_b, prior_a, prior_b0, prior_b1, max_iter=50, variant=0, alpha=1.0, damping=1.0, clip_llr=20.0,
           osd=None):
    """The chain -> (x_a, x_b, conv_a, conv_b, it_a, it_b)."""
    hard, conv_a, it_a, llr = oracle.decode_batch(Hx, syn_a, prior_a, max_iter, variant, alpha, damping, clip_llr)
    x_a = _osd(Hx, syn_a, llr, hard, conv_a, osd)
    hard, conv_b, it_b, llr = decode_cond(Hz, syn_b, x_a, prior_b0, prior_b1, max_iter, variant, alpha, clip_llr)
    x_b = _osd(Hz, syn_b, llr, hard, conv_b, osd)
    return x_a, x_b, conv_a, conv_b, it_a, it_b


def _syn(H, e):
    return (e.astype(np.int64) @ np.asarray(H).astype(np.int64).T % 2).astype(np.uint8)


def sector_counters(H, L, distance, errors, x, conv, iters):
    """One sector's row: oracle.classify_trials, and [10] = the corrections that miss their syndrome."""
    s = _syn(H, errors)
    cnt = oracle.classify_trials(H, L, distance, errors, s, x, conv, iters)
    cnt[10] = int((_syn(H, x) != s).any(axis=1).sum())
    return cnt


def counters(Hx, Hz, Lx, Lz, distance, e_a, e_b, prior_a, prior_b0, prior_b1, **kw):
    """qbp_css_mc_run_errors: int64[3, 12]."""
    decoded = decode(Hx, Hz, _syn(Hx, e_a), _syn(Hz, e_b), prior_a, prior_b0, prior_b1, **kw)
    return classify(Hx, Hz, Lx, Lz, distance, e_a, e_b, decoded)


def classify(Hx, Hz, Lx, Lz, distance, e_a, e_b, decoded):
    """The three counter rows of what ``decode`` returned on the syndromes of (e_a, e_b): the decode does not look at
    the logical operators, so one decode serves every (Lx, Lz), k = 0 included."""
    x_a, x_b, conv_a, conv_b, it_a, it_b = decoded
    Lx, Lz = np.asarray(Lx, np.uint8), np.asarray(Lz, np.uint8)
    out = np.zeros((3, 12), np.int64)
    out[0] = sector_counters(Hx, Lx, distance, e_a, x_a, conv_a, it_a)
    out[1] = sector_counters(Hz, Lz, distance, e_b, x_b, conv_b, it_b)
    logical = ((_syn(Lx, x_a ^ e_a).any(axis=1) if len(Lx) else np.zeros(len(e_a), bool)) |
               (_syn(Lz, x_b ^ e_b).any(axis=1) if len(Lz) else np.zeros(len(e_a), bool)))
    unconv = ~conv_a | ~conv_b
    bad = (_syn(Hx, x_a ^ e_a).any(axis=1)) | (_syn(Hz, x_b ^ e_b).any(axis=1))
    exact = (x_a == e_a).all(axis=1) & (x_b == e_b).all(axis=1)
    out[2, 0] = len(e_a)
    out[2, 1] = logical.sum()
    out[2, 6] = unconv.sum()
    out[2, 8] = (logical & unconv).sum()
    out[2, 9] = exact.sum()
    out[2, 10] = bad.sum()
    return out


# ---- GF(2) helpers and the hypergraph product -------------------------------------------------------------------------
def gf2_rref(A):
    """-> (reduced rows uint8, pivot columns)."""
    A = np.array(A, np.uint8) & 1
    piv, r = [], 0
    for c in range(A.shape[1]):
        rows = np.flatnonzero(A[r:, c]) + r
        if rows.size == 0:
            continue
        A[[r, rows[0]]] = A[[rows[0], r]]
        for i in np.flatnonzero(A[:, c]):
            if i != r:
                A[i] ^= A[r]
        piv.append(c)
        r += 1
        if r == A.shape[0]:
            break
    return A[:r], piv


def gf2_rank(A):
    return len(gf2_rref(A)[1])


def gf2_kernel(A):
    """A basis of {v : A v = 0}, uint8[n - rank, n]."""
    R, piv = gf2_rref(A)
    n = np.asarray(A).shape[1]
    free = [c for c in range(n) if c not in piv]
    K = np.zeros((len(free), n), np.uint8)
    for i, f in enumerate(free):
        K[i, f] = 1
        for r, p in enumerate(piv):
            K[i, p] = R[r, f]
    return K


def logicals(H_commute, H_stab):
    """Representatives of ker(H_commute) / rowspace(H_stab), by elimination: the kernel vectors that stay independent
    of the stabilizers (and of each other)."""
    out = []
    basis = np.array(H_stab, np.uint8) & 1
    rank = gf2_rank(basis)
    for v in gf2_kernel(H_commute):
        cand = np.vstack([basis, v[None, :]])
        if gf2_rank(cand) > rank:
            basis, rank = cand, rank + 1
            out.append(v)
    return np.array(out, np.uint8).reshape(len(out), np.asarray(H_stab).shape[1])


CHAIN = np.array([[1, 1, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 1, 1]], np.uint8)    # 4 x 5, full rank


def hgp(H1, H2):
    """Hypergraph product of two classical matrices H1 (r1 x n1) and H2 (r2 x n2) -> (Hx, Hz, Lx, Lz) on
    n1 n2 + r1 r2 qubits: Hx = [H1 (x) I_n2 | I_r1 (x) H2^T] with r1 n2 rows, Hz = [I_n1 (x) H2 | H1^T (x) I_r2] with
    n1 r2 rows.  Hx Lz^T = Hz Lx^T = Hx Hz^T = 0.  With H1 != H2 the two sectors differ in shape and weights."""
    H1, H2 = np.asarray(H1, np.uint8), np.asarray(H2, np.uint8)
    (r1, n1), (r2, n2) = H1.shape, H2.shape
    eye = lambda k: np.eye(k, dtype=np.uint8)
    Hx = np.hstack([np.kron(H1, eye(n2)), np.kron(eye(r1), H2.T)]) & 1
    Hz = np.hstack([np.kron(eye(n1), H2), np.kron(H1.T, eye(r2))]) & 1
    Lx = logicals(Hz, Hx)          # X-type logicals commute with the Z checks; sector A's residuals live here
    Lz = logicals(Hx, Hz)
    return Hx.astype(np.uint8), Hz.astype(np.uint8), Lx, Lz


def hgp_steane():
    """Hypergraph product of STEANE_H (3 x 7) with itself -> (Hx 21 x 58, Hz 21 x 58, Lx 16 x 58, Lz 16 x 58): the
    [[58, 16, 3]] code; column weights 2 to 6 in both matrices."""
    return hgp(STEANE_H, STEANE_H)


def hgp_asymmetric(tag):
    """The two orientations of STEANE_H (3 x 7) x CHAIN (4 x 5), n = 47, k = 4: "wide_a" -> Hx 15 x 47 (column weights
    1 .. 3, rows up to 6), Hz 28 x 47 (columns 1 .. 4, rows up to 5); "wide_b" -> the shapes exchanged."""
    return hgp(STEANE_H, CHAIN) if tag == "wide_a" else hgp(CHAIN, STEANE_H)


def biased_priors(n, seed=7):
    """Per-qubit, biased Pauli rates and their three prior vectors (the formulas of qldpc_amd.css.pauli_priors,
    per qubit): -> (prior_a, prior_b0, prior_b1) float64[n].  px ~ 0.02, py ~ 0.015, pz ~ 0.03, each spread over the
    qubits, so no vector is constant, pz != py and prior_b1 = log(pz / py) takes both signs."""
    rng = np.random.default_rng(seed)
    px = 0.02 * rng.uniform(0.8, 1.25, n)
    py = 0.015 * rng.uniform(0.5, 2.0, n)
    pz = 0.03 * rng.uniform(0.8, 1.25, n)
    return np.log((1 - py - pz) / (py + pz)), np.log((1 - px - py - pz) / px), np.log(pz / py)


BIASED_RATES = (0.02, 0.015, 0.03)       # the sampler's scalar (px, py, pz) that go with biased_priors


# ---- the inputs of tests/test_gpu_css_shapes.py, and their statement computed once -----------------------------------
# The sampler takes scalar rates and the priors are per qubit: mismatched on purpose, a decoder is under test and not
# a logical error rate.  Unconverged trials of the 2000 on the statement (row 0 / row 1, [6]), sum-product: wide_a
# 699 / 19 to 25 (with the OSD mode: sector B's prior follows sector A's correction), wide_b 34 / 372 to 379; min-sum
# (alpha 0.8): wide_a 401 / 64 to 66, wide_b 114 / 412 to 415.  tests/test_css_cpu.py asserts the five of each.
ASYM_T, ASYM_B, ASYM_MAX_ITER, ASYM_DISTANCE = 2000, 200, 30, 3
ASYM_SEED, ASYM_BEGIN = (9 << 32) + 5, (1 << 32) - 100           # the trial indices cross 2^32
MIN_SUM = 2                                                      # QBP_MIN_SUM
ASYM_MODES = {"none": dict(osd=None), "osd0": dict(osd=0), "cs7": dict(osd=("cs", 7)),
              "minsum": dict(osd=None, variant=MIN_SUM, alpha=0.8), "minsum_osd0": dict(osd=0, variant=MIN_SUM, alpha=0.8)}
_ASYM = {}


def asym_inputs(tag):
    """"wide_a" / "wide_b" -> the code, ASYM_T errors and the biased priors (shared: do not write to them)."""
    if tag not in _ASYM:
        Hx, Hz, Lx, Lz = hgp_asymmetric(tag)
        n = Hx.shape[1]
        ea, eb = sample_pauli(n, *BIASED_RATES, ASYM_SEED, ASYM_BEGIN, ASYM_T)
        for a in (Hx, Hz, Lx, Lz, ea, eb):
            a.setflags(write=False)
        _ASYM[tag] = dict(Hx=Hx, Hz=Hz, Lx=Lx, Lz=Lz, d=ASYM_DISTANCE, n=n, ea=ea, eb=eb, priors=biased_priors(n))
    return _ASYM[tag]


def asym_decoded(tag, mode):
    """``decode`` on the syndromes of the ASYM_T errors, once per (tag, mode)."""
    s = asym_inputs(tag)
    if ("decoded", mode) not in s:
        s["decoded", mode] = decode(s["Hx"], s["Hz"], _syn(s["Hx"], s["ea"]), _syn(s["Hz"], s["eb"]), *s["priors"],
                                    max_iter=ASYM_MAX_ITER, **ASYM_MODES[mode])
    return s["decoded", mode]


def asym_statement(tag, mode, Lx=None, Lz=None):
    """The counters [3][12] of the ASYM_T trials (a fresh array), with other logical operators if given."""
    s = asym_inputs(tag)
    return classify(s["Hx"], s["Hz"], s["Lx"] if Lx is None else Lx, s["Lz"] if Lz is None else Lz, s["d"], s["ea"],
                    s["eb"], asym_decoded(tag, mode))


def asym_batch_syndromes(s):
    """The syndromes of the first ASYM_B errors, every 13th of sector A and every 17th of sector B with a fifth of its
    bits flipped: any syndrome is legal for a decode call, and these leave BP unconverged."""
    rng = np.random.default_rng(4)
    syn_a, syn_b = _syn(s["Hx"], s["ea"][:ASYM_B]), _syn(s["Hz"], s["eb"][:ASYM_B])
    syn_b[::17] ^= (rng.random(syn_b[::17].shape) < 0.2).astype(np.uint8)
    syn_a[::13] ^= (rng.random(syn_a[::13].shape) < 0.2).astype(np.uint8)
    return syn_a, syn_b
