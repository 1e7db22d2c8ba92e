"""Inputs shared by tests/test_quant_large_cpu.py and tests/test_gpu_quant_large.py: the launch arithmetic of
bp_quant_kernel restated in Python (quant_slots and quant_launch of qbp.hip, on quant.lds_bytes -- usable without a GPU),
the matrices that reach what the small ones of quant_cases do not (m > 256 and m > 320, dynamic LDS between 64 and 160
KiB, a column of 300 entries, m > n), their records, and (cached) the statement's outputs on them by its edge-indexed
twin, quant_oracle.decode_batch_edges."""
import functools

import numpy as np

import quant_cases as qc
import quant_oracle as qo
import record_kernel_util as ru
from oracle import oracle
from qldpc_amd import codes, dem, quant

THREADS, MAX_SLOTS = 256, 32
LDS_LIMIT = 160 * 1024
LDS_TWO_PER_CU = 80 * 1024                   # what keeps two workgroups on a CU: the bound of the automatic slots
LDS_DEFAULT = 64 * 1024                      # dynamic LDS a kernel gets without hipFuncSetAttribute
MAX_ITER = 12
Q4, Q6, Q8, Q16 = qc.PARAMS                  # int8 messages: Q4, Q6, Q8; int16: Q16
MC_PARAMS = (Q6, Q16)                        # every Monte-Carlo test runs both instantiations of the Monte-Carlo build
BATCH_PARAMS = {"ph72x9": (Q6, Q8, Q16), "tall": (Q4, Q8, Q16)}     # the sets of the batch tests, per matrix


def wide(params):
    return params[0] > 8


# ---- launch arithmetic (no GPU) ---------------------------------------------------------------------------------------
def lds_bytes(shape, S, is_wide):
    m, n, E = shape
    return quant.lds_bytes(m, n, E, S, is_wide)


def slots(shape, is_wide, B, opt_slots=0):
    """quant_slots: QBP_OPT_QUANT_SLOTS as given, or about four variables per thread and two workgroups per CU; either
    lowered to what fits 160 KiB; never more than the records."""
    S = opt_slots
    if S <= 0:
        S = max(1, min(MAX_SLOTS, 4 * THREADS // max(1, shape[1])))
        while S > 1 and lds_bytes(shape, S, is_wide) > LDS_TWO_PER_CU:
            S -= 1
    while S > 1 and lds_bytes(shape, S, is_wide) > LDS_LIMIT:
        S -= 1
    return max(1, min(S, B))


def geometry(shape, is_wide, B, num_cu, opt_slots=0, blocks_per_cu=0):
    """(slots, grid, lds_bytes) of quant_launch on B records."""
    S = slots(shape, is_wide, B, opt_slots)
    lds = lds_bytes(shape, S, is_wide)
    per_cu = max(1, min(8, LDS_LIMIT // lds))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return S, max(1, min(-(-B // S), num_cu * per_cu)), lds


# ---- the matrices ---------------------------------------------------------------------------------------------------------
TALL_M, TALL_N, TALL_HEAVY, TALL_EMPTY = 300, 96, 0, (50, 95)


def tall_matrix():
    """300 x 96, m > n and m > 256: column 0 stands in every row (300 entries: more than the 256 threads of the
    workgroup, more than M = 127 of int8 messages), columns 50 and 95 are empty, every row has two or three entries
    more (weight 3 or 4) in the other 93 columns, which come to a weight of about 9."""
    rng = np.random.default_rng(96)
    others = np.array([v for v in range(1, TALL_N) if v not in TALL_EMPTY])
    H = np.zeros((TALL_M, TALL_N), np.uint8)
    H[:, TALL_HEAVY] = 1
    for c in range(TALL_M):
        H[c, rng.choice(others, 2 + int(rng.random() < 0.7), replace=False)] = 1
    return H


class Case:
    """A matrix, logical rows, distance, per-column probabilities and B error patterns with their syndromes."""

    def __init__(self, tag, H, L, d, probs, errors):
        self.tag, self.H, self.d, self.probs = tag, H, d, probs
        self.L = np.ascontiguousarray(L, np.uint8)
        self.errors = np.ascontiguousarray(errors, np.uint8)
        self.m, self.n = H.shape
        self.E = int((H != 0).sum())
        self.shape = (self.m, self.n, self.E)
        self.syn = qc.syndromes_of(H, self.errors)

    def prior(self, kind):
        """"uniform": the prior of the mean probability; "noisy": the probabilities' own prior times uniform(0.5, 1.5)
        per variable (record_kernel_util.noisy_prior); "mixed": the noisy one with +-inf, values that clamp at every bit
        width, a half-way value and an exact zero on variables 1 to 6, as quant_cases.case has them."""
        if kind == "uniform":
            p = float(np.mean(self.probs))
            return np.full(self.n, np.log((1 - p) / p))
        prior = ru.noisy_prior(self.probs, self.n, np.random.default_rng(1000 + self.n))
        if kind == "mixed":
            prior[1], prior[2], prior[3], prior[4], prior[5], prior[6] = np.inf, -np.inf, 600.0, -2500.0, 0.0, 1.25
        else:
            assert kind == "noisy"
        return prior


# tag -> (error rates of the quarters of the batch, seed).  Chosen on the statement's output alone, so that the batch
# holds every record class at every parameter set and kind of prior: tests/test_quant_large_cpu.py asserts the counts.
BATCH = 48
RATES = {"ph72x9": ((0.002, 0.006, 0.012, 0.03), 9), "tall": ((0.03, 0.1, 0.2, 0.3), 7)}
TAGS = tuple(RATES)
REFILL_POOL = 192


@functools.lru_cache(maxsize=None)
def case(tag):
    if tag == "refill":
        # quant_cases.matrix("72") with the probabilities of test_gpu_quant.mc_case: small n, so many slots, and a
        # statement that is cheap on many records
        H = qc.matrix("72")
        c = codes.load_code("[[72, 12, 6]]")
        probs = np.where(np.arange(72) % 3 == 0, 0.09, 0.05)
        errors = (np.random.default_rng(41).random((REFILL_POOL, 72)) < probs[None, :] * 1.3).astype(np.uint8)
        return Case(tag, H, np.asarray(c.Lx), c.distance, probs, errors)
    rates, seed = RATES[tag]
    rng = np.random.default_rng(seed)
    if tag == "ph72x9":
        Hs, L, probs = dem.phenomenological("[[72, 12, 6]]", 9, 0.02, 0.02)
        H = np.ascontiguousarray(Hs.toarray(), dtype=np.uint8)
        d = 6
    else:
        H = tall_matrix()
        L = (rng.random((3, TALL_N)) < 0.3).astype(np.uint8)
        probs, d = np.full(TALL_N, 0.05), 4
    n = H.shape[1]
    errors = (rng.random((BATCH, n)) < np.repeat(rates, BATCH // len(rates))[:, None]).astype(np.uint8)
    errors[0] = 0                           # the zero syndrome
    return Case(tag, H, L, d, probs, errors)


def batch_inputs(tag, kind):
    """(syndromes, prior) of the batch tests: under "mixed", variables 2 and 4 (priors -inf and -2500) are in error."""
    c = case(tag)
    if kind != "mixed":
        return c.syn, c.prior(kind)
    errors = c.errors.copy()
    errors[1:, [2, 4]] = 1
    return qc.syndromes_of(c.H, errors), c.prior(kind)


@functools.lru_cache(maxsize=None)
def statement(tag, kind, params, max_iter=MAX_ITER):
    """The statement's five outputs on batch_inputs(tag, kind)."""
    syn, prior = batch_inputs(tag, kind)
    return qo.decode_batch_edges(case(tag).H, syn, prior, max_iter, *params)


@functools.lru_cache(maxsize=None)
def mc_statement(tag, params):
    """The Monte-Carlo runs decode case(tag).errors under the noisy prior: the statement's outputs, and the counters of
    the statement + classification."""
    c = case(tag)
    out = qo.decode_batch_edges(c.H, c.syn, c.prior("noisy"), MAX_ITER, *params)
    return out, classify(c, c.errors, c.syn, out[0], out[1], out[2])


def classify(c, errors, syn, hard, conv, iters):
    return oracle.classify_trials(c.H, c.L, c.d, errors, syn, hard, conv, iters)


def trial_counters(c, errors, syn, detections, conv, iters):
    """oracle.classify_trials trial by trial: int64 [T, 12], whose sum over any rows are the counters of those trials."""
    return np.stack([classify(c, errors[i:i + 1], syn[i:i + 1], detections[i:i + 1], conv[i:i + 1], iters[i:i + 1])
                     for i in range(len(errors))])


def residual_classes(c, out):
    """Of the trials the statement converges: (those with hard != error, those of them with a nonzero logical mask); and
    the trials it never converges."""
    hard, conv = out[0], out[1]
    res = hard ^ c.errors
    wrong = conv & res.any(axis=1)
    logical = wrong & ((res.astype(np.int64) @ c.L.T.astype(np.int64)) % 2).any(axis=1)
    return int(wrong.sum()), int(logical.sum()), int((~conv).sum())
