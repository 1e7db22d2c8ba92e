"""Inputs shared by tests/test_quant_cpu.py and tests/test_gpu_quant.py: the parameter sets, the matrices, the records
and (cached) the statement's outputs on them."""
import functools

import numpy as np

import layered_oracle as lo
import quant_oracle as qo

# (bits, scale, alpha_num, alpha_shift, beta)
PARAMS = [(4, 1.0, 3, 2, 0), (6, 2.0, 13, 4, 0), (8, 8.0, 1, 0, 2), (16, 64.0, 7, 3, 0)]
MATRICES = ["steane", "72", "72zero", "irr37", "disjoint70", "rows", "144"]
MAX_ITERS = (1, 2, 30)


def rows_matrix():
    """12 x 30: a row of weight 1 (row 0), a row of weight 0 (row 1), a row of weight 14 (row 2), the rest of weight
    3 to 5; column 29 is isolated."""
    rng = np.random.default_rng(12)
    H = np.zeros((12, 30), np.uint8)
    H[0, 4] = 1
    H[2, rng.choice(29, 14, replace=False)] = 1
    for c in range(3, 12):
        H[c, rng.choice(29, int(rng.integers(3, 6)), replace=False)] = 1
    assert H[0].sum() == 1 and H[1].sum() == 0 and H[2].sum() >= 12 and H[:, 29].sum() == 0
    return H


def matrix(name):
    if name == "72zero":
        H = lo.matrix("72").copy()
        H[:, [7, 40]] = 0                   # two zero columns: isolated variables keep V = P
        return H
    if name == "rows":
        return rows_matrix()
    return lo.matrix(name)


def syndromes_of(H, errors):
    return (errors.astype(np.int64) @ np.asarray(H).T.astype(np.int64) % 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def issue_case():
    """The records of the issue: [[72,12,6]] Hx, 40 Bernoulli(0.08) errors from default_rng(5), the prior of p = 0.08."""
    H = lo.matrix("72")
    errors = (np.random.default_rng(5).random((40, 72)) < 0.08).astype(np.uint8)
    return H, errors, syndromes_of(H, errors), np.full(72, np.log(0.92 / 0.08))


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(H, errors, syndromes, prior).  kind "uniform": the prior of p = 0.08; "mixed": a prior per variable with +-inf,
    values that clamp at every bit width of PARAMS, a half-way value and an exact zero."""
    H = matrix(name)
    n = H.shape[1]
    rng = np.random.default_rng(300 + n + len(name))
    B = 24 if n > 100 else 32
    errors = (rng.random((B, n)) < np.repeat([0.02, 0.06, 0.1, 0.16], B // 4)[:, None]).astype(np.uint8)
    errors[0] = 0                           # the zero syndrome
    if kind == "mixed":
        errors[:, [1 % n, 3 % n]] = 1       # (the variables whose prior says "1": -inf and -2500)
    syn = syndromes_of(H, errors)
    if name == "rows":
        syn[3, 1] = 1                       # an unsatisfiable empty check
    if kind == "uniform":
        prior = np.full(n, np.log(0.92 / 0.08))
    else:
        prior = np.log(0.92 / 0.08) * rng.uniform(0.3, 1.7, n)
        prior[0], prior[1 % n], prior[2 % n] = np.inf, -np.inf, 600.0
        prior[3 % n], prior[4 % n], prior[5 % n] = -2500.0, 0.0, 1.25
    return H, errors, syn, prior


@functools.lru_cache(maxsize=None)
def statement(name, kind, params, max_iter):
    H, _, syn, prior = case(name, kind)
    return qo.decode_batch(H, syn, prior, max_iter, *params)


def classes(conv, iters):
    """(converged at iteration 0, converged later, never converged)"""
    conv, iters = np.asarray(conv, bool), np.asarray(iters)
    return int((conv & (iters == 0)).sum()), int((conv & (iters > 0)).sum()), int((~conv).sum())
