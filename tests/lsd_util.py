"""Inputs shared by tests/test_lsd_cpu.py and tests/test_gpu_lsd.py: the matrices, and BP outputs to post-process
(computed by the CPU oracle, so the inputs are the same with and without a device)."""
import numpy as np

from oracle import oracle
from qldpc_amd import codes

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]], np.uint8)
NAMES = {"72": "[[72, 12, 6]]", "144": "[[144, 12, 12]]", "288": "[[288, 12, 18]]"}


def irregular37():
    """The irregular 20 x 37 matrix of tests/test_gd_cpu.py (row weights 1 .. 13, column weights 1 .. 7)."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.3, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1
    return H


def disjoint70():
    """70 disjoint rows of weight 3: more rows than lanes, every cluster stays on its own row."""
    H = np.zeros((70, 210), np.uint8)
    H[np.repeat(np.arange(70), 3), np.arange(210)] = 1
    return H


def matrix(name):
    if name == "steane":
        return STEANE
    if name == "rand37":
        return irregular37()
    if name == "rows70":
        return disjoint70()
    if name == "74":                    # [[72,12,6]] with two all-zero columns
        H = np.asarray(codes.load_code(NAMES["72"]).Hx, np.uint8)
        return np.concatenate([H, np.zeros((H.shape[0], 2), np.uint8)], axis=1)
    return np.asarray(codes.load_code(NAMES[name]).Hx, np.uint8)


def diag(H1, H2):
    H = np.zeros((H1.shape[0] + H2.shape[0], H1.shape[1] + H2.shape[1]), np.uint8)
    H[:H1.shape[0], :H1.shape[1]] = H1
    H[H1.shape[0]:, H1.shape[1]:] = H2
    return H


def bp_outputs(H, p, seed, B, iters):
    """B syndromes of Bernoulli(p) errors and what sum-product BP(iters) makes of them: (syn, llr, hard, converged)."""
    n = H.shape[1]
    errors = (np.random.default_rng(seed).random((B, n)) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, _, llr = oracle.decode_batch(H, syn, np.full(n, np.log((1 - p) / p)), iters)
    return syn, np.ascontiguousarray(llr, np.float64), np.ascontiguousarray(hard, np.uint8), np.asarray(conv, bool)


def bp_failures(H, p, seed, count, iters, batch=4096):
    """The first `count` records of a stream of BP(iters) outputs that did not converge."""
    syn, llr, hard, conv = bp_outputs(H, p, seed, batch, iters)
    f = np.flatnonzero(~conv)[:count]
    assert len(f) == count, (len(f), count)
    return syn[f], llr[f], hard[f]
