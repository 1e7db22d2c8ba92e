"""Inputs shared by tests/test_lsd_cpu.py, tests/test_gpu_lsd.py and tests/test_gpu_lsd_sizes.py: the matrices, BP
outputs to post-process (computed by the CPU oracle, so the inputs are the same with and without a device), and the
launch arithmetic of lsd_kernel restated in Python (lsd_lds_bytes of qbp_lsd.hpp, the grid of lsd_launch in qbp.hip)."""
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


def rows2048(extra_row=False):
    """2048 x 384 (one row more: 2049 x 384), every row of weight 3, no empty column: as many rows as the kernel's 32-bit
    per-lane row masks hold.  Rows 0 .. 63 live on columns 0 .. 31 and rows 1984 .. 2047 on columns 352 .. 383, which no
    other row touches: a column of the upper block finds its pivot in the last 64-row pass (bit 31 of the masks), and
    the two blocks are clusters of their own.  The rows between, and the extra row, are random on columns 32 .. 351."""
    rng = np.random.default_rng(2048)
    m = 2049 if extra_row else 2048
    H = np.zeros((m, 384), np.uint8)
    for r in range(2048):
        lo, width = (0, 32) if r < 64 else (352, 32) if r >= 1984 else (32, 320)
        H[r, lo + rng.choice(width, 3, replace=False)] = 1
    if extra_row:
        H[2048, 32 + rng.choice(320, 3, replace=False)] = 1
    assert H.sum(1).tolist() == [3] * m and H.sum(0).min() > 0
    return H


def sort_edge(n):
    """An irregular 100 x n matrix in the style of irregular37 (row weights 2 .. 21, no empty column): n = 256 is a
    power of two (the bitonic sort runs without a padding key), n = 257 pads to 512 (255 padding keys)."""
    rng = np.random.default_rng(n)
    H = (rng.random((100, n)) < rng.uniform(0.01, 0.05, size=(100, 1))).astype(np.uint8)
    H[np.arange(100), rng.integers(0, n, 100)] = 1
    H[rng.integers(0, 100, n), np.arange(n)] = 1
    return H


# ---- the launch arithmetic of lsd_kernel (no GPU) ------------------------------------------------------------------------
LDS_LIMIT = 160 * 1024
MAX_ROWS, MAX_COLS = 64 * 32, 65535


def lsd_lds_bytes(m, n):
    """lsd_lds_bytes of qbp_lsd.hpp: osd_region0_bytes { u64 keys[NP] | u32 A[m][W + 1] }, then int pivcol / label and
    u32 pick / prev [m], u16 idx[NP] and rank[n], u8 sol / act [n], u8 bad[m], and 16 spare bytes."""
    W = -(-n // 32)
    NP = 1
    while NP < n:
        NP <<= 1
    region0 = -(-max(8 * NP, 4 * m * (W + 1)) // 8) * 8
    return region0 + 16 * m + 2 * NP + 4 * n + m + 16


def lsd_lds16(m, n):
    """What the launch asks for: the size rounded up to 16."""
    return -(-lsd_lds_bytes(m, n) // 16) * 16


def lsd_grid(m, n, B, num_cu, blocks_per_cu=0):
    """The grid of lsd_launch: one wavefront per workgroup, as many per CU as the LDS holds, at most 32;
    QBP_OPT_BLOCKS_PER_CU overrides the count."""
    per_cu = max(1, min(32, LDS_LIMIT // lsd_lds16(m, n)))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return max(1, min(B, num_cu * per_cu))


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
