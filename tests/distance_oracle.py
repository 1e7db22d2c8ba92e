"""numpy statement of the randomized information-set distance search (include/qbp.h, qbp_distance_search) -- TEST
INFRASTRUCTURE.  The algorithm is QDistRnd's (Pryadko, Shabashov, Kozin 2022).

Inputs: G [r][n] 0/1, every row in ker H (rows may be dependent); L [k][n] 0/1, 1 <= k <= 64; a 64-bit seed; global trial
indices [trial_begin, trial_end).

Trial t:
  1. key[v] = word v & 3 of Philox4x32-10(counter (lo32(t), hi32(t), v >> 2, PHILOX_STREAM), key (lo32(seed), hi32(seed)));
     the column order is the columns sorted ascending by (key[v], v).
  2. Gauss-Jordan on a copy of G, columns in that order: the pivot of a column is the lowest not yet used row with a 1 in
     it; none: skip the column; else XOR the pivot row into every other row with a 1 there and mark it used.  Stop when
     every row is used or the columns are exhausted.
  3. For every row i of the reduced matrix: w_i its weight, lm_i the mask whose bit l is parity(L[l] & row_i); the row is
     a candidate when lm_i != 0.
  4. The trial's result is the candidate with the smallest (w_i, i); none: the trial has no result.
Call: hist[w] += 1 per trial with a result (ADDED to); result = (trials run, smallest w or -1, smallest trial index that
reached it or -1, that trial's row i or -1); codeword = that row, logical_mask = its lm (both untouched without a result).

WRONG STATEMENTS.  ``trial`` and ``search`` take optional keyword arguments, each of which replaces one rule above by a
defect a kernel could have; the defaults are the rules.  tests/test_distance_large_cpu.py uses them to show that a case
tells the defect from the statement (a GPU comparison on that case then means something about it):
  ties="descending"     step 1 orders equal keys by descending column
  pivot_rows=R          step 2 never chooses a row >= R as a pivot
  column_budget=C       step 2 stops after the first C columns of the order
  candidate_rows=R      step 3 never considers a row >= R
  weight_columns=C      step 3 counts w_i over the columns < C only
"""
import numpy as np

from dem_sampler import philox4x32_10

PHILOX_STREAM = 4                # counter word 3 (QBP_DISTANCE_PHILOX_STREAM)
_MASK = 0xFFFFFFFF


def column_keys(seed, t, n):
    """key[v] of trial t, uint64[n] holding 32-bit words."""
    seed, t = int(seed), int(t)
    n4 = (n + 3) // 4
    g = np.arange(n4, dtype=np.uint64)
    words = philox4x32_10((np.full(n4, t & _MASK, np.uint64), np.full(n4, (t >> 32) & _MASK, np.uint64), g,
                           np.full(n4, PHILOX_STREAM, np.uint64)), (seed & _MASK, (seed >> 32) & _MASK))
    return np.stack(words, axis=-1).reshape(4 * n4)[:n]


def column_order(seed, t, n, ties="ascending"):
    keys = column_keys(seed, t, n)
    if ties == "descending":                      # (a wrong statement)
        return (n - 1 - np.argsort(keys[::-1], kind="stable")).astype(np.int64)
    assert ties == "ascending"
    return np.argsort(keys, kind="stable")                            # ties in the key: by column index


def reduce_rows(G, order, pivot_rows=None, column_budget=None):
    """Step 2 -> the reduced matrix uint8[r][n].  (pivot_rows, column_budget: wrong statements.)"""
    A = (np.asarray(G).astype(np.uint8) & 1).copy()
    r = A.shape[0]
    used = np.zeros(r, bool)
    left = r
    for c in order if column_budget is None else order[:column_budget]:
        if left == 0:
            break
        has = A[:, c] != 0
        cand = np.flatnonzero(has & ~used)
        if pivot_rows is not None:
            cand = cand[cand < pivot_rows]
        if cand.size == 0:
            continue
        p = int(cand[0])
        has[p] = False
        A[has] ^= A[p]
        used[p] = True
        left -= 1
    return A


def logical_masks(A, L):
    """lm of every row of A: python ints (bit l: parity(L[l] & row))."""
    par = (A.astype(np.int64) @ (np.asarray(L).astype(np.int64) & 1).T) % 2          # [r][k]
    return [sum(1 << int(l) for l in np.flatnonzero(row)) for row in par]


def trial(G, L, seed, t, ties="ascending", pivot_rows=None, column_budget=None, candidate_rows=None, weight_columns=None):
    """The result of trial t: (w, i, row uint8[n], lm) or None.  (The keyword arguments: wrong statements.)"""
    n = np.asarray(G).shape[1]
    A = reduce_rows(G, column_order(seed, t, n, ties), pivot_rows, column_budget)
    w = A[:, :weight_columns].sum(axis=1, dtype=np.int64)
    lm = logical_masks(A, L)
    best = None
    for i in range(A.shape[0] if candidate_rows is None else min(A.shape[0], candidate_rows)):
        if lm[i] and (best is None or (int(w[i]), i) < best[:2]):
            best = (int(w[i]), i, A[i].copy(), lm[i])
    return best


def search(G, L, seed, trial_begin, trial_end, hist=None, **wrong):
    """The call -> dict(result int64[4], hist int64[n + 1] (``hist`` added to, a copy), codeword uint8[n] or None,
    logical_mask int or None).  (``wrong``: the keyword arguments of ``trial``.)"""
    G, L = np.asarray(G), np.asarray(L)
    n = G.shape[1]
    assert L.ndim == 2 and L.shape[1] == n and 1 <= L.shape[0] <= 64 and G.shape[0] >= 1
    hist = np.zeros(n + 1, np.int64) if hist is None else np.array(hist, np.int64)
    best = None                                   # (w, t, i, row, lm)
    for t in range(int(trial_begin), int(trial_end)):
        res = trial(G, L, seed, t, **wrong)
        if res is None:
            continue
        w, i, row, lm = res
        hist[w] += 1
        if best is None or w < best[0]:           # (ascending t: the smallest trial index that reaches a weight)
            best = (w, t, i, row, lm)
    result = np.array([int(trial_end) - int(trial_begin), -1, -1, -1], np.int64)
    if best is not None:
        result[1:] = best[:3]
    return dict(result=result, hist=hist, codeword=None if best is None else best[3],
                logical_mask=None if best is None else best[4])


def merge(a, b):
    """Two adjacent ranges -> their union (a first)."""
    ra, rb = a["result"], b["result"]
    pick = a if rb[1] < 0 or (ra[1] >= 0 and (ra[1], ra[2]) <= (rb[1], rb[2])) else b
    result = pick["result"].copy()
    result[0] = ra[0] + rb[0]
    return dict(result=result, hist=a["hist"] + b["hist"], codeword=pick["codeword"], logical_mask=pick["logical_mask"])
