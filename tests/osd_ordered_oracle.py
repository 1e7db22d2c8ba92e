"""numpy statement of OSD with a GIVEN column order (include/qbp.h, qbp_osd_batch_ordered) -- TEST INFRASTRUCTURE.

The eight rules of tests/osd_order_oracle.py with "sorted by key" replaced by "the given permutation":

1. columns in the order ``order`` (a permutation of 0..n-1, least reliable first); ``|llr|`` plays no part in it;
2. Gauss-Jordan in that order up to rank(H): pivot columns S, fully reduced matrix A, reduced syndrome s;
3. candidate 0 = OSD-0: ``e_S = s``, ``e_T = 0``, ``x = hard ^ e``;
4. T = the non-pivot columns in the given order, ``w' = min(w, len(T))``;
5.-7. flip sets, cost (the sum of ``fabs(llr_i)`` over the support, NaN rules included) and selection as there;
8. a syndrome outside the column space of H returns the OSD-0 output, no search.

``osd0`` is decoding/OSD.py:3-72 on the permuted matrix, row swaps included: on a syndrome outside the column space
its output depends on them, and it is the reference's output for the reference's ``ordering``.
"""
from __future__ import annotations

import numpy as np

import osd_order_oracle as ordo
from osd_order_oracle import Reduced, candidates, costs, select


def _inputs(H, syndrome, hard, order):
    Hb = (np.asarray(H) != 0).astype(np.uint8)
    m, n = Hb.shape
    order = np.asarray(order).astype(np.int64)
    if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError("order must be a permutation of 0..n-1")
    hard = np.asarray(hard).astype(np.uint8) & 1
    syn = np.asarray(syndrome).astype(np.uint8) & 1
    s = ((syn.astype(np.int64) + hard.astype(np.int64) @ Hb.T.astype(np.int64)) % 2).astype(np.uint8)
    return Hb, m, n, order, hard, s


def osd0(H, syndrome, llr, hard, order):
    """uint8[n]: OSD-0 in the given column order, pivot rows swapped up as the reference does (``llr`` is unused: the
    order is given)."""
    Hb, m, n, order, hard, s = _inputs(H, syndrome, hard, order)
    A = np.concatenate([Hb[:, order], s[:, None]], axis=1)
    row, piv = 0, []
    for col in range(n):
        if row >= m:
            break
        below = np.flatnonzero(A[row:, col])
        if len(below) == 0:
            continue
        p = row + int(below[0])
        if p != row:
            A[[row, p]] = A[[p, row]]
        others = np.flatnonzero(A[:, col])
        others = others[others != row]
        A[others] ^= A[row]
        piv.append(col)
        row += 1
    x = hard.copy()
    if piv:
        x[order[np.array(piv)]] ^= A[:len(piv), n]
    return x


def reduce(H, syndrome, llr, hard, order) -> Reduced:
    """Rules 1-4 (the structure of osd_order_oracle.reduce)."""
    Hb, m, n, order, hard, s = _inputs(H, syndrome, hard, order)
    llr = np.asarray(llr, np.float64)
    A = np.concatenate([Hb, s[:, None]], axis=1)
    used = np.zeros(m, bool)
    piv_row, piv_col = [], []
    for c in order:
        if len(piv_row) == m:
            break
        cand = np.flatnonzero((A[:, c] == 1) & ~used)
        if len(cand) == 0:
            continue
        p = cand[0]
        others = np.flatnonzero(A[:, c] == 1)
        others = others[others != p]
        A[others] ^= A[p]
        used[p] = True
        piv_row.append(p)
        piv_col.append(c)
    if A[~used, n].any():
        return Reduced(osd0(Hb, syndrome, llr, hard, order), False, np.array(piv_col, np.int64),
                       np.zeros((len(piv_row), 0), np.uint8), np.zeros(0, np.int64), np.abs(llr))
    x0 = hard.copy()
    rows = np.array(piv_row, np.int64)
    S = np.array(piv_col, np.int64)
    x0[S] ^= A[rows, n] if len(rows) else np.zeros(0, np.uint8)
    is_piv = np.zeros(n, bool)
    is_piv[S] = True
    T = order[~is_piv[order]]
    A_T = A[np.ix_(rows, T)] if len(rows) else np.zeros((0, len(T)), np.uint8)
    return Reduced(x0, True, S, A_T, T, np.abs(llr))


def osd_order(H, syndrome, llr, hard, order, w, method="cs", red: Reduced | None = None):
    """uint8[n]: the order-w OSD solution of one record in the column order ``order``."""
    red = reduce(H, syndrome, llr, hard, order) if red is None else red
    if not red.consistent or w == 0:
        return red.x0.copy()
    X = candidates(red, method, w)
    return X[select(costs(X, red.absl))]


def osd_order_batch(H, syndromes, llrs, hards, orders, w, method="cs"):
    return np.stack([osd_order(H, s, l, h, o, w, method) for s, l, h, o in zip(syndromes, llrs, hards, orders)])


sort_order = ordo.sort_order
