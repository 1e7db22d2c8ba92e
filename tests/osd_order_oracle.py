"""numpy statement of order-w OSD (include/qbp.h, qbp_osd_batch) -- TEST INFRASTRUCTURE.

One record ``(H, syndrome, llr, hard)``, method "cs" (combination sweep) or "e" (exhaustive), order w:

1. columns sorted by ``(|llr| as the OSD-0 sort key, column index)`` ascending (NaN last, NaNs equal);
2. Gauss-Jordan in that order up to rank(H): pivot columns S, fully reduced matrix A, reduced syndrome s;
3. candidate 0 = OSD-0: ``e_S = s``, ``e_T = 0``, ``x = hard ^ e``;
4. T = the non-pivot columns in sort order, ``w' = min(w, len(T))``;
5. a candidate flips ``F`` within T: ``e_T = 1_F``, ``e_S(r) = s_r ^ XOR_{j in F} A[r][j]``; CS: all weight-1 sets
   over T, then the weight-2 sets over ``T[:w']`` (itertools.combinations order); E: every non-empty subset of
   ``T[:w']`` by weight, then combinations order;
6. ``cost(x)`` = sum of ``fabs(llr_i)`` over ``x_i = 1``, added left to right in ascending column from +0.0;
7. the first candidate of least cost wins; an OSD-0 cost of NaN returns OSD-0, NaN costs never win;
8. a syndrome outside the column space of H returns the OSD-0 output (``oracle.osd0``), no search.

Order 0 is OSD-0 for either method.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

from oracle import oracle

MAX_ORDER = {"cs": 64, "e": 12}


def order_key(llr):
    """The OSD-0 sort key: the bit pattern of |llr| (monotone for non-negative doubles), one pattern for NaN."""
    a = np.abs(np.asarray(llr, np.float64))
    key = a.view(np.uint64).copy()
    key[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return key


def sort_order(llr):
    n = len(llr)
    return np.lexsort((np.arange(n), order_key(llr)))


@dataclass
class Reduced:
    x0: np.ndarray          # OSD-0 solution, uint8[n]
    consistent: bool
    S: np.ndarray           # pivot column of each pivot row (in pivot order)
    A_T: np.ndarray         # uint8[rank, k']: reduced entries of the pivot rows on T
    T: np.ndarray           # non-pivot columns in sort order
    absl: np.ndarray        # |llr|


def reduce(H, syndrome, llr, hard) -> Reduced:
    """Steps 1-4: the full Gauss-Jordan sweep and the OSD-0 candidate."""
    Hb = (np.asarray(H) != 0).astype(np.uint8)
    m, n = Hb.shape
    llr = np.asarray(llr, np.float64)
    hard = np.asarray(hard).astype(np.uint8) & 1
    syn = np.asarray(syndrome).astype(np.uint8) & 1
    s = (syn.astype(np.int64) + hard.astype(np.int64) @ Hb.T.astype(np.int64)) % 2
    A = np.concatenate([Hb, s.astype(np.uint8)[:, None]], axis=1)
    used = np.zeros(m, bool)
    piv_row, piv_col = [], []
    for c in sort_order(llr):
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
    consistent = not A[~used, n].any()
    if not consistent:
        return Reduced(oracle.osd0(Hb, syn, llr, hard), False, np.array(piv_col, np.int64),
                       np.zeros((len(piv_row), 0), np.uint8), np.zeros(0, np.int64), np.abs(llr))
    x0 = hard.copy()
    rows = np.array(piv_row, np.int64)
    S = np.array(piv_col, np.int64)
    x0[S] ^= A[rows, n] if len(rows) else np.zeros(0, np.uint8)
    is_piv = np.zeros(n, bool)
    is_piv[S] = True
    order = sort_order(llr)
    T = order[~is_piv[order]]
    A_T = A[np.ix_(rows, T)] if len(rows) else np.zeros((0, len(T)), np.uint8)
    return Reduced(x0, True, S, A_T, T, np.abs(llr))


def flip_sets(method, order, kp):
    """Step 5: the flip sets (tuples of positions in T) after OSD-0, in enumeration order."""
    if method not in MAX_ORDER:
        raise ValueError(method)
    if order == 0:
        return []
    wp = min(order, kp)
    if method == "cs":
        return [(t,) for t in range(kp)] + list(itertools.combinations(range(wp), 2))
    return [F for k in range(1, wp + 1) for F in itertools.combinations(range(wp), k)]


def candidates(red: Reduced, method, order):
    """uint8[1 + len(flip sets), n]: OSD-0, then every candidate in enumeration order."""
    sets = flip_sets(method, order, len(red.T))
    X = np.repeat(red.x0[None, :], 1 + len(sets), axis=0)
    if sets:
        Fm = np.zeros((len(sets), len(red.T)), np.uint8)
        for i, F in enumerate(sets):
            Fm[i, list(F)] = 1
        dS = (Fm.astype(np.int64) @ red.A_T.T.astype(np.int64)) % 2
        X[1:, red.T] ^= Fm
        X[1:, red.S] ^= dS.astype(np.uint8)
    return X


def costs(X, absl):
    """Step 6 for every row of X: left-to-right sums from +0.0 (zero terms are exact no-ops)."""
    terms = np.where(X.astype(bool), absl[None, :], 0.0)
    if terms.shape[1] == 0:
        return np.zeros(len(X))
    return np.cumsum(terms, axis=1)[:, -1]


def select(c):
    """Step 7: index of the winning candidate."""
    if np.isnan(c[0]):
        return 0
    ok = ~np.isnan(c)
    best = c[ok].min()
    return int(np.flatnonzero(ok & (c == best))[0])


def osd_order(H, syndrome, llr, hard, order, method="cs", red: Reduced | None = None):
    """uint8[n]: the order-w OSD solution of one record (``red``: a precomputed ``reduce`` of it)."""
    red = reduce(H, syndrome, llr, hard) if red is None else red
    if not red.consistent or order == 0:
        return red.x0.copy()
    X = candidates(red, method, order)
    return X[select(costs(X, red.absl))]


def osd_order_batch(H, syndromes, llrs, hards, order, method="cs"):
    return np.stack([osd_order(H, s, l, h, order, method) for s, l, h in zip(syndromes, llrs, hards)])
