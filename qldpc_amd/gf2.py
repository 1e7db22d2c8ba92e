"""Linear algebra over GF(2) on the host (numpy): rank, reduced row echelon form, null space.

Cold code: it runs once per code (``codes.css_logicals``, ``distance.bound``), on matrices of a few thousand columns at
the most.  Rows are bit-packed into bytes (``np.packbits``), so one row operation is one XOR of ``n / 8`` bytes.

Everything here is deterministic, by one rule: the columns are visited in ascending order, and the pivot of a column is
the LOWEST row (smallest index) among the rows that do not serve as a pivot yet and have a 1 there.  Rows are never
swapped: a pivot row stays where it is.
"""
from __future__ import annotations

import numpy as np


def _as_bits(A) -> np.ndarray:
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError(f"a matrix is needed, got shape {A.shape}")
    return (A.astype(np.int64) & 1).astype(np.uint8)


def _eliminate(A: np.ndarray):
    """Gauss-Jordan by the rule above -> (packed reduced rows [m][ceil(n / 8)], pivot rows, pivot columns), the last
    two in the order the pivots were found (ascending columns)."""
    m, n = A.shape
    P = np.packbits(A, axis=1) if n else np.zeros((m, 0), np.uint8)
    used = np.zeros(m, bool)
    prow, pcol = [], []
    for c in range(n):
        if len(prow) == m:
            break
        byte, bit = c >> 3, np.uint8(0x80 >> (c & 7))
        has = (P[:, byte] & bit) != 0
        cand = np.flatnonzero(has & ~used)
        if cand.size == 0:
            continue
        p = int(cand[0])
        has[p] = False
        P[has] ^= P[p]
        used[p] = True
        prow.append(p)
        pcol.append(c)
    return P, np.asarray(prow, np.int64), np.asarray(pcol, np.int64)


def rank(A) -> int:
    """Rank of ``A`` over GF(2)."""
    return int(_eliminate(_as_bits(A))[1].size)


def row_reduce(A):
    """Reduced row echelon form of ``A`` -> ``(R, pivots)``: ``R`` uint8 ``[rank][n]``, its rows the pivot rows in
    ascending order of their pivot columns ``pivots`` (int64 ``[rank]``); column ``pivots[i]`` of ``R`` is the unit
    vector ``e_i``.  The row space of ``R`` is the row space of ``A``."""
    A = _as_bits(A)
    P, prow, pcol = _eliminate(A)
    n = A.shape[1]
    R = np.unpackbits(P[prow], axis=1)[:, :n] if n else np.zeros((prow.size, 0), np.uint8)
    return np.ascontiguousarray(R, np.uint8), pcol


def nullspace(A) -> np.ndarray:
    """A basis of ``{v : A v = 0}`` over GF(2), uint8 ``[n - rank][n]``.

    The rule: ``A`` is reduced with pivots in ascending column order, lowest row first (see the module docstring);
    there is one basis vector per free (non-pivot) column, in ascending order of the free columns.  The vector of free
    column ``f`` has a 1 at ``f``, a 0 at every other free column, and at pivot column ``pivots[i]`` the entry
    ``R[i, f]`` of the reduced matrix."""
    A = _as_bits(A)
    n = A.shape[1]
    R, piv = row_reduce(A)
    free = np.setdiff1d(np.arange(n), piv)
    N = np.zeros((free.size, n), np.uint8)
    N[np.arange(free.size), free] = 1
    if piv.size:
        N[:, piv] = R[:, free].T
    return N
