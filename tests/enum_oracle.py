"""The pattern order of the weight-w enumeration (include/qbp.h), stated independently of qldpc_amd/enumerate.py:
``patterns`` walks ``itertools.combinations`` itself, ``unrank_int`` is a Python-int unranker for ranks no walk
reaches, and ``kinds_of`` is the numpy statement of what qbp_enum_failures captures."""
import itertools
import math

import numpy as np


def patterns(n, w, begin=0, T=None):
    """uint8[T, n]: rows begin .. begin + T of the class, in the order of itertools.combinations(range(n), w)."""
    total = math.comb(n, w)
    T = total - begin if T is None else T
    assert 0 <= begin and begin + T <= total
    out = np.zeros((T, n), np.uint8)
    for b, cols in enumerate(itertools.islice(itertools.combinations(range(n), w), begin, begin + T)):
        out[b, list(cols)] = 1
    return out


def unrank_int(n, w, r):
    """The ascending columns of rank r: peel the first column off by counting the tuples that start with each
    candidate (recursive in the remaining columns; Python ints)."""
    assert 0 <= r < math.comb(n, w)
    cols, first = [], 0
    for left in range(w, 0, -1):
        for c in range(first, n):
            starting_here = math.comb(n - c - 1, left - 1)
            if r < starting_here:
                cols.append(c)
                first = c + 1
                break
            r -= starting_here
    assert r == 0 and len(cols) == w
    return cols


def rows_of(n, cols_list):
    out = np.zeros((len(cols_list), n), np.uint8)
    for b, cols in enumerate(cols_list):
        out[b, cols] = 1
    return out


def kinds_of(H, L, rows, prior, max_iter, osd=False, threads=8):
    """(kinds uint8[T], hard uint8[T, n], conv bool[T], iters): kind = (L x != L e) | 2 (BP did not converge), x = BP's
    hard decision, or OSD-0's solution where BP did not converge and ``osd`` is set."""
    from oracle import oracle
    H = np.asarray(H).astype(np.int64)
    L = np.asarray(L).astype(np.int64)
    syn = (rows.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, llr = oracle.decode_batch(H, syn, prior, max_iter, threads=threads)
    hard = hard.copy()
    if osd:
        for i in np.flatnonzero(~conv):
            hard[i] = oracle.osd0(H, syn[i], llr[i], hard[i])
    logical = (((hard.astype(np.int64) ^ rows.astype(np.int64)) @ L.T) % 2).any(axis=1)
    return (logical.astype(np.uint8) | (2 * (~conv)).astype(np.uint8)), hard, conv, iters
