"""The statement of Relay-BP in numpy -- TEST INFRASTRUCTURE: the rules of include/qbp.h (qbp_relay_decode_batch) as
array operations on the CPU, which the kernel is compared with bit for bit.

The reference has no such decoder.  The statement is anchored to it by one identity (tests/test_relay_cpu.py): with
gammas all zero, one leg and stop_after = 1 it is performMinSum_Symmetric (rework/decoding.py:5-75) with damping = 1.0,
which oracle.decode_batch(variant=2) restates and the project reproduces bit for bit.

All B records advance together, one iteration per pass, each in its own leg (a record that finds a solution leaves its
leg early, so records of one batch are in different legs).  Messages live on the edges: row c holds the messages of
check c in ascending column order, padded to the largest row weight.  Every floating-point operation is one numpy
operation on float64, in the association the rules give; nothing is fused or reordered.
"""
from __future__ import annotations

import numpy as np


class Tables:
    """Edge lists of H: check c's columns in ascending order (ridx, rmask: [m, dmax]); variable v's edges in ascending
    check order as flat indices c * dmax + j (cidx, cmask: [n, cmax])."""

    def __init__(self, H):
        Hb = np.asarray(H) != 0
        self.m, self.n = Hb.shape
        rows = [np.flatnonzero(Hb[c]) for c in range(self.m)]
        self.dmax = max(1, max(len(r) for r in rows))
        self.ridx = np.zeros((self.m, self.dmax), np.int64)
        self.rmask = np.zeros((self.m, self.dmax), bool)
        cols = [[] for _ in range(self.n)]
        for c, r in enumerate(rows):                      # ascending check: a column's list ends up in that order
            self.ridx[c, :len(r)] = r
            self.rmask[c, :len(r)] = True
            for j, v in enumerate(r):
                cols[v].append(c * self.dmax + j)
        self.cmax = max(1, max(len(e) for e in cols))
        self.cidx = np.zeros((self.n, self.cmax), np.int64)
        self.cmask = np.zeros((self.n, self.cmax), bool)
        for v, e in enumerate(cols):
            self.cidx[v, :len(e)] = e
            self.cmask[v, :len(e)] = True


def _check_step(T, Q, ssign, alpha):
    """Rule 2a on Q [A, m, dmax]: the min-sum check update of rework/decoding.py:28-56 on the edges of every row --
    sign of a message with 0 -> +1 (NaN stays NaN), the row's sign product, the smallest magnitude (first occurrence:
    lowest column) and the smallest of the others, R = alpha * syndrome_sign * (row sign * own sign) * magnitude."""
    with np.errstate(invalid="ignore"):
        sgn = np.where(np.isnan(Q), np.nan, np.where(Q < 0.0, -1.0, 1.0))
        sgn = np.where(T.rmask, sgn, 1.0)
        row_sign = np.prod(sgn, axis=2, keepdims=True)
        r_signs = row_sign * sgn
        a = np.where(T.rmask, np.abs(Q), np.inf)
        i1 = np.argmin(a, axis=2)[..., None]
        min1 = np.take_along_axis(a, i1, axis=2)
        rest = a.copy()
        np.put_along_axis(rest, i1, np.inf, axis=2)
        min2 = np.min(rest, axis=2, keepdims=True)
        mag = np.where(a == min1, min2, min1)
        R = alpha * ssign * r_signs * mag
    return np.where(T.rmask, R, 0.0)


def _column_sums(T, R):
    """Rule 2c's colsum: every column's messages added in ascending check order, left to right; an empty column is 0."""
    Rf = R.reshape(R.shape[0], -1)
    acc = np.where(T.cmask[:, 0], Rf[:, T.cidx[:, 0]], 0.0)
    with np.errstate(invalid="ignore"):
        for j in range(1, T.cmax):
            acc = np.where(T.cmask[:, j], acc + Rf[:, T.cidx[:, j]], acc)
    return acc


def relay_decode_batch(H, syndromes, prior, gammas, leg_iters, stop_after=1, alpha=1.0, clip_llr=20.0):
    """The rules on B syndromes.  Returns a dict: hard uint8[B, n], llr float64[B, n], converged bool[B], iters, legs,
    solutions, best_leg (-1: none), first_leg (leg of the first solution, -1: none), replaced (times a later solution
    strictly replaced the best one) -- int32[B] each."""
    T = Tables(H)
    syn = np.atleast_2d(np.asarray(syndromes)).astype(np.int64) & 1
    B = syn.shape[0]
    assert syn.shape[1] == T.m
    P = np.asarray(prior, np.float64)
    G = np.asarray(gammas, np.float64)
    iters_of = np.asarray(leg_iters, np.int64)
    L = G.shape[0]
    assert P.shape == (T.n,) and G.shape == (L, T.n) and iters_of.shape == (L,) and L >= 1
    assert np.all(iters_of >= 1) and stop_after >= 1
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(G))
    alpha, clip = float(alpha), float(clip_llr)
    ssign_all = (1 - 2 * syn).astype(np.float64)[:, :, None]

    # rule 1
    Q = np.where(T.rmask, P[T.ridx], 0.0)[None].repeat(B, axis=0)
    V = P[None].repeat(B, axis=0)
    found, total, t = (np.zeros(B, np.int32) for _ in range(3))
    leg = np.zeros(B, np.int64)
    legs = np.ones(B, np.int32)
    best_w = np.zeros(B, np.float64)
    best_leg, first_leg = (np.full(B, -1, np.int32) for _ in range(2))
    replaced = np.zeros(B, np.int32)
    out_hard = np.zeros((B, T.n), np.uint8)
    out_llr = np.zeros((B, T.n), np.float64)
    done = np.zeros(B, bool)

    while not done.all():
        A = np.flatnonzero(~done)
        g = G[leg[A]]
        R = _check_step(T, Q[A], ssign_all[A], alpha)                    # 2a
        with np.errstate(invalid="ignore"):
            bias = (1.0 - g) * P + g * V[A]                              # 2b
            Vn = _column_sums(T, R) + bias                               # 2c
            Qn = np.clip(Vn[:, T.ridx] - R, -clip, clip)                 # 2d
        Q[A] = np.where(T.rmask, Qn, 0.0)
        V[A] = Vn                                                        # 2e
        total[A] += 1
        t[A] += 1
        hard = Vn < 0.0                                                  # 2f
        ok = np.all((hard[:, T.ridx] & T.rmask).sum(axis=2) % 2 == syn[A], axis=1)
        for k in np.flatnonzero(ok):
            b = A[k]
            w = 0.0
            for v in np.flatnonzero(hard[k]):                            # ascending v, from +0.0
                w += P[v]
            if found[b] == 0 or w < best_w[b]:
                if found[b] > 0:
                    replaced[b] += 1
                else:
                    first_leg[b] = leg[b]
                best_w[b], best_leg[b] = w, leg[b]
                out_hard[b], out_llr[b] = hard[k], Vn[k]
            found[b] += 1
        for k in np.flatnonzero(ok | (t[A] >= iters_of[leg[A]])):        # the leg ends
            b = A[k]
            if found[b] >= stop_after or leg[b] + 1 >= L:                # rule 3
                done[b] = True
            else:
                leg[b] += 1
                legs[b] += 1
                t[b] = 0
    none = found == 0                                                    # rule 4
    out_hard[none] = V[none] < 0.0
    out_llr[none] = V[none]
    return dict(hard=out_hard, llr=out_llr, converged=found > 0, iters=total, legs=legs, solutions=found,
                best_leg=best_leg, first_leg=first_leg, replaced=replaced)


def relay_decode(H, syndrome, prior, gammas, leg_iters, stop_after=1, alpha=1.0, clip_llr=20.0):
    """One record: the dict of ``relay_decode_batch`` with the leading axis removed."""
    r = relay_decode_batch(H, np.asarray(syndrome).reshape(1, -1), prior, gammas, leg_iters, stop_after, alpha, clip_llr)
    return {k: v[0] for k, v in r.items()}


def classes(r):
    """The four classes the device tests need present: solved in leg 0, solved only in a later leg, a second solution
    that strictly replaced the first, never solved (counts)."""
    return dict(leg0=int((r["first_leg"] == 0).sum()), later=int((r["first_leg"] > 0).sum()),
                replaced=int((r["replaced"] > 0).sum()), never=int((~r["converged"]).sum()))


def same(a, b):
    """Bit-for-bit equality of two outputs, NaN equal to NaN (a NaN carries no payload the rules define)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return np.array_equal(a, b)
