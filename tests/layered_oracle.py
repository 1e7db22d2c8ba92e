"""The statement of layered (check-serial) BP in numpy -- TEST INFRASTRUCTURE: the rules of include/qbp.h
(qbp_layered_configure) on the CPU, which the kernel is compared with bit for bit.

The reference has no such decoder.  The statement is anchored to it through its row update:
  * sum-product rows are computed by the oracle itself (oracle.check_messages, iteration 0: tanh, the sequential
    product in ascending column order, t_safe, the division, the syndrome sign, the clip and 2 arctanh of
    beliefPropagation.py:114-126 in the oracle's host-independent numpy arithmetic).  The oracle's message dump takes
    the variants 1 and 2 only; variant 1 with alpha = 1.0 dumps R before the alpha scaling, computed by the very lines
    that variant 0 runs (bp_oracle.c, the `else` branch of the horizontal step), so that is the call made here.  Every
    row handed to it gets private columns holding its own d values -- the rows of one level share no variable, so this
    is exactly the row update;
  * min-sum rows are written as in tests/relay_oracle.py:_check_step (rework/decoding.py:28-56).

Two forms of one iteration: `sequential` visits the checks one after another in `order`; `level` runs level after level,
all checks of a level at once (the level of a check: 1 + the largest level of the checks that share a variable with it and
come earlier in the order).  tests/test_layered_cpu.py asserts that they agree in every bit.

All B records advance together; a record that has converged is frozen.  Every floating-point operation is one numpy
operation on float64 in the association the rules give.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import csr_matrix

from oracle import oracle

SUM_PRODUCT, MIN_SUM = 0, 2


class Tables:
    """Check c's columns in ascending order (ridx, rmask: [m, dmax]) and its weight."""

    def __init__(self, H):
        Hb = np.asarray(H) != 0
        self.Hb = Hb
        self.m, self.n = Hb.shape
        rows = [np.flatnonzero(Hb[c]) for c in range(self.m)]
        self.deg = np.array([len(r) for r in rows], np.int64)
        self.dmax = max(1, int(self.deg.max()))
        self.ridx = np.zeros((self.m, self.dmax), np.int64)
        self.rmask = np.zeros((self.m, self.dmax), bool)
        for c, r in enumerate(rows):
            self.ridx[c, :len(r)] = r
            self.rmask[c, :len(r)] = True


def default_order(H):
    """Greedy colouring: checks in ascending index, each the smallest colour no earlier neighbour (a check sharing a
    variable) holds; the order is by (colour, index).  Returns (order int32[m], colour int64[m])."""
    Hb = (np.asarray(H) != 0).astype(np.int64)
    m = Hb.shape[0]
    share = (Hb @ Hb.T) > 0
    colour = np.zeros(m, np.int64)
    for c in range(m):
        used = set(colour[c2] for c2 in range(c) if share[c, c2])
        k = 0
        while k in used:
            k += 1
        colour[c] = k
    order = np.array(sorted(range(m), key=lambda c: (colour[c], c)), np.int32)
    return order, colour


def check_levels(H, order):
    """Level of every check under `order` (1-based), int64[m]."""
    Hb = np.asarray(H) != 0
    m, n = Hb.shape
    var_level = np.zeros(n, np.int64)
    level = np.ones(m, np.int64)
    for c in np.asarray(order):
        vs = np.flatnonzero(Hb[c])
        lv = int(var_level[vs].max()) + 1 if len(vs) else 1
        level[c] = lv
        var_level[vs] = lv
    return level


def levels_of(H, order):
    """The levels as a list of arrays: the order sorted by level, stable."""
    order = np.asarray(order)
    level = check_levels(H, order)
    lv = level[order]
    return [order[lv == k] for k in range(1, int(lv.max()) + 1)] if len(order) else []


def _sp_rows(q, mask, sbits):
    """Sum-product row update of the valid entries of q [A, k, dmax] (rows (a, c), syndrome bits sbits [A, k]) by the
    oracle: a matrix with one row per (a, c) and private columns, the q values as its prior."""
    deg = mask.sum(axis=2).reshape(-1)
    E = int(deg.sum())
    indptr = np.concatenate(([0], np.cumsum(deg))).astype(np.int32)
    Hbig = csr_matrix((np.ones(E), np.arange(E, dtype=np.int32), indptr), shape=(len(deg), E))
    r = oracle.check_messages(Hbig, sbits.reshape(1, -1), q[mask], oracle.VARIANT_DAMPED_SP, alpha=1.0, iteration=0)
    out = np.zeros_like(q)
    out[mask] = r[0]
    return out


def _ms_rows(q, mask, sbits, alpha):
    """Min-sum row update (rework/decoding.py:28-56; tests/relay_oracle.py:_check_step) of q [A, k, dmax]."""
    ssign = (1 - 2 * sbits.astype(np.int64)).astype(np.float64)[:, :, None]
    with np.errstate(invalid="ignore"):
        sgn = np.where(np.isnan(q), np.nan, np.where(q < 0.0, -1.0, 1.0))
        sgn = np.where(mask, sgn, 1.0)
        row_sign = np.prod(sgn, axis=2, keepdims=True)
        r_signs = row_sign * sgn
        a = np.where(mask, np.abs(q), np.inf)
        i1 = np.argmin(a, axis=2)[..., None]
        min1 = np.take_along_axis(a, i1, axis=2)
        rest = a.copy()
        np.put_along_axis(rest, i1, np.inf, axis=2)
        min2 = np.min(rest, axis=2, keepdims=True)
        mag = np.where(a == min1, min2, min1)
        R = alpha * ssign * r_signs * mag
    return np.where(mask, R, 0.0)


def _step(T, cs, R, V, syn, variant, alpha, clip):
    """Steps 1 - 3 of the rules on the checks `cs` (which share no variable) of the records R [A, m, dmax], V [A, n],
    in place."""
    cs = np.asarray(cs, np.int64)
    A = R.shape[0]
    idx = T.ridx[cs]                                            # [k, dmax]
    mask = np.broadcast_to(T.rmask[cs][None], (A,) + idx.shape)
    d = V[:, idx] - R[:, cs, :]                                 # 1.
    if variant == MIN_SUM:
        r = _ms_rows(np.clip(d, -clip, clip), mask, syn[:, cs], alpha)
    else:
        r = _sp_rows(d, mask, syn[:, cs])                       # 2.
    R[:, cs, :] = np.where(mask, r, 0.0)                        # 3.
    rec = np.broadcast_to(np.arange(A)[:, None, None], mask.shape)
    var = np.broadcast_to(idx[None], mask.shape)
    V[rec[mask], var[mask]] = (d + r)[mask]


def layered_decode_batch(H, syndromes, prior, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, clip_llr=20.0, order=None,
                         form="level"):
    """The rules on B syndromes.  `order`: a permutation of the checks (None: the default order); `form`: "sequential"
    or "level".  Returns ``(hard uint8[B, n], converged bool[B], iters int32[B], llr float64[B, n])``."""
    assert variant in (SUM_PRODUCT, MIN_SUM) and max_iter >= 1 and form in ("sequential", "level")
    T = Tables(H)
    syn = np.atleast_2d(np.asarray(syndromes)).astype(np.uint8) & 1
    B = syn.shape[0]
    assert syn.shape[1] == T.m
    P = np.asarray(prior, np.float64)
    assert P.shape == (T.n,) and np.all(np.isfinite(P))
    order = default_order(H)[0] if order is None else np.asarray(order)
    assert sorted(order.tolist()) == list(range(T.m))
    if form == "level":
        groups = [g[T.deg[g] > 0] for g in levels_of(H, order)]
    else:
        groups = [np.array([c]) for c in order if T.deg[c] > 0]
    groups = [g for g in groups if len(g)]
    Hi = T.Hb.astype(np.int64)

    R = np.zeros((B, T.m, T.dmax), np.float64)
    V = P[None].repeat(B, axis=0)
    out_hard = np.zeros((B, T.n), np.uint8)
    out_llr = np.zeros((B, T.n), np.float64)
    conv = np.zeros(B, bool)
    iters = np.full(B, max_iter - 1, np.int32)
    for t in range(max_iter):
        A = np.flatnonzero(~conv)
        if len(A) == 0:
            break
        Ra, Va, sa = R[A], V[A], syn[A]
        for cs in groups:
            _step(T, cs, Ra, Va, sa, variant, float(alpha), float(clip_llr))
        R[A], V[A] = Ra, Va
        hard = Va < 0.0
        ok = np.all((hard.astype(np.int64) @ Hi.T) % 2 == sa, axis=1)
        b = A[ok]
        out_hard[b], out_llr[b], conv[b], iters[b] = hard[ok], Va[ok], True, t
    rest = ~conv
    out_hard[rest], out_llr[rest] = V[rest] < 0.0, V[rest]
    return out_hard, conv, iters, out_llr


def same(a, b):
    """Bit-for-bit equality of two outputs, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return np.array_equal(a, b)


# ---- the matrices of the tests -----------------------------------------------------------------------------------------
def steane():
    return np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]], np.uint8)


def irregular37():
    """An irregular 20 x 37 matrix with an empty check (row 5), an isolated variable (column 11) and one row of weight 11
    (row 3)."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.25, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1
    H[3] = 0
    H[3, rng.choice(37, 11, replace=False)] = 1
    H[5] = 0
    H[:, 11] = 0
    for c in range(20):                 # (no row of weight 1: its min-sum message is infinite, rework/decoding.py:44-53)
        while c != 5 and H[c].sum() < 2:
            H[c, rng.choice(np.setdiff1d(np.arange(37), [11]))] = 1
    assert H[3].sum() == 11 and H[5].sum() == 0 and H[:, 11].sum() == 0
    return H


def disjoint70():
    """70 pairwise disjoint rows of weight 3 (70 x 210): one level, wider than a wavefront."""
    H = np.zeros((70, 210), np.uint8)
    perm = np.random.default_rng(70).permutation(210)
    for c in range(70):
        H[c, perm[3 * c:3 * c + 3]] = 1
    return H


def matrix(name):
    from qldpc_amd import codes
    if name == "steane":
        return steane()
    if name == "72":
        return np.asarray(codes.load_code("[[72, 12, 6]]").Hx).astype(np.uint8)
    if name == "irr37":
        return irregular37()
    if name == "disjoint70":
        return disjoint70()
    if name == "144":
        return np.asarray(codes.load_code("[[144, 12, 12]]").Hx).astype(np.uint8)
    raise KeyError(name)


def order_of(H, kind):
    """The three orders of the tests: "default", "ascending", "random" (seeded)."""
    m = np.asarray(H).shape[0]
    if kind == "default":
        return default_order(H)[0]
    if kind == "ascending":
        return np.arange(m, dtype=np.int32)
    if kind == "random":
        return np.random.default_rng(1000 + m).permutation(m).astype(np.int32)
    raise KeyError(kind)
