"""The statement of BP guided decimation (BPGD) in numpy -- TEST INFRASTRUCTURE: the rules of include/qbp.h
(qbp_gd_decode_batch) as array operations on the CPU, which the kernel is compared with bit for bit.

The reference has no such decoder.  The statement is anchored to it by one identity (tests/test_gd_cpu.py): with
max_rounds = 0 it is oracle.decode_batch(max_iter = T) -- the plain sum-product, or min-sum with damping = 1.0.

  * min-sum rows and the column sum are those of tests/relay_oracle.py (_check_step, _column_sums);
  * sum-product rows are computed by the oracle itself, the way tests/layered_oracle.py takes them (_sp_rows:
    oracle.check_messages on a matrix with one private column per edge, in the oracle's host-independent numpy
    arithmetic).

All B records advance together, one iteration per pass, each in its own round.  Messages live on the edges: row c holds
the messages of check c in ascending column order, padded to the largest row weight.  Every floating-point operation
is one numpy operation on float64, in the association the rules give; nothing is fused or reordered.
"""
from __future__ import annotations

import numpy as np

import layered_oracle as lo
import relay_oracle as ro

SUM_PRODUCT, MIN_SUM = 0, 2
same = ro.same


def choose(V, decimated, col_weight):
    """Rule 3 on one record: the variable to decimate, or -1.  Candidates: not decimated, column weight >= 1, V not NaN;
    the largest |V|, equal values to the lowest index (np.argmax returns the first maximum)."""
    V = np.asarray(V, np.float64)
    cand = ~np.asarray(decimated, bool) & (np.asarray(col_weight) >= 1) & ~np.isnan(V)
    if not cand.any():
        return -1
    key = np.where(cand, np.abs(V), -1.0)
    return int(np.argmax(key))


def gd_decode_batch(H, syndromes, prior, iters_per_round, max_rounds, decim_llr, variant=MIN_SUM, alpha=1.0,
                    clip_llr=20.0):
    """The rules on B syndromes.  Returns a dict: hard uint8[B, n], llr float64[B, n], converged bool[B], iters,
    rounds int32[B], and `cls` int8[B]: 0 solved in round 0 (before any decimation), 1 solved after >= 1 decimation,
    2 never solved."""
    assert variant in (SUM_PRODUCT, MIN_SUM)
    T = ro.Tables(H)
    col_weight = (np.asarray(H) != 0).sum(axis=0)
    syn = np.atleast_2d(np.asarray(syndromes)).astype(np.int64) & 1
    B = syn.shape[0]
    assert syn.shape[1] == T.m
    P = np.asarray(prior, np.float64)
    assert P.shape == (T.n,) and np.all(np.isfinite(P))
    Tr, max_rounds = int(iters_per_round), int(max_rounds)
    alpha, clip, dl = float(alpha), float(clip_llr), float(decim_llr)
    assert Tr >= 1 and max_rounds >= 0 and dl > 0 and np.isfinite(dl)
    ssign_all = (1 - 2 * syn).astype(np.float64)[:, :, None]

    # rule 1
    W = P[None].repeat(B, axis=0)
    Q = np.where(T.rmask, P[T.ridx], 0.0)[None].repeat(B, axis=0)
    V = P[None].repeat(B, axis=0)
    D = np.zeros((B, T.n), bool)
    total, rounds, t = (np.zeros(B, np.int32) for _ in range(3))
    conv = np.zeros(B, bool)
    done = np.zeros(B, bool)

    while not done.all():
        A = np.flatnonzero(~done)
        if variant == MIN_SUM:                                            # 2.1
            R = ro._check_step(T, Q[A], ssign_all[A], alpha)
        else:
            mask = np.broadcast_to(T.rmask[None], (len(A),) + T.rmask.shape)
            R = lo._sp_rows(Q[A], mask, syn[A].astype(np.uint8))
        with np.errstate(invalid="ignore"):
            Vn = ro._column_sums(T, R) + W[A]                             # 2.2
            Qn = Vn[:, T.ridx] - R                                        # 2.3
            if variant == MIN_SUM:
                Qn = np.clip(Qn, -clip, clip)
        Q[A] = np.where(T.rmask, Qn, 0.0)
        V[A] = Vn                                                         # 2.4
        total[A] += 1
        t[A] += 1
        hard = Vn < 0.0                                                   # 2.5
        ok = np.all((hard[:, T.ridx] & T.rmask).sum(axis=2) % 2 == syn[A], axis=1)
        conv[A[ok]] = True
        done[A[ok]] = True
        for k in np.flatnonzero(~ok & (t[A] >= Tr)):                      # rule 3: the round ends without a solution
            b = A[k]
            if rounds[b] == max_rounds:
                done[b] = True
                continue
            v = choose(V[b], D[b], col_weight)
            if v < 0:
                done[b] = True
                continue
            W[b, v] = -dl if V[b, v] < 0.0 else dl
            D[b, v] = True
            rounds[b] += 1
            t[b] = 0
    cls = np.where(~conv, 2, np.where(rounds > 0, 1, 0)).astype(np.int8)
    return dict(hard=(V < 0.0).astype(np.uint8), llr=V, converged=conv, iters=total, rounds=rounds, cls=cls,
                decimated=D, working_prior=W)


def gd_decode(H, syndrome, prior, iters_per_round, max_rounds, decim_llr, variant=MIN_SUM, alpha=1.0, clip_llr=20.0):
    """One record: the dict of ``gd_decode_batch`` with the leading axis removed."""
    r = gd_decode_batch(H, np.asarray(syndrome).reshape(1, -1), prior, iters_per_round, max_rounds, decim_llr, variant,
                        alpha, clip_llr)
    return {k: v[0] for k, v in r.items()}


def classes(r):
    """Counts of the three classes: solved in round 0, solved after >= 1 decimation, never solved."""
    return dict(round0=int((r["cls"] == 0).sum()), later=int((r["cls"] == 1).sum()), never=int((r["cls"] == 2).sum()))
