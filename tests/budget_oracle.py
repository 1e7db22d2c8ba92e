"""Numpy statement of the semantics of ``qbp_mc_run_budgets`` (include/qbp.h) on top of the CPU oracle: the counter
table int64[K, 12] of a ladder of BP iteration limits b_0 < ... < b_{K-1} from ONE full decode.

A trial whose syndrome is first satisfied in 0-based iteration k (the oracle's ``iters`` of a converged trial):
  * rows with b_j > k   -- the prefix rule: converged, contributes k, classified on the outputs of the decode at
                           b_{K-1}, which stopped at k;
  * rows with b_j <= k  -- not converged at that limit: only these trials are decoded again, at max_iter = b_j, and
                           must come back unconverged with iteration index b_j - 1.
"""
import numpy as np

from oracle import oracle


def ladder_counters(H, Lx, distance, p, prior, trial_begin, trial_end, budgets, draws=1, seed=0, variant=0,
                    alpha=1.0, damping=1.0, clip_llr=20.0, osd=False):
    H = np.asarray(H).astype(np.int64)
    budgets = [int(b) for b in budgets]
    assert all(b >= 1 for b in budgets) and all(a < b for a, b in zip(budgets, budgets[1:]))
    T = trial_end - trial_begin
    errors = oracle.mc_errors(H.shape[1], p, draws, seed, trial_begin, T)
    syndromes = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    kw = dict(variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr)
    hard_f, conv_f, iters_f, llr_f = oracle.decode_batch(H, syndromes, prior, budgets[-1], **kw)
    k = np.where(conv_f, iters_f.astype(np.int64), np.iinfo(np.int64).max)      # first satisfied iteration
    table = np.zeros((len(budgets), 12), np.int64)
    for j, b in enumerate(budgets):
        hard, conv, iters, llr = hard_f.copy(), conv_f.copy(), iters_f.copy(), llr_f.copy()
        late = np.flatnonzero(k >= b)                     # not converged within b iterations
        if len(late) and b != budgets[-1]:
            h2, c2, i2, l2 = oracle.decode_batch(H, syndromes[late], prior, b, **kw)
            assert not c2.any() and (i2 == b - 1).all()
            hard[late], conv[late], iters[late], llr[late] = h2, c2, i2, l2
        assert not conv[late].any() and (iters[late] == b - 1).all() and conv[k < b].all()
        if osd:
            for i in late:
                hard[i] = oracle.osd0(H, syndromes[i], llr[i], hard[i])
        cnt = oracle.classify_trials(H, Lx, distance, errors, syndromes, hard, conv, iters)
        if osd:
            cnt[10] = sum(not np.array_equal((hard[i].astype(np.int64) @ H.T) % 2, syndromes[i]) for i in late)
        table[j] = cnt
    return table
