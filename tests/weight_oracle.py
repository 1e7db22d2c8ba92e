"""numpy statement of the fixed-weight Monte-Carlo sampler (include/qbp.h, qbp_mc_run_weight) -- TEST INFRASTRUCTURE.

Trial t, weight w, n columns: Floyd's subset sampling.  S starts empty; for i = 0 .. w - 1: j = n - w + i, r = word
i % 4 of Philox4x32-10(counter (t lo, t hi, i / 4, 2), key seed), u = (r (j + 1)) >> 32; add j to S if u is in S
already, else add u.  errors[t][v] = 1 iff v in S.
"""
import numpy as np

from dem_sampler import philox4x32_10

_MASK = np.uint64(0xFFFFFFFF)


def errors_weight(n, w, seed, trial_begin, T):
    """Errors uint8[T, n] of trials trial_begin .. + T, every row of weight exactly w."""
    n, w, T, seed = int(n), int(w), int(T), int(seed)
    if not 0 <= w <= n:
        raise ValueError(f"weight {w} out of [0, {n}]")
    out = np.zeros((T, n), np.uint8)
    t = np.uint64(trial_begin) + np.arange(T, dtype=np.uint64)
    rows = np.arange(T)
    words = None
    for i in range(w):
        if i % 4 == 0:
            words = philox4x32_10((t & _MASK, t >> np.uint64(32), np.full(T, i // 4, np.uint64),
                                   np.full(T, 2, np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
        j = n - w + i
        u = ((words[i % 4] * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        taken = out[rows, u] != 0
        out[rows, np.where(taken, j, u)] = 1
    return out
