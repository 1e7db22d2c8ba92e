"""numpy statement of the per-column Monte-Carlo sampler (include/qbp.h, qbp_mc_run_probs) -- TEST INFRASTRUCTURE.

Trial t, column v: bit = XOR over d < draws of [word v % 4 of Philox4x32-10(counter (t lo, t hi, v / 4, d), key
seed) < thr[v]], thr[v] = floor(p_v 2^32) clamped to [0, 2^32 - 1].
"""
import numpy as np

_MASK = np.uint64(0xFFFFFFFF)


def thresholds(probs):
    t = np.floor(np.asarray(probs, np.float64) * 4294967296.0)
    return np.clip(t, 0.0, 4294967295.0).astype(np.uint64)


def philox4x32_10(c, key):
    """c: four uint64 arrays holding 32-bit words; key: (k0, k1).  Returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & _MASK for x in c)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = c0 * np.uint64(0xD2511F53)
        p1 = c2 * np.uint64(0xCD9E8D57)
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & _MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & _MASK
    return c0, c1, c2, c3


def errors_probs(probs, draws, seed, trial_begin, T):
    """Errors uint8[T, n] of trials trial_begin .. + T under per-column probabilities."""
    thr = thresholds(probs)
    n = thr.size
    n4 = (n + 3) // 4
    t = (np.uint64(trial_begin) + np.arange(T, dtype=np.uint64))[:, None]
    g = np.arange(n4, dtype=np.uint64)[None, :]
    t_lo, t_hi = np.broadcast_to(t & _MASK, (T, n4)), np.broadcast_to(t >> np.uint64(32), (T, n4))
    g = np.broadcast_to(g, (T, n4))
    seed = int(seed)
    out = np.zeros((T, n), np.uint8)
    for d in range(int(draws)):
        words = philox4x32_10((t_lo, t_hi, g, np.full((T, n4), d, np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
        w = np.stack(words, axis=-1).reshape(T, 4 * n4)[:, :n]
        out ^= (w < thr[None, :]).astype(np.uint8)
    return out
