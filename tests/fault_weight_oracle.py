"""numpy statement of the fixed-weight FAULT sampler (include/qbp.h, qbp_mc_run_fault_weight) -- TEST INFRASTRUCTURE.

Inputs: N active sites with first_fault[s] (index into the circuit's fault numbering) and K[s] in {1, 3, 15};
fault_column[F] (-1 for a fault that flips nothing); n columns, weight w, seed, trial t.  Philox4x32-10 with the key
(lo32(seed), hi32(seed)); counter word 3 is 6.

  Sites (Floyd, over N):  for i = 0 .. w - 1:  j = N - w + i;  r = word i % 4 of the block at counter
      (lo32(t), hi32(t), i / 4, 6);  u = (r (j + 1)) >> 32;  s_i = j if u was already chosen, else u.
  Codes:  r' = word i % 4 of the block at counter (lo32(t), hi32(t), 0x80000000 | i / 4, 6);  c_i = (r' K[s_i]) >> 32;
      fault f_i = first_fault[s_i] + c_i.
  Row:  errors[t][v] = parity of the number of i with fault_column[f_i] == v.

Written trial by trial with a Python set for the chosen sites -- not the way qldpc_amd/circuit.py: fault_sets states
it -- so that the two can be held against each other.
"""
import numpy as np

from dem_sampler import philox4x32_10

PHILOX_STREAM = 6                # counter word 3 (QBP_FAULT_PHILOX_STREAM)
WEIGHT_MAX = 256                 # QBP_FAULT_WEIGHT_MAX
_MASK = np.uint64(0xFFFFFFFF)


def _words(t, blocks, top, seed):
    """uint64 [T, 4 * blocks]: the words of blocks 0 .. blocks - 1 of every trial; ``top``: the bit of the code stream."""
    T = t.size
    g = np.broadcast_to(np.arange(blocks, dtype=np.uint64)[None, :] | np.uint64(top), (T, blocks))
    lo = np.broadcast_to((t & _MASK)[:, None], (T, blocks))
    hi = np.broadcast_to((t >> np.uint64(32))[:, None], (T, blocks))
    words = philox4x32_10((lo, hi, g, np.full((T, blocks), PHILOX_STREAM, np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(words, axis=-1).reshape(T, 4 * blocks)


def picks(first_fault, K, w, seed, trial_begin, T):
    """(sites int64 [T, w], faults int64 [T, w]) of trials trial_begin .. + T, in step order."""
    first_fault, K = np.asarray(first_fault, np.int64), np.asarray(K, np.int64)
    N, w, T, seed = len(K), int(w), int(T), int(seed)
    if not 0 <= w <= min(N, WEIGHT_MAX):
        raise ValueError(f"weight {w} out of [0, {min(N, WEIGHT_MAX)}]")
    sites = np.zeros((T, w), np.int64)
    faults = np.zeros((T, w), np.int64)
    if w == 0 or T == 0:
        return sites, faults
    t = np.uint64(trial_begin) + np.arange(T, dtype=np.uint64)
    blocks = (w + 3) // 4
    r = _words(t, blocks, 0, seed)
    rc = _words(t, blocks, 0x80000000, seed)
    for b in range(T):
        chosen = set()
        for i in range(w):
            j = N - w + i
            u = (int(r[b, i]) * (j + 1)) >> 32
            s = j if u in chosen else u
            chosen.add(s)
            sites[b, i] = s
            faults[b, i] = int(first_fault[s]) + ((int(rc[b, i]) * int(K[s])) >> 32)
    return sites, faults


def rows_of_faults(faults, fault_column, n):
    """uint8 [T, n]: the parity per column of the faults of every trial; -1 contributes nothing."""
    faults = np.asarray(faults, np.int64)
    col = np.asarray(fault_column, np.int64)[faults]
    out = np.zeros((faults.shape[0], int(n)), np.uint8)
    for i in range(faults.shape[1]):
        hit = np.flatnonzero(col[:, i] >= 0)
        out[hit, col[hit, i]] ^= 1
    return out


def errors_fault_weight(first_fault, K, fault_column, n, w, seed, trial_begin, T):
    """Rows uint8 [T, n] of trials trial_begin .. + T."""
    return rows_of_faults(picks(first_fault, K, w, seed, trial_begin, T)[1], fault_column, n)
