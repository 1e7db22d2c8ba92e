"""numpy statement of the Pauli-frame simulator (include/qbp.h, qbp_frame_*) -- TEST INFRASTRUCTURE.

One byte per record and frame bit.  One record: X and Z frame bits per qubit, all zero at the start; RZ / RX clear both
bits of the target; CX a->b: X[b] ^= X[a], then Z[a] ^= Z[b]; MZ records X[q], MX records Z[q]; a fault with Pauli P on
q: X[q] ^= P & 1, Z[q] ^= P >> 1 & 1; a detector or observable is the XOR of its record bits.  Sites are the targets
(pairs) of the noise ops in op order, then target order; site j has K faults with codes 1 .. K (XERR: the Pauli X,
ZERR: the Pauli Z, DEP1: code = Pauli, 1 X, 2 Z, 3 Y; DEP2: code & 3 on the first qubit, code >> 2 on the second);
faults are numbered by site, then code.

Injectors.  Enumeration: record f is fault f alone.  Sampling: for site j of shot t, u = word j % 4 of
Philox4x32-10(counter (t lo, t hi, j / 4, PHILOX_STREAM), key seed); the site faults iff u < thr =
floor(rate[class] 2^32), with code 1 + (u K) // thr.

``defect=`` names a deliberately WRONG statement (tests assert that each changes the output on a named case):
  "z_forward"     Z propagated control -> target (Z[b] ^= Z[a]) instead of target -> control
  "reset_keeps"   a reset does not clear the frame bits
  "y_as_x"        the Pauli Y treated as X
  "swap_pair"     the two halves of a pair code exchanged
  "mx_reads_x"    MX records the X bit
  "final_no_prev" a detector of more than two records (memory_experiment's final ones) loses its last record, Z_{T-1}
"""
import numpy as np

from dem_sampler import philox4x32_10, thresholds

PHILOX_STREAM = 5                # counter word 3 (QBP_FRAME_PHILOX_STREAM)
_MASK = np.uint64(0xFFFFFFFF)
DEFECTS = ("z_forward", "reset_keeps", "y_as_x", "swap_pair", "mx_reads_x", "final_no_prev")
K_OF = dict(XERR=1, ZERR=1, DEP1=3, DEP2=15)


def sites_of(circuit):
    """[(kind, q0, q1, rate class, K)] in site order, and site_base (one entry more: the number of faults)."""
    out = []
    for kind, t, cls in circuit.ops:
        if kind == "DEP2":
            out.extend((kind, a, b, cls, 15) for a, b in zip(t[::2], t[1::2]))
        elif kind in K_OF:
            out.extend((kind, q, -1, cls, K_OF[kind]) for q in t)
    base = np.concatenate([[0], np.cumsum([s[4] for s in out])]).astype(np.int64)
    return out, base


def _pauli(kind, code, defect):
    """Site codes -> 4-bit Paulis (bits 0-1 on the first qubit, 2-3 on the second)."""
    code = np.asarray(code, np.int64)
    p = np.full_like(code, 1) if kind == "XERR" else np.full_like(code, 2) if kind == "ZERR" else code.copy()
    if defect == "swap_pair" and kind == "DEP2":
        p = (p >> 2) | ((p & 3) << 2)
    if defect == "y_as_x":
        lo, hi = p & 3, p >> 2
        p = np.where(lo == 3, 1, lo) | (np.where(hi == 3, 1, hi) << 2)
    return p


def propagate(circuit, R, inject, defect=None):
    """``R`` records at once -> measurement records uint8 [R, n_records].  ``inject(j)`` -> (record indices, codes) of
    the faults at site j."""
    assert defect is None or defect in DEFECTS
    X = np.zeros((circuit.nq, R), np.uint8)
    Z = np.zeros((circuit.nq, R), np.uint8)
    rec = np.zeros((circuit.n_records, R), np.uint8)
    r = j = 0
    for kind, t, cls in circuit.ops:
        if kind in ("RZ", "RX"):
            if defect != "reset_keeps":
                X[list(t)] = 0
                Z[list(t)] = 0
        elif kind == "CX":
            for a, b in zip(t[::2], t[1::2]):
                X[b] ^= X[a]
                if defect == "z_forward":
                    Z[b] ^= Z[a]
                else:
                    Z[a] ^= Z[b]
        elif kind == "MZ":
            for q in t:
                rec[r] = X[q]
                r += 1
        elif kind == "MX":
            for q in t:
                rec[r] = X[q] if defect == "mx_reads_x" else Z[q]
                r += 1
        else:
            targets = list(zip(t[::2], t[1::2])) if kind == "DEP2" else [(q, -1) for q in t]
            for a, b in targets:
                idx, code = inject(j)
                j += 1
                if len(idx) == 0:
                    continue
                p = _pauli(kind, code, defect).astype(np.uint8)
                X[a, idx] ^= p & 1
                Z[a, idx] ^= (p >> 1) & 1
                if b >= 0:
                    X[b, idx] ^= (p >> 2) & 1
                    Z[b, idx] ^= (p >> 3) & 1
    return np.ascontiguousarray(rec.T)


def assemble(circuit, rec, defect=None):
    """Measurement records [R, n_records] -> (det uint8 [R, m], obs uint8 [R, k])."""
    def xor(lists, cut):
        out = np.zeros((rec.shape[0], len(lists)), np.uint8)
        for c, idx in enumerate(lists):
            idx = list(idx)
            if cut and len(idx) > 2:
                idx = idx[:-1]
            for i in idx:
                out[:, c] ^= rec[:, i]
        return out
    return xor(circuit.detectors, defect == "final_no_prev"), xor(circuit.observables, False)


def pack(det, obs):
    """(det [R, m], obs [R, k]) -> (b8 rows uint8 [R, ceil(m / 8)], masks uint64 [R]): the layout of the library."""
    bits = np.packbits(det, axis=1, bitorder="little") if det.shape[1] else np.zeros((det.shape[0], 0), np.uint8)
    masks = np.zeros(det.shape[0], np.uint64)
    for l in range(obs.shape[1]):
        masks |= obs[:, l].astype(np.uint64) << np.uint64(l)
    return np.ascontiguousarray(bits), masks


def faults(circuit, begin=0, T=None, defect=None):
    """Enumeration: records ``begin .. begin + T - 1`` are those faults -> (det [T, m], obs [T, k])."""
    sites, base = sites_of(circuit)
    T = int(base[-1]) - begin if T is None else int(T)

    def inject(j):
        f = np.arange(max(base[j], begin), min(base[j + 1], begin + T), dtype=np.int64)
        return f - begin, f - base[j] + 1
    return assemble(circuit, propagate(circuit, T, inject, defect), defect)


def sample_faults(circuit, rates, seed, shot_begin, T):
    """The sampler alone: per site the (shot indices relative to shot_begin, codes) of its faults."""
    sites, _ = sites_of(circuit)
    S = len(sites)
    n4 = (S + 3) // 4
    thr = np.zeros(4 * n4, np.uint64)
    K = np.zeros(4 * n4, np.uint64)
    thr[:S] = thresholds([rates[s[3]] for s in sites])
    K[:S] = [s[4] for s in sites]
    seed = int(seed)
    hits = [[] for _ in range(S)]
    step = max(1, (1 << 22) // max(n4, 1))
    for a in range(0, T, step):
        n = min(step, T - a)
        t = ((np.arange(n, dtype=np.uint64) + np.uint64(a)) + np.uint64(shot_begin))[:, None]    # (wraps mod 2^64)
        g = np.broadcast_to(np.arange(n4, dtype=np.uint64)[None, :], (n, n4))
        words = philox4x32_10((np.broadcast_to(t & _MASK, (n, n4)), np.broadcast_to(t >> np.uint64(32), (n, n4)), g,
                               np.full((n, n4), PHILOX_STREAM, np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
        u = np.stack(words, axis=-1).reshape(n, 4 * n4)
        rows, cols = np.nonzero(u < thr[None, :])
        code = 1 + (u[rows, cols] * K[cols]) // thr[cols]
        order = np.argsort(cols, kind="stable")
        rows, cols, code = rows[order], cols[order], code[order]
        cut = np.searchsorted(cols, np.arange(S + 1))
        for j in np.unique(cols):
            hits[j].append((rows[cut[j]:cut[j + 1]] + a, code[cut[j]:cut[j + 1]].astype(np.int64)))
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    return [(np.concatenate([h[0] for h in hs]), np.concatenate([h[1] for h in hs])) if hs else empty for hs in hits]


def sample(circuit, rates, seed, shot_begin, T, defect=None):
    """Sampling: shots ``shot_begin .. shot_begin + T - 1`` -> (det [T, m], obs [T, k]).  ``rates``: per class."""
    hits = sample_faults(circuit, np.asarray(rates, np.float64), seed, shot_begin, int(T))
    return assemble(circuit, propagate(circuit, int(T), lambda j: hits[j], defect), defect)


def merge(det, obs):
    """The column merge: faults that flip nothing are dropped, equal (detectors, observables) merge, columns keep the
    order of first appearance -> (H uint8 [m, n], L uint8 [k, n], fault_column int64 [faults], -1 = dropped)."""
    cols, col_of = {}, np.full(det.shape[0], -1, np.int64)
    for f in range(det.shape[0]):
        if not det[f].any() and not obs[f].any():
            continue
        key = det[f].tobytes() + obs[f].tobytes()
        col_of[f] = cols.setdefault(key, len(cols))
    first = np.full(len(cols), -1, np.int64)
    for f in range(det.shape[0] - 1, -1, -1):
        if col_of[f] >= 0:
            first[col_of[f]] = f
    return np.ascontiguousarray(det[first].T), np.ascontiguousarray(obs[first].T), col_of
