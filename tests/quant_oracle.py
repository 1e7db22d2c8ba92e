"""The numpy statement of fixed-point min-sum BP (include/qbp.h, qbp_quant_configure, rules 1-7): vectorised integer
arrays over the batch, a plain loop over the checks and the variables, every rule written as the header words it.  It
shares no code with the kernel; tests/test_quant_cpu.py ties it to the reference-generated min-sum goldens and to
``oracle.decode_batch``."""
import numpy as np


def M_of(bits):
    return (1 << (int(bits) - 1)) - 1


def quantize(prior, bits, scale):
    """Rule 1: int64 P -- 0 for a NaN, else clamp(rint(prior * scale), -M, M); +-inf clamp to +-M."""
    M = M_of(bits)
    out = np.zeros(np.shape(prior), np.int64)
    flat = out.reshape(-1)
    for i, x in enumerate(np.asarray(prior, np.float64).reshape(-1)):
        y = np.float64(x) * np.float64(scale)           # one IEEE double multiply
        if np.isnan(y):
            flat[i] = 0
        elif y >= M:
            flat[i] = M
        elif y <= -M:
            flat[i] = -M
        else:
            flat[i] = int(np.rint(y))                   # half to even; |y| < M, so the result is within [-M, M]
    return out


def decode_batch(H, syndromes, prior, max_iter, bits, scale, alpha_num, alpha_shift, beta):
    """Rules 2-7 on B syndromes uint8[B, m] -> (hard uint8[B, n], converged bool[B], iters int32[B],
    posterior_q int32[B, n], llr float64[B, n]).  Every record runs all iterations and keeps the outputs of its first
    converged one, which is also what stopping there gives."""
    H = (np.asarray(H) != 0)
    m, n = H.shape
    syn = np.asarray(syndromes).astype(np.int64) & 1
    B = syn.shape[0]
    M = M_of(bits)
    P = quantize(prior, bits, scale)
    assert P.shape == (n,)
    rows = [np.flatnonzero(H[c]) for c in range(m)]
    # messages as dense [B, m, n] integer arrays, read only where H is set
    Q = np.zeros((B, m, n), np.int64)
    for c in range(m):
        Q[:, c, rows[c]] = P[rows[c]]                                   # rule 2
    R = np.zeros((B, m, n), np.int64)
    Hi = H.astype(np.int64)
    done = np.zeros(B, bool)
    out_V = np.zeros((B, n), np.int64)
    out_it = np.full(B, max_iter - 1, np.int32)
    V = np.zeros((B, n), np.int64)
    for t in range(max_iter):
        for c in range(m):                                              # rule 3
            vs = rows[c]
            q = Q[:, c, vs]                                             # [B, d]
            for j, v in enumerate(vs):
                others = np.delete(q, j, axis=1)
                neg = (syn[:, c] + (others < 0).sum(axis=1)) & 1
                mag = np.abs(others).min(axis=1) if others.shape[1] else np.full(B, M, np.int64)
                mag = np.maximum(((mag * alpha_num) >> alpha_shift) - beta, 0)
                R[:, c, v] = np.where(neg == 1, -mag, mag)
        V = P[None, :] + (R * Hi[None]).sum(axis=1)                     # rule 4
        assert np.abs(V).max(initial=0) < 2 ** 31
        Q = np.clip(V[:, None, :] - R, -M, M) * Hi[None]
        hard = (V < 0).astype(np.int64)                                 # rule 5
        ok = ((hard @ Hi.T) & 1 == syn).all(axis=1)
        first = ok & ~done
        out_V[first] = V[first]                                         # rule 6
        out_it[first] = t
        done |= ok
    out_V[~done] = V[~done]
    return ((out_V < 0).astype(np.uint8), done, out_it, out_V.astype(np.int32), out_V.astype(np.float64))


def decode_batch_edges(H, syndromes, prior, max_iter, bits, scale, alpha_num, alpha_shift, beta):
    """decode_batch with the messages stored per entry of H, int64 [B, E] in row-major order of the entries, for
    matrices whose dense [B, m, n] arrays are too large: the same rules 2-7 in the header's wording ("all the other
    entries of the row" for every entry on its own), plain loops over the rows and the columns of the entry lists, the
    same outputs.  tests/test_quant_cpu.py asserts that the two are equal on every case of quant_cases."""
    H = (np.asarray(H) != 0)
    m, n = H.shape
    syn = np.asarray(syndromes).astype(np.int64) & 1
    B = syn.shape[0]
    M = M_of(bits)
    P = quantize(prior, bits, scale)
    assert P.shape == (n,)
    edge_row, edge_col = np.nonzero(H)                                  # row after row, columns ascending
    E = len(edge_row)
    row_edges = [np.flatnonzero(edge_row == c) for c in range(m)]       # the entries of row c
    col_edges = [np.flatnonzero(edge_col == v) for v in range(n)]       # the entries of column v
    Q = np.tile(P[edge_col], (B, 1))                                    # rule 2
    R = np.zeros((B, E), np.int64)
    done = np.zeros(B, bool)
    out_V = np.zeros((B, n), np.int64)
    out_it = np.full(B, max_iter - 1, np.int32)
    V = np.zeros((B, n), np.int64)
    for t in range(max_iter):
        for c in range(m):                                              # rule 3
            es = row_edges[c]
            for e in es:
                others = Q[:, es[es != e]]                              # [B, d - 1]
                neg = (syn[:, c] + (others < 0).sum(axis=1)) & 1
                mag = np.abs(others).min(axis=1) if others.shape[1] else np.full(B, M, np.int64)
                mag = np.maximum(((mag * alpha_num) >> alpha_shift) - beta, 0)
                R[:, e] = np.where(neg == 1, -mag, mag)
        for v in range(n):                                              # rule 4
            es = col_edges[v]
            V[:, v] = P[v] + R[:, es].sum(axis=1)
            Q[:, es] = np.clip(V[:, v, None] - R[:, es], -M, M)
        assert np.abs(V).max(initial=0) < 2 ** 31
        hard = (V < 0).astype(np.int64)                                 # rule 5
        ok = np.ones(B, bool)
        for c in range(m):
            ok &= (hard[:, edge_col[row_edges[c]]].sum(axis=1) & 1) == syn[:, c]
        first = ok & ~done
        out_V[first] = V[first]                                         # rule 6
        out_it[first] = t
        done |= ok
    out_V[~done] = V[~done]
    return ((out_V < 0).astype(np.uint8), done, out_it, out_V.astype(np.int32), out_V.astype(np.float64))
