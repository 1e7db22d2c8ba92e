"""The numpy statement of sliding-window decoding (include/qbp.h, "Sliding-window decoding": the rule).  It owns no
decoder: ``decode(Hk, syndromes, prior) -> (hard, conv, it, llr)`` and ``osd(Hk, syndromes, llr, hard) -> hard`` are
passed in, so the same statement composes the CPU oracle or separate ordinary GPU decoders on the H_k."""
import numpy as np


def dense(H):
    return np.asarray(H.todense() if hasattr(H, "todense") else H).astype(np.uint8)


def plan(H, check_round, W, F):
    """The partition as ``_lib.window_plan`` returns it, plus ``R`` and ``var_round``."""
    H = dense(H)
    m, n = H.shape
    cr = np.asarray(check_round, np.int64)
    assert cr.shape == (m,) and (cr >= 0).all() and W >= 1 and 1 <= F <= W
    R = int(cr.max()) + 1
    var_round = np.array([cr[H[:, v] != 0].min() if H[:, v].any() else 0 for v in range(n)], np.int64)
    k_last = 0
    while k_last * F + W < R:
        k_last += 1
    K = k_last + 1
    check_ptr, var_ptr, checks, vars_, commit, cls, seen = [0], [0], [], [], [], [], []
    for k in range(K):
        lo, hi = k * F, min(k * F + W, R)
        C = np.flatnonzero((cr >= lo) & (cr < hi))
        U = np.flatnonzero((var_round >= lo) & (var_round < hi))
        checks += C.tolist()
        vars_ += U.tolist()
        commit += (np.ones(U.size, bool) if k == K - 1 else var_round[U] < lo + F).astype(np.uint8).tolist()
        check_ptr.append(len(checks))
        var_ptr.append(len(vars_))
        if C.size == 0 or U.size == 0:                # a skipped window (rule 0)
            cls.append(-1)
            continue
        Hk = H[np.ix_(C, U)]
        for i, other in enumerate(seen):
            if other.shape == Hk.shape and np.array_equal(other, Hk):
                cls.append(i)
                break
        else:
            cls.append(len(seen))
            seen.append(Hk)
    return dict(K=K, R=R, var_round=var_round, check_ptr=np.array(check_ptr, np.int32), checks=np.array(checks, np.int32),
                var_ptr=np.array(var_ptr, np.int32), vars=np.array(vars_, np.int32), commit=np.array(commit, np.uint8),
                cls=np.array(cls, np.int32))


def windows(H, P):
    """(C_k, U_k, commit mask over U_k, H_k) of every window of a plan."""
    H = dense(H)
    for k in range(P["K"]):
        C = P["checks"][P["check_ptr"][k]:P["check_ptr"][k + 1]]
        U = P["vars"][P["var_ptr"][k]:P["var_ptr"][k + 1]]
        yield C, U, P["commit"][P["var_ptr"][k]:P["var_ptr"][k + 1]].astype(bool), np.ascontiguousarray(H[np.ix_(C, U)])


def decode(H, check_round, W, F, syndromes, prior, decode, osd=None, P=None):
    """-> (correction uint8[B, n], converged bool[B], iters int32[B], llr float64[B, n], window_fails int32[B])."""
    H = dense(H)
    m, n = H.shape
    P = plan(H, check_round, W, F) if P is None else P
    r = np.array(syndromes, np.uint8) & 1
    B = r.shape[0]
    prior = np.asarray(prior, np.float64)
    x = np.zeros((B, n), np.uint8)
    llr_out = np.zeros((B, n), np.float64)
    iters = np.zeros(B, np.int32)
    fails = np.zeros(B, np.int32)
    for C, U, M, Hk in windows(H, P):
        if C.size == 0 or U.size == 0:                # rule 0: nothing decoded or counted
            x[:, U[M]] = 0
            llr_out[:, U[M]] = prior[U[M]]
            continue
        hard, conv, it, llr = decode(Hk, np.ascontiguousarray(r[:, C]), np.ascontiguousarray(prior[U]))
        hard = np.array(hard, np.uint8)
        conv = np.asarray(conv, bool)
        bad = np.flatnonzero(~conv)
        if osd is not None and bad.size:
            hard[bad] = osd(Hk, np.ascontiguousarray(r[bad][:, C]), np.ascontiguousarray(llr[bad]),
                            np.ascontiguousarray(hard[bad]))
        x[:, U[M]] = hard[:, M]
        llr_out[:, U[M]] = llr[:, M]
        r ^= ((hard[:, M].astype(np.int64) @ H[:, U[M]].T.astype(np.int64)) & 1).astype(np.uint8)
        iters += np.asarray(it, np.int32)
        fails += (~conv).astype(np.int32)
    return x, ~r.any(axis=1), iters, llr_out, fails


# ---- the matrices of the window tests ---------------------------------------------------------------------------------
def spacetime(Hx, rounds):
    """[I_T (x) Hx | I + shift] and its check_round: the phenomenological matrix of Hx over ``rounds`` rounds."""
    Hx = np.asarray(Hx, np.uint8)
    m0, n0 = Hx.shape
    T = int(rounds)
    H = np.zeros((m0 * T, n0 * T + m0 * T), np.uint8)
    for t in range(T):
        H[t * m0:(t + 1) * m0, t * n0:(t + 1) * n0] = Hx
    for j in range(m0 * T):
        H[j, n0 * T + j] = 1
        if j + m0 < m0 * T:
            H[j + m0, n0 * T + j] = 1
    return H, (np.arange(m0 * T) // m0).astype(np.int32)


def irregular(seed=20251):
    """24 x 50, six rounds in shuffled check order: round 2 has no check (so no variable starts there and the window
    that commits round 2 alone commits nothing), columns span one to three of the rounds that have checks, the first
    column of every such round stays inside it, and the last column is empty."""
    rng = np.random.default_rng(seed)
    present = [0, 1, 3, 4, 5]
    cr = np.array([0] * 5 + [1] * 5 + [3] * 5 + [4] * 5 + [5] * 4, np.int32)
    cr = cr[rng.permutation(24)]
    H = np.zeros((24, 50), np.uint8)
    for v in range(49):
        start = v % 5
        for i in range(start, min(start + 1 + (v // 5) % 3, 5)):
            H[rng.choice(np.flatnonzero(cr == present[i])), v] = 1
    return H, cr
