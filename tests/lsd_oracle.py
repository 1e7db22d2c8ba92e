"""Localized statistics decoding (BP+LSD) in plain numpy / Python: the statement that ``lsd_kernel`` reproduces bit for
bit (include/qbp.h, ``qbp_lsd_batch``, states the same rules in words).

Deliberately naive: the connected components of the Tanner graph induced on the active checks and variables are
recomputed from scratch in every round, and the elimination runs on a dense uint8 matrix ``[H | residual]`` of all m
rows.  Nothing here is shared with the kernel."""
import numpy as np

NAN_KEY = np.uint64(0x7FF8000000000000)


def order_keys(llr):
    """The sort key of OSD-0: |llr| by IEEE bit pattern (finite < inf < NaN), every NaN the same key."""
    a = np.abs(np.asarray(llr, np.float64))
    keys = a.view(np.uint64).copy()
    keys[np.isnan(a)] = NAN_KEY
    return keys


def ranks(llr):
    """rank[v]: position of column v in the ascending order of (key, v)."""
    keys = order_keys(llr)
    order = np.lexsort((np.arange(len(keys)), keys))
    rank = np.empty(len(keys), np.int64)
    rank[order] = np.arange(len(keys))
    return rank


def clusters_of(H, seeds, active):
    """Connected components of the graph induced on the active checks (seeds + neighbours of active variables) and the
    active variables -> list of (checks, variables), both sorted lists."""
    m, n = H.shape
    act_c = seeds.copy()
    for v in np.flatnonzero(active):
        act_c |= H[:, v].astype(bool)
    seen_c = np.zeros(m, bool)
    seen_v = np.zeros(n, bool)
    out = []
    for c0 in range(m):
        if not act_c[c0] or seen_c[c0]:
            continue
        checks, variables, todo = [], [], [("c", c0)]
        seen_c[c0] = True
        while todo:
            kind, x = todo.pop()
            if kind == "c":
                checks.append(x)
                for v in np.flatnonzero(H[x]):
                    if active[v] and not seen_v[v]:
                        seen_v[v] = True
                        todo.append(("v", v))
            else:
                variables.append(x)
                for c in np.flatnonzero(H[:, x]):
                    if not seen_c[c]:                      # (adjacent to an active variable: an active check)
                        seen_c[c] = True
                        todo.append(("c", c))
        out.append((sorted(checks), sorted(variables)))
    return out


def lsd_decode(H, syndrome, llr, hard, bits_per_step=1):
    """One record -> dict(solution uint8[n], stats int32[4] = {rounds, active variables, clusters, valid},
    e uint8[n], active bool[n], merged bool, skipped int (columns without a pivot), max_clusters int,
    pivot_rows int64[*] (the rows that serve as a pivot, ascending), cluster_lows int64[clusters] (the lowest check of
    every cluster at the end))."""
    H = np.asarray(H, np.uint8) & 1
    m, n = H.shape
    g = int(bits_per_step)
    hard = np.asarray(hard, np.uint8) & 1
    rank = ranks(llr)
    r = ((np.asarray(syndrome, np.int64) & 1) + H.astype(np.int64) @ hard) % 2
    A = np.concatenate([H, r.astype(np.uint8)[:, None]], axis=1)
    seeds = r.astype(bool)
    active = np.zeros(n, bool)
    is_pivot = np.zeros(m, bool)
    pivcol = -np.ones(m, np.int64)
    rounds, skipped, merged = 0, 0, False

    def invalid(cl):
        return any(A[c, n] and not is_pivot[c] for c in cl[0])

    cl = clusters_of(H, seeds, active)
    max_clusters = len(cl)
    for _ in range(n):
        new = set()
        for c in cl:
            if not invalid(c):
                continue
            cand = sorted({int(v) for chk in c[0] for v in np.flatnonzero(H[chk]) if not active[v]},
                          key=lambda v: rank[v])
            new.update(cand if g == 0 else cand[:g])
        if not new:
            break
        rounds += 1
        for v in new:
            active[v] = True
        for col in sorted(new, key=lambda v: rank[v]):
            rows = [i for i in range(m) if A[i, col] and not is_pivot[i]]
            if not rows:
                skipped += 1
                continue
            p = rows[0]
            for i in range(m):
                if i != p and A[i, col]:
                    A[i] ^= A[p]
            is_pivot[p] = True
            pivcol[p] = col
        before = len(cl)
        cl = clusters_of(H, seeds, active)
        merged |= len(cl) < before
        max_clusters = max(max_clusters, len(cl))
    e = np.zeros(n, np.uint8)
    for i in range(m):
        if is_pivot[i]:
            e[pivcol[i]] = A[i, n]
    valid = not any(invalid(c) for c in cl)
    stats = np.array([rounds, int(active.sum()), len(cl), int(valid)], np.int32)
    return dict(solution=hard ^ e, stats=stats, e=e, active=active, merged=merged, skipped=skipped,
                max_clusters=max_clusters, pivot_rows=np.flatnonzero(is_pivot),
                cluster_lows=np.array([c[0][0] for c in cl], np.int64))


def lsd_decode_batch(H, syndromes, llr, hard, bits_per_step=1):
    """B records -> dict(solution uint8[B, n], stats int32[B, 4], e, active, merged bool[B], skipped int[B], and the
    lists pivot_rows and cluster_lows of one array per record)."""
    recs = [lsd_decode(H, syndromes[b], llr[b], hard[b], bits_per_step) for b in range(len(syndromes))]
    n = np.asarray(H).shape[1]
    out = {}
    for k, dt, shape in (("solution", np.uint8, (0, n)), ("stats", np.int32, (0, 4)), ("e", np.uint8, (0, n)),
                         ("active", bool, (0, n)), ("merged", bool, (0,)), ("skipped", np.int64, (0,))):
        out[k] = np.array([x[k] for x in recs], dt) if recs else np.zeros(shape, dt)
    for k in ("pivot_rows", "cluster_lows"):
        out[k] = [x[k] for x in recs]
    return out


def presence(res):
    """How many records show each situation the tests want covered."""
    s = res["stats"]
    return dict(two_clusters=int((s[:, 2] >= 2).sum()), merged=int(res["merged"].sum()),
                three_rounds=int((s[:, 0] >= 3).sum()), skipped=int((res["skipped"] > 0).sum()),
                invalid=int((s[:, 3] == 0).sum()), trivial=int((s[:, 1] == 0).sum()))
