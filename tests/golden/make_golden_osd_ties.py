#!/usr/bin/env python3
"""OSD-0 on TIED reliabilities, produced by RUNNING THE REAL REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_osd_ties.py

  decoding/OSD.py:3   performOSD(H, syndrome, llr, hard)     ordering = np.argsort(np.abs(llr))     (:10-11)

Where |llr| values are equal the reference's column order is whatever its numpy build's argsort leaves (an unstable
sort), and its solution depends on it.  So every record stores, besides (syndrome, llr, hard) and the reference's
solution, the reference's `ordering` itself (uint16): qbp_osd_batch_ordered on that order must return that solution,
on any host.  H is not stored: codes.load_code / the spaceTime.py formula give it (checked below).

Groups <tag>/...: steane, 72, 144, 288.  `kind` per record:
  0 all |llr| equal (1.0)                           1 three magnitudes {0.5, 1, 2}, random signs
  2 round(2 N(0,1)): many ties, +-0.0               3 blocks of 8 columns with one value each, random signs
  4 reference BP output after ONE iteration from a uniform prior, BP not converged (real ties)
  5 three magnitudes with NaN, +inf, -inf entries
24 records per kind (6 of kind 5); syndromes of Bernoulli(0.06) errors (steane 0.2), hard = (llr < 0).
  6 (72, 144, 288 only: steane's Hx has full row rank) 8 random syndromes OUTSIDE the column space, three magnitudes --
    there the output depends on the reference's row swaps as well.
Group st144: the 864 x 2592 space-time matrix of [[144,12,12]] over 12 rounds, 8 records of kind 1 (p = 0.02).
Group ka: known-answer vectors -- `ka/llr<n>` and `ka/order<n>` = np.argsort(np.abs(.)) as THIS numpy build computed
it; a host whose numpy sorts them to the same orders shares the reference's tie order (tests gate on that).

Condition asserted here (and re-asserted by tests/test_osd_ordered_cpu.py): in every group but steane at least half
of the records of kinds 1 and 2 have a reference solution different from the column-index tie rule's (oracle.osd0).
"""
import contextlib
import io
import os
import sys

import numpy as np

REF = os.environ.get("QLDPC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, REF)
with contextlib.redirect_stdout(io.StringIO()):
    from decoding.beliefPropagation import performBeliefPropagationFast
    from decoding import OSD as ref_osd
sys.path.insert(1, ROOT)
from oracle import oracle  # noqa: E402
from qldpc_amd import codes  # noqa: E402

SEEDS = {"steane": 20261017, "72": 20261017, "144": 20261017, "288": 20261017, "st144": 20261017}
FILES = {"steane": "steane", "72": "[[72, 12, 6]]", "144": "[[144, 12, 12]]", "288": "[[288, 12, 18]]"}


def reference_osd(H, s, l, h):
    """(ordering, solution) of the reference's performOSD: the ordering is read off its own gf2_elimination call."""
    seen = {}
    inner = ref_osd.gf2_elimination

    def spy(Hp, rs):
        seen["Hp"] = Hp
        return inner(Hp, rs)

    ref_osd.gf2_elimination = spy
    try:
        sol = ref_osd.performOSD(H, s, l, h)
    finally:
        ref_osd.gf2_elimination = inner
    ordering = np.argsort(np.abs(l))            # the same call on the same array in the same process ...
    assert np.array_equal(seen["Hp"], H[:, ordering])    # ... and checked against what performOSD did
    return ordering, np.asarray(sol)


def three(rng, n):
    return rng.choice([0.5, 1.0, 2.0], size=n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)


def llr_of_kind(kind, rng, n, H, s, p):
    if kind == 0:
        return np.ones(n)
    if kind == 1:
        return three(rng, n)
    if kind == 2:
        return np.round(2.0 * rng.standard_normal(n))        # -0.0 where a small negative number rounds
    if kind == 3:
        vals = np.repeat(rng.normal(0, 3, (n + 7) // 8), 8)[:n]
        return np.abs(vals) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if kind == 5:
        l = three(rng, n)
        pos = rng.choice(n, 3, replace=False)
        l[pos[0]], l[pos[1]], l[pos[2]] = np.inf, -np.inf, np.nan
        return l
    raise ValueError(kind)


def in_column_space(H, s):
    A = np.concatenate([H % 2, s[:, None]], axis=1).astype(np.uint8)
    r = 0
    for c in range(H.shape[1]):
        nz = np.flatnonzero(A[r:, c])
        if len(nz) == 0:
            continue
        p = r + nz[0]
        A[[r, p]] = A[[p, r]]
        o = np.flatnonzero(A[:, c])
        o = o[o != r]
        A[o] ^= A[r]
        r += 1
        if r == H.shape[0]:
            break
    return not A[r:, -1].any()


def group(tag, H, kinds, p, rng, out):
    m, n = H.shape
    rec = {k: [] for k in ("syndromes", "llr", "hard", "ordering", "solution", "kind")}

    def add(s, l, h, kind):
        ordering, sol = reference_osd(H, s, l, h)
        rec["syndromes"].append(s); rec["llr"].append(l); rec["hard"].append(h)
        rec["ordering"].append(ordering); rec["solution"].append(sol); rec["kind"].append(kind)

    for kind, count in kinds:
        made = 0
        while made < count:
            if kind == 6:
                s = (rng.random(m) < 0.5).astype(np.int64)
                if in_column_space(H, s):
                    continue
                l = three(rng, n)
                h = (rng.random(n) < 0.3).astype(np.int64)
            else:
                e = (rng.random(n) < p).astype(np.int64)
                s = (e @ H.T) % 2
                if kind == 4:
                    h, conv, l = performBeliefPropagationFast(H, s, np.full(n, np.log((1 - p) / p)), verbose=False,
                                                              maxIter=1)
                    if conv:
                        continue
                    l = np.asarray(l, np.float64)
                    h = np.asarray(h).astype(np.int64)
                else:
                    l = llr_of_kind(kind, rng, n, H, s, p)
                    h = (l < 0).astype(np.int64)
            add(s, l, h, kind)
            made += 1
    sol = np.array(rec["solution"], np.uint8)
    kind = np.array(rec["kind"], np.uint8)
    out[f"{tag}/syndromes"] = np.array(rec["syndromes"], np.uint8)
    out[f"{tag}/llr"] = np.array(rec["llr"], np.float64)
    out[f"{tag}/hard"] = np.array(rec["hard"], np.uint8)
    out[f"{tag}/ordering"] = np.array(rec["ordering"], np.uint16)
    out[f"{tag}/solution"] = sol
    out[f"{tag}/kind"] = kind
    pick = np.flatnonzero((kind == 1) | (kind == 2))
    differ = sum(not np.array_equal(oracle.osd0(H, rec["syndromes"][i], rec["llr"][i], rec["hard"][i]), sol[i])
                 for i in pick)
    print(f"{tag}: {len(kind)} records; reference differs from the column-index rule on {differ} of {len(pick)} "
          f"records of kinds 1 and 2")
    if tag != "steane":
        assert 2 * differ >= len(pick), f"{tag}: change its seed"


def main():
    out = {}
    for tag, fname in FILES.items():
        H = np.load(os.path.join(REF, "codes", f"{fname}.npz"))["Hx"].astype(np.int64)
        assert np.array_equal(H, codes.load_code(fname).Hx)
        kinds = [(0, 24), (1, 24), (2, 24), (3, 24), (4, 24), (5, 6)] + ([(6, 8)] if tag != "steane" else [])
        group(tag, H, kinds, 0.2 if tag == "steane" else 0.06, np.random.default_rng(SEEDS[tag]), out)
    H144 = codes.load_code("[[144, 12, 12]]").Hx.astype(np.int64)
    mm, T = H144.shape[0], 12
    st = np.hstack([np.kron(np.eye(T, dtype=np.int64), H144),
                    (np.eye(mm * T, dtype=np.int64) + np.eye(mm * T, k=-mm, dtype=np.int64)) % 2])
    from spaceTime import spaceTimeMatrix
    assert np.array_equal(st, np.asarray(spaceTimeMatrix(H144, T)).astype(np.int64))
    group("st144", st, [(1, 8)], 0.02, np.random.default_rng(SEEDS["st144"]), out)
    rng = np.random.default_rng(7)
    for n in (7, 72, 144, 288, 2592):
        l = np.concatenate([three(rng, n)[: n // 2], np.round(2.0 * rng.standard_normal(n - n // 2))])
        out[f"ka/llr{n}"] = l
        out[f"ka/order{n}"] = np.argsort(np.abs(l)).astype(np.uint16)
    path = os.path.join(HERE, "osd_ties.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
