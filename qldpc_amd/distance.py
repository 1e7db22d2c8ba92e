"""Distance upper bounds on the GPU: a randomized information-set search over ``ker H`` (QDistRnd's algorithm;
``qbp_distance_search``, include/qbp.h states a trial).

``bound(H, L)``: the lightest vector of ``ker H`` found that a row of ``L`` detects -- for ``(Hx, Lx)`` or ``(Hz, Lz)``
of a CSS code one sector's distance bound, for ``H, L`` of a detector error model (``dem.load_dem``,
``dem.phenomenological``) the weight of the lightest undetectable logical fault found.  ``estimate(code)``: both
sectors of a ``codes.Code``; it fills in ``code.distance`` where that was None, which is what the Monte-Carlo entries
of ``mc`` ask of a code from ``codes.register``.  An upper bound only: every codeword returned is checked by the
library to lie in ``ker H``, but no number of trials proves that nothing lighter exists.

    python -m qldpc_amd.distance --code NAME_OR_NPZ --trials N [--seed S]
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import codes, gf2
from .mc import shard_range


def _dense(H) -> np.ndarray:
    H = H.toarray() if hasattr(H, "toarray") else np.asarray(H)
    return (H.astype(np.int64) & 1).astype(np.uint8)


def merge(a: dict, b: dict) -> dict:
    """Two ``bound`` results of disjoint trial ranges -> that of their union: histograms add, the best is the smaller
    ``(weight, trial)``."""
    def key(x):
        return (x["weight"], x["trial"]) if x["weight"] >= 0 else (np.inf, np.inf)
    out = dict(a if key(a) <= key(b) else b)
    out["hist"] = a["hist"] + b["hist"]
    out["trials"] = a["trials"] + b["trials"]
    return out


def bound(H, L, trials=4096, seed=0, device=None, rank=0, world=1) -> dict:
    """``trials`` trials of the search, global indices ``[0, trials)``, of which this rank runs its ``mc.shard_range``.
    Returns ``weight`` (-1: no trial found a vector ``L`` detects), ``codeword`` uint8[n] and ``logical`` (the mask:
    bit l = ``L[l] . codeword``; both None without a result), ``trial`` (the first trial that reached the weight, -1),
    ``hist`` int64[n + 1] (trials by the weight they found) and ``trials`` (trials run).  With ``world > 1`` the
    result is this rank's shard: ``merge`` joins shards, in any order.  A matrix beyond the kernel's limits (2048
    rows of ``ker H``, 160 KiB of LDS -- in effect n <= 16384: 10 bytes per sorted column, the columns rounded up to a
    power of two) raises the library's ``QbpError`` (``E_UNSUPPORTED``)."""
    from . import bp
    Hd = _dense(H)
    L = np.ascontiguousarray(_dense(L))
    G = gf2.nullspace(Hd)
    n = Hd.shape[1]
    begin, end = shard_range(int(trials), rank, world)
    if G.shape[0] == 0:                      # ker H = {0}: nothing to search, nothing to find
        return dict(weight=-1, codeword=None, logical=None, trial=-1, hist=np.zeros(n + 1, np.int64), trials=end - begin)
    dec = bp.decoder_for(H if hasattr(H, "toarray") else Hd, device=device)
    result, hist, codeword, mask = dec.distance_search(G, L, begin, end, seed=seed)
    return dict(weight=int(result[1]), codeword=codeword, logical=mask, trial=int(result[2]), hist=hist,
                trials=int(result[0]))


def estimate(code, trials=4096, seed=0, device=None) -> dict:
    """Both sectors of ``code`` (a ``codes.Code`` or a name ``codes.load_code`` knows): ``x`` = ``bound(Hx, Lx)``, ``z`` =
    ``bound(Hz, Lz)``, ``distance`` = the smaller weight (None when neither side found anything, e.g. k = 0).  Sets
    ``code.distance`` to it when that was None."""
    c = codes.load_code(code) if isinstance(code, str) else code
    Lx, Lz = (c.Lx, c.Lz) if c.Lx is not None and c.Lz is not None else codes.css_logicals(c.Hx, c.Hz)
    sides = {}
    for side, H, L in (("x", c.Hx, Lx), ("z", c.Hz, Lz)):
        if L.shape[0] == 0:
            sides[side] = dict(weight=-1, codeword=None, logical=None, trial=-1,
                               hist=np.zeros(c.n + 1, np.int64), trials=0)
        else:
            sides[side] = bound(H, L, trials=trials, seed=seed, device=device)
    found = [s["weight"] for s in sides.values() if s["weight"] >= 0]
    d = min(found) if found else None
    if c.distance is None and d is not None:
        c.distance = d
    return dict(x=sides["x"], z=sides["z"], distance=d)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m qldpc_amd.distance", description=__doc__.split("\n\n")[0])
    ap.add_argument("--code", required=True, help="a name codes.load_code knows, or a path ending in .npz (Hx, Hz)")
    ap.add_argument("--trials", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    code = codes.load_code(args.code)
    est = estimate(code, trials=args.trials, seed=args.seed)

    def side(s):
        return dict(weight=s["weight"], trial=s["trial"], trials=s["trials"],
                    hist={int(w): int(s["hist"][w]) for w in np.flatnonzero(s["hist"])})
    k = code.n - gf2.rank(code.Hx) - gf2.rank(code.Hz)
    print(json.dumps(dict(code=code.name, n=code.n, k=k, trials=args.trials, seed=args.seed, distance_bound=est["distance"],
                          x=side(est["x"]), z=side(est["z"]))))


if __name__ == "__main__":
    main()
