#!/usr/bin/env python3
"""Golden vectors for the memory-order rules of bp.dense_colsum_flags, produced by RUNNING THE REAL
REFERENCE decoders on the same inputs with H in C order and in Fortran order:

    python tests/golden/make_golden_layout.py <reference checkout>      (or QLDPC_REFERENCE=<checkout>)

  rework/decoding.py:77   performBeliefPropagationFast(H, s, prior, maxIter=30)                      "fast4"
  rework/decoding.py:5    performMinSum_Symmetric(..., alpha=0.8, damping=0.7, clip_llr=25.0)         "minsum"
  rework/decoding.py:131  performBeliefPropagation_Symmetric(..., alpha=0.9, damping=0.8, clip_llr=20.0) "sym"

Codes [[144,12,12]] and [[288,12,18]] (qldpc_amd/codes), six p = 0.06 syndromes each, non-uniform priors
(iteration 0 matters).  tests/test_column_order.py replays the oracle on these inputs.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from qldpc_amd import codes  # noqa: E402

FUNCS = {"fast4": ("performBeliefPropagationFast", {}),
         "minsum": ("performMinSum_Symmetric", dict(alpha=0.8, damping=0.7, clip_llr=25.0)),
         "sym": ("performBeliefPropagation_Symmetric", dict(alpha=0.9, damping=0.8, clip_llr=20.0))}
MAX_ITER = 30


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("QLDPC_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_golden_layout.py <reference checkout>")
    spec = importlib.util.spec_from_file_location("ref_rework_decoding", os.path.join(ref, "rework", "decoding.py"))
    rework = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rework)
    rng = np.random.default_rng(5)
    out = {"max_iter": np.int64(MAX_ITER)}
    for tag in ("144", "288"):
        code = codes.load_code(tag)
        p = 0.06
        prior = np.log((1 - p) / p) * rng.uniform(0.7, 1.3, code.n)
        syn = np.stack([((rng.random(code.n) < p).astype(np.int64) @ code.Hx.T % 2).astype(np.int8) for _ in range(6)])
        out[f"{tag}_prior"], out[f"{tag}_syndromes"] = prior, syn.astype(np.uint8)
        for order, layout in (("C", np.ascontiguousarray), ("F", np.asfortranarray)):
            H = layout(code.Hx)
            for name, (fn, kw) in FUNCS.items():
                res = [getattr(rework, fn)(H, s, prior, maxIter=MAX_ITER, **kw) for s in syn]
                key = f"{tag}_{order}_{name}"
                out[key + "_hard"] = np.array([np.asarray(r[0]) for r in res], np.uint8)
                out[key + "_converged"] = np.array([bool(r[1]) for r in res])
                out[key + "_llr"] = np.array([np.asarray(r[2], np.float64) for r in res])
                out[key + "_iters"] = np.array([int(r[3]) for r in res], np.int64)
    np.savez_compressed(os.path.join(HERE, "layout.npz"), **out)
    print(f"wrote {os.path.join(HERE, 'layout.npz')}: {len(out)} arrays")


if __name__ == "__main__":
    main()
