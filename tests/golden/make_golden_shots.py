#!/usr/bin/env python3
"""Recorded shots decoded by RUNNING THE REAL REFERENCE (build container only):
    MPLBACKEND=Agg python tests/golden/make_golden_shots.py

The loop of studies/studyComplete.py:91-109 -- detection events and actual observables per shot, BP, OSD on BP's
failures, `L @ prediction % 2` -- with the reference's own functions:

  rework/decoding.py:77  performBeliefPropagationFast(H, syndrome, initialBelief, maxIter=20)
  decoding/OSD.py:3      performOSD(H, syndrome, llr, hard)          (on the shots BP did not converge on)

on 256 shots drawn with numpy from the phenomenological model of [[72,12,6]] over 4 rounds (data rate P, measurement
rate Q: qldpc_amd/dem.py builds the matrices, no stim needed; at P = 0.01, Q = 0.02 only 10 of the 256 shots stay
unconverged after 20 iterations, so the rates are 0.015 and 0.03: 37 do).  Stored: the shots bit-packed as the decoder takes them
(detections, stim's b8 layout), the actual observables and the reference's predictions as uint64 masks, its converged
flags and iteration indices.  H is handed to the reference C-ordered (h_order), which fixes its column-sum order
(oracle.colsum_flags).  The script refuses to write a fixture with fewer than 16 unconverged shots (raise the rates)
or one in which a shot handed to OSD has two columns of exactly equal |LLR| (np.argsort's order of ties is the one
output the project does not pin: take another seed).
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
sys.path.insert(0, ROOT)
from qldpc_amd import dem, mc, shots                                      # noqa: E402

sys.path.insert(0, REF)
with contextlib.redirect_stdout(io.StringIO()):
    from decoding.OSD import performOSD                                   # noqa: E402
    from rework.decoding import performBeliefPropagationFast              # noqa: E402

CODE, ROUNDS, P, Q = "[[72, 12, 6]]", 4, 0.015, 0.03
SEED, SHOTS, MAX_ITER = 20260128, 256, 20


def main():
    H, L, probs = dem.phenomenological(CODE, ROUNDS, P, Q)
    Hd = np.ascontiguousarray(H.toarray().astype(np.int64))              # C order
    m, n = Hd.shape
    prior = mc.dem_prior(probs)
    rng = np.random.default_rng(SEED)
    errors = (rng.random((SHOTS, n)) < probs).astype(np.int64)
    syn = errors @ Hd.T % 2
    actual = errors @ L.astype(np.int64).T % 2
    xs, conv, iters = [], [], []
    ties = 0
    for t in range(SHOTS):
        x, ok, llr, it = performBeliefPropagationFast(Hd, syn[t], prior, maxIter=MAX_ITER)
        x = np.asarray(x, np.int64)
        if not ok:
            ties += len(np.unique(np.abs(llr))) != n
            x = np.asarray(performOSD(Hd, syn[t], np.asarray(llr), x), np.int64)
        xs.append(x % 2); conv.append(bool(ok)); iters.append(int(it))
    xs, conv, iters = np.array(xs), np.array(conv), np.array(iters, np.int32)
    pred = xs @ L.astype(np.int64).T % 2
    bad = int(sum(not np.array_equal(xs[t] @ Hd.T % 2, syn[t]) for t in np.flatnonzero(~conv)))
    print(f"{SHOTS} shots of {m} x {n}: {int((~conv).sum())} unconverged, {int((pred != actual).any(1).sum())} wrong "
          f"predictions, {bad} OSD outputs that miss the syndrome, {ties} OSD shots with tied |LLR|")
    if (~conv).sum() < 16 or conv.sum() < 16:
        raise SystemExit("the fixture needs at least 16 converged and 16 unconverged shots: change the rates")
    if ties:
        raise SystemExit("an OSD shot has tied |LLR|s: take another seed")
    path = os.path.join(HERE, "shots.npz")
    np.savez_compressed(
        path, code=np.array(CODE), rounds=np.int64(ROUNDS), p=np.float64(P), q=np.float64(Q), max_iter=np.int64(MAX_ITER),
        h_order=np.array("C"), detections=shots.pack_bits(syn), actual=shots.masks_of(actual),
        predictions=shots.masks_of(pred), converged=conv, iters=iters)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
