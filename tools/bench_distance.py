#!/usr/bin/env python3
"""Trials per second of qbp_distance_search (dist_search_kernel) on [[72,12,6]], [[144,12,12]] and [[288,12,18]], the
numpy statement (tests/distance_oracle.py) on the host for comparison, and the number of trials before weight 18 first
appears on [[288,12,18]] at seed 0.  Writes profiles/r32_distance.json.  There is no parent-commit baseline: the
entry is new.

    python tools/bench_distance.py [--trials N] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from qldpc_amd import bp, codes, gf2      # noqa: E402

CODES = ("[[72, 12, 6]]", "[[144, 12, 12]]", "[[288, 12, 18]]")
REPS = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--trials", type=int, default=1 << 18, help="trials per timed call")
    ap.add_argument("--oracle-trials", type=int, default=200)
    ap.add_argument("--first-18-limit", type=int, default=1 << 22, help="give up the search for weight 18 after this many")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_distance.json"))
    args = ap.parse_args()
    import distance_oracle as do

    rows = []
    for name in CODES:
        code = codes.load_code(name)
        G = gf2.nullspace(code.Hx)
        dec = bp.decoder_for(code.Hx)
        dec.distance_search(G, code.Lx, 0, 1024, want_codeword=False)                 # warm-up
        times, out = [], None
        for _ in range(REPS):
            t0 = time.perf_counter()
            out = dec.distance_search(G, code.Lx, 0, args.trials)
            times.append(time.perf_counter() - t0)
        result, hist = out[0], out[1]
        rows.append(dict(code=name, side="Hx, Lx", generator_rows=int(G.shape[0]), n=code.n, trials=args.trials, seed=0,
                         t_s=min(times), all_t_s=times, trials_per_s=args.trials / min(times),
                         weight=int(result[1]), first_trial=int(result[2]), distance=code.distance,
                         grid=dec.info("grid"), lds_bytes=dec.info("lds_bytes"),
                         hist={int(w): int(hist[w]) for w in np.flatnonzero(hist)}))
        print(json.dumps(rows[-1]), flush=True)

    # the statement on the host
    code = codes.load_code("[[144, 12, 12]]")
    G = gf2.nullspace(code.Hx)
    t0 = time.perf_counter()
    want = do.search(G, code.Lx, 0, 0, args.oracle_trials)
    t_oracle = time.perf_counter() - t0
    got = bp.decoder_for(code.Hx).distance_search(G, code.Lx, 0, args.oracle_trials)
    oracle = dict(code=code.name, trials=args.oracle_trials, t_s=t_oracle, trials_per_s=args.oracle_trials / t_oracle,
                  equal_to_the_kernel=bool(np.array_equal(want["result"], got[0]) and np.array_equal(want["hist"], got[1])))
    print(json.dumps(oracle), flush=True)

    # trials before 18 first appears on [[288,12,18]] at seed 0: doubling ranges, the first trial of the first hit
    code = codes.load_code("[[288, 12, 18]]")
    G = gf2.nullspace(code.Hx)
    dec = bp.decoder_for(code.Hx)
    first, begin, step, lightest = None, 0, 1 << 12, None
    while begin < args.first_18_limit:
        result = dec.distance_search(G, code.Lx, begin, begin + step, want_codeword=False)[0]
        if result[1] >= 0 and (lightest is None or result[1] < lightest):
            lightest = int(result[1])
        if result[1] == 18:
            first = int(result[2])
            break
        begin, step = begin + step, step * 2
    first_18 = dict(code=code.name, seed=0, first_trial_with_18=first, trials_searched=begin + (step if first is not None else 0),
                    lightest_seen=lightest)
    print(json.dumps(first_18), flush=True)

    doc = dict(tool="tools/bench_distance.py", device="MI355X (gfx950)", reps=REPS,
               timing="host clock around qbp_distance_search (host entry: H g = 0 check, bit-packing, upload, the search "
                      "launch, the capture launch, download), best of reps after one warm-up call",
               baseline="none: the entry is new", rows=rows, oracle=oracle, first_18=first_18)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
