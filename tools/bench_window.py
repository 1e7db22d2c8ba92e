#!/usr/bin/env python3
"""Sliding-window decoding against the whole-matrix decode: trials/s and logical error rate on the 2592 x 7776 and
864 x 2592 phenomenological matrices of [[288,12,18]] (18 and 6 rounds), p = q = 0.004, BP(50) + OSD-0, windows (6, 3)
and (4, 2); best of three runs.  Writes profiles/r15_window.json.

The whole-matrix rows are measured twice: on this build, and -- with --parent-lib LIBQBP.SO, the library of a checkout of
the parent commit -- on that build, in a child process of its own (one library per process), whose rows are merged into
the same file under the decoder name "whole (parent build)"."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CODE, DISTANCE = "[[288, 12, 18]]", 18


def measure(args, whole_label, windows):
    from qldpc_amd import _lib, bp, dem, mc, window
    flags = _lib.osd_flags("cs", 0)
    rows = []
    for rounds in (18, 6):
        H, L, probs = dem.phenomenological(CODE, rounds, args.p)
        cr = window.phenomenological_rounds(CODE, rounds)
        prior = mc.dem_prior(probs)
        step = 1 << 14                                    # (whole-matrix calls with OSD keep per-trial records)
        runs = [(whole_label, None)] + [(f"window {w}", w) for w in windows if w[0] < rounds]
        for label, wf in runs:
            dec = bp.decoder_for(H) if wf is None else window.decoder_for(H, cr, *wf)
            best, cnt = float("inf"), None
            for rep in range(args.repeats + 1):           # (the first run warms up and is dropped)
                cnt = np.zeros(_lib.NUM_COUNTERS, np.int64)
                t0 = time.perf_counter()
                for a in range(0, args.trials, step):
                    part = dec.mc_run_probs(L, DISTANCE, probs, prior, a, min(a + step, args.trials), seed=1, max_iter=50,
                                            flags=flags)
                    cnt += part
                dt = time.perf_counter() - t0
                if rep:
                    best = min(best, dt)
            ler = cnt[1] / cnt[0]
            rows.append(dict(matrix=f"{H.shape[0]}x{H.shape[1]}", decoder=label, trials=int(cnt[0]),
                             trials_per_s=float(cnt[0] / best), ler=float(ler),
                             ler_se=math.sqrt(max(ler * (1 - ler), 0) / cnt[0]), not_converged=int(cnt[6]),
                             missed=int(cnt[10])))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=100000)
    ap.add_argument("--p", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libqbp.so built from the parent commit: its whole-matrix rows too")
    ap.add_argument("--rows-only", action="store_true", help="(the child process of --parent-lib) whole-matrix rows as JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_window.json"))
    args = ap.parse_args()
    if args.rows_only:
        print("ROWS " + json.dumps(measure(args, "whole (parent build)", [])))
        return
    rows = measure(args, "whole", [(6, 3), (4, 2)])
    if args.parent_lib:
        env = dict(os.environ, QBP_LIB_PATH=os.path.abspath(args.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-only", "--trials", str(args.trials), "--p",
                              str(args.p), "--repeats", str(args.repeats)], env=env, check=True, capture_output=True,
                             text=True).stdout
        rows += json.loads([ln for ln in out.splitlines() if ln.startswith("ROWS ")][-1][5:])
    with open(args.out, "w") as f:
        json.dump(dict(p=args.p, max_iter=50, osd="OSD-0", parent_build=bool(args.parent_lib), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
