#!/usr/bin/env python3
"""Timing of the Monte-Carlo with residual-weight spectra and iteration histogram (qbp_mc_run_spectrum) against the
plain run it extends.

Per workload, device-resident, same seed and trial count, best of three after a warm-up, the two timings taken
alternately inside each repetition:
  t_spectrum  qbp_mc_run_spectrum_device: counters + spectrum [4, n + 1] + iter_hist [max_iter + 1]   (this build)
  t_plain     qbp_mc_run_probs_device with the same arguments        (--baseline-lib: the library of the parent commit)
and the counters of the two must be identical.  Nobody set a threshold: t_spectrum / t_plain is reported.  Calls are
split by the libraries' OSD step where OSD keeps per-trial records.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_spectrum.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r07_spectrum.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_budgets import BaselineDecoder  # noqa: E402
from qldpc_amd import _lib, bp, codes, dem, mc  # noqa: E402

MAX_ITER = 50


def run_workload(name, H, L, distance, probs, prior, trials, osd, baseline_lib, reps):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = np.ascontiguousarray(L, np.uint8)
    probs = np.ascontiguousarray(probs, np.float64)
    dec = bp.decoder_for(H)
    base = BaselineDecoder(baseline_lib, H)
    d_prior = torch.from_numpy(np.ascontiguousarray(prior, np.float64)).to(dev)
    n = int(H.shape[1])
    flags = _lib.FLAG_OSD0 if osd else 0
    seed = 2026

    def spectrum():
        tab = torch.zeros(12 + 4 * (n + 1) + MAX_ITER + 1, dtype=torch.int64, device=dev)
        step = dec.mc_osd_step() if osd else trials
        for a in range(0, trials, step):
            dec.mc_run_spectrum_device(L, distance, probs, d_prior.data_ptr(), a, min(a + step, trials), tab.data_ptr(),
                                       tab.data_ptr() + 8 * 12, tab.data_ptr() + 8 * (12 + 4 * (n + 1)), seed=seed,
                                       max_iter=MAX_ITER, flags=flags, stream=stream)
        return tab

    def plain():
        tab = torch.zeros(12, dtype=torch.int64, device=dev)
        step = base.mc_osd_step() if osd else trials
        for a in range(0, trials, step):
            base.mc_run_probs_device(L, distance, probs, d_prior.data_ptr(), a, min(a + step, trials), tab.data_ptr(),
                                     seed, MAX_ITER, flags, stream)
        return tab

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tab = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, tab.cpu().numpy()

    trials_full, trials = trials, min(trials, 20000)      # warm-up: every kernel of the timed window
    timed(spectrum), timed(plain)
    trials = trials_full
    timed(spectrum), timed(plain)                          # (buffers at their full size)
    t_spec, t_plain = [], []
    for _ in range(reps):
        t, got = timed(spectrum)
        t_spec.append(t)
        t, want = timed(plain)
        t_plain.append(t)
        if not np.array_equal(got[:12], want):
            raise SystemExit(f"{name}: the spectrum run's counters differ from the plain run's\n{got[:12]}\n{want}")
    base.close()
    weights = got[12:12 + 4 * (n + 1)].reshape(4, n + 1)
    row = dict(workload=name, m=int(H.shape[0]), n=n, trials=trials, max_iter=MAX_ITER, osd=bool(osd),
               t_spectrum_s=min(t_spec), t_plain_s=min(t_plain), all_t_spectrum_s=t_spec, all_t_plain_s=t_plain,
               spectrum_over_plain=min(t_spec) / min(t_plain), counters_identical=True,
               row_sums=weights.sum(axis=1).tolist(), not_converged=int(got[6]), kernel=dec.info("last_kernel"))
    print(json.dumps({k: v for k, v in row.items() if not k.startswith("all_")}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", required=True, help="libqbp.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trials", type=int, default=1000000, help="[[288,12,18]] workloads (the DEM one runs a tenth)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring of the workload names to run")
    args = ap.parse_args()
    code = codes.load_code("[[288, 12, 18]]")
    work = []
    for p in (0.01, 0.05):
        for osd in (False, True):
            work.append((f"[[288,12,18]] p={p}" + (" +OSD-0" if osd else ""), code.Hx, code.Lx, code.distance,
                         np.full(code.n, p), mc.prior_of(p, code.n), args.trials, osd))
    H, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.004, 0.004)
    work.append(("phenomenological 864x2592 p=q=0.004 +OSD-0", H, L, 0, probs, mc.dem_prior(probs),
                 max(args.trials // 10, 1), True))
    rows = [run_workload(*w, args.baseline_lib, args.reps) for w in work if args.only is None or args.only in w[0]]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_spectrum.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_plain: qbp_mc_run_probs_device of the parent commit's library", rows=rows),
                      f, indent=1)


if __name__ == "__main__":
    main()
