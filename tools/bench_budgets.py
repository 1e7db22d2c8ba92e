#!/usr/bin/env python3
"""Timing of the ladder of BP iteration budgets (qbp_mc_run_budgets) against what it replaces.

Per workload, device-resident, same seed and trial count, best of three after a warm-up, the three timings taken
alternately inside each repetition:
  t_ladder  one ladder call over all budgets                       (this build)
  t_max     one qbp_mc_run_probs_device at the largest budget      (--baseline-lib: the library of the parent commit)
  t_sep     one qbp_mc_run_probs_device per budget, summed         (--baseline-lib)
and the counter tables of the ladder and of the separate calls must be identical.  The condition is
t_ladder < t_sep on every workload; t_ladder / t_max (what checkpointing costs over a plain run at the largest
budget) is reported.  Calls are split by the libraries' OSD steps where OSD keeps per-trial records.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_budgets.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r06_budgets.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qldpc_amd import _lib, bp, codes, dem, mc  # noqa: E402

TENS = tuple(range(10, 100, 10))


class BaselineDecoder:
    """qbp_mc_run_probs_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_probs_device", "qbp_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        rc = self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device,
                                 C.byref(self.h))
        if rc:
            raise RuntimeError(f"baseline qbp_create: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_osd_step(self):
        return max(1, min(_lib.MC_OSD_MAX_TRIALS, (8 << 30) // (self.m + 10 * self.n)))

    def mc_run_probs_device(self, L, distance, probs, d_prior, begin, end, d_counters, seed, max_iter, flags, stream):
        rc = self.lib.qbp_mc_run_probs_device(self.h, L.ctypes.data, L.shape[0], int(distance), probs.ctypes.data, 1,
                                              int(seed), int(begin), int(end), d_prior, int(max_iter), 0, 1.0, 1.0,
                                              20.0, int(flags), d_counters, stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_probs_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def run_workload(name, H, L, distance, probs, prior, budgets, trials, osd, baseline_lib, reps):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = np.ascontiguousarray(L, np.uint8)
    probs = np.ascontiguousarray(probs, np.float64)
    dec = bp.decoder_for(H)
    base = BaselineDecoder(baseline_lib, H)
    d_prior = torch.from_numpy(np.ascontiguousarray(prior, np.float64)).to(dev)
    K = len(budgets)
    flags = _lib.FLAG_OSD0 if osd else 0
    seed = 2026

    def ladder():
        tab = torch.zeros((K, 12), dtype=torch.int64, device=dev)
        step = dec.mc_budgets_step(K) if osd else trials
        for a in range(0, trials, step):
            dec.mc_run_budgets_device(L, distance, probs, d_prior.data_ptr(), budgets, a, min(a + step, trials),
                                      tab.data_ptr(), seed=seed, flags=flags, stream=stream)
        return tab

    def plain(rows):
        tab = torch.zeros((len(rows), 12), dtype=torch.int64, device=dev)
        step = base.mc_osd_step() if osd else trials
        for j, b in enumerate(rows):
            for a in range(0, trials, step):
                base.mc_run_probs_device(L, distance, probs, d_prior.data_ptr(), a, min(a + step, trials),
                                         tab[j].data_ptr(), seed, b, flags, stream)
        return tab

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tab = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, tab.cpu().numpy()

    warm = min(trials, 20000)
    trials_full, trials = trials, warm          # warm-up: every kernel and buffer size class of the timed window
    timed(ladder), timed(lambda: plain(budgets))
    trials = trials_full
    timed(ladder), timed(lambda: plain(budgets[-1:]))        # (buffers at their full size)
    t_ladder, t_max, t_sep = [], [], []
    for _ in range(reps):
        t, got = timed(ladder)
        t_ladder.append(t)
        t, last = timed(lambda: plain(budgets[-1:]))
        t_max.append(t)
        t, want = timed(lambda: plain(budgets))
        t_sep.append(t)
        if not (np.array_equal(got, want) and np.array_equal(last[0], want[-1])):
            raise SystemExit(f"{name}: the ladder's counter table differs from the separate calls\n{got}\n{want}")
    base.close()
    row = dict(workload=name, m=int(H.shape[0]), n=int(H.shape[1]), trials=trials, budgets=list(budgets), osd=bool(osd),
               t_ladder_s=min(t_ladder), t_max_s=min(t_max), t_sep_s=min(t_sep),
               all_t_ladder_s=t_ladder, all_t_max_s=t_max, all_t_sep_s=t_sep,
               ladder_over_max=min(t_ladder) / min(t_max), sep_over_ladder=min(t_sep) / min(t_ladder),
               tables_identical=True, not_converged=got[:, 6].tolist(), kernel=dec.info("last_kernel"))
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
    rows = []
    code = codes.load_code("[[288, 12, 18]]")
    work = []
    for p in (0.01, 0.05):
        for osd in (False, True):
            work.append((f"[[288,12,18]] p={p}" + (" +OSD-0" if osd else ""), code.Hx, code.Lx, code.distance,
                         np.full(code.n, p), mc.prior_of(p, code.n), TENS, args.trials, osd))
    H, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.004, 0.004)
    work.append(("phenomenological 864x2592 p=q=0.004 +OSD-0", H, L, 0, probs, mc.dem_prior(probs), TENS,
                 max(args.trials // 10, 1), True))
    for w in work:
        if args.only is None or args.only in w[0]:
            rows.append(run_workload(*w, args.baseline_lib, args.reps))
    ok = all(r["t_ladder_s"] < r["t_sep_s"] for r in rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_budgets.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_max and t_sep: the parent commit's library", condition_t_ladder_lt_t_sep=ok,
                           rows=rows), f, indent=1)
    if not ok:
        raise SystemExit("t_ladder >= t_sep on some workload")


if __name__ == "__main__":
    main()
