#!/usr/bin/env python3
"""What the posterior-LLR histograms cost: qbp_mc_run_llr_hist against qbp_mc_run_budgets of the parent commit's library.

Per workload, device-resident, same seed, trial count and arguments, best of three after a warm-up, the two timings
taken alternately inside each repetition:
  t_hist    one qbp_mc_run_llr_hist_device call, 128 bins of [-30, 30]    (this build)
  t_ladder  one qbp_mc_run_budgets_device call                            (--baseline-lib: the parent commit's library)
The counter tables must be identical, and the table must satisfy sum = n * trials per budget.  No ratio is a
condition; t_hist / t_ladder is what n LDS atomics per emission (runs of equal cells of a lane merged) cost.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_llr_hist.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r28_llr_hist.json
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
BINS, RANGE = 128, (-30.0, 30.0)


class BaselineDecoder:
    """qbp_mc_run_budgets_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_budgets_device", "qbp_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        rc = self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device, C.byref(self.h))
        if rc:
            raise RuntimeError(f"baseline qbp_create: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_run_budgets_device(self, L, distance, probs, d_prior, budgets, begin, end, d_counters, seed, flags, stream):
        bud = np.ascontiguousarray(budgets, np.int32)
        rc = self.lib.qbp_mc_run_budgets_device(self.h, L.ctypes.data, L.shape[0], int(distance), probs.ctypes.data, 1,
                                                int(seed), int(begin), int(end), d_prior, bud.ctypes.data, len(bud), 0, 1.0,
                                                1.0, 20.0, int(flags), d_counters, stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_budgets_device: {rc} {self.lib.qbp_last_error().decode()}")

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
    K, n = len(budgets), H.shape[1]
    flags = _lib.FLAG_OSD0 if osd else 0
    seed = 2026
    step = dec.mc_budgets_step(K) if osd else trials

    def hist(T):
        out = torch.zeros(K * 12 + K * 4 * (BINS + 3), dtype=torch.int64, device=dev)
        for a in range(0, T, step):
            dec.mc_run_llr_hist_device(L, distance, probs, d_prior.data_ptr(), budgets, BINS, RANGE, a, min(a + step, T),
                                       out.data_ptr(), out.data_ptr() + 8 * K * 12, seed=seed, flags=flags, stream=stream)
        return out

    def ladder(T):
        tab = torch.zeros(K * 12, dtype=torch.int64, device=dev)
        for a in range(0, T, step):
            base.mc_run_budgets_device(L, distance, probs, d_prior.data_ptr(), budgets, a, min(a + step, T), tab.data_ptr(),
                                       seed, flags, stream)
        return tab

    def timed(fn, T):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tab = fn(T)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, tab.cpu().numpy()

    for T in (min(trials, 20000), trials):          # warm-up: every kernel and buffer size class of the timed window
        timed(hist, T), timed(ladder, T)
    t_hist, t_ladder = [], []
    for _ in range(reps):
        t, got = timed(hist, trials)
        t_hist.append(t)
        t, want = timed(ladder, trials)
        t_ladder.append(t)
        cnt, table = mc._split_llr_hist(got, K, BINS)
        if not np.array_equal(cnt.ravel(), want) or not (table.sum(axis=(1, 2)) == n * trials).all():
            raise SystemExit(f"{name}: counters differ from the parent's ladder, or the table does not add up")
    base.close()
    row = dict(workload=name, m=int(H.shape[0]), n=int(n), trials=trials, budgets=list(budgets), bins=BINS, osd=bool(osd),
               t_hist_s=min(t_hist), t_ladder_s=min(t_ladder), all_t_hist_s=t_hist, all_t_ladder_s=t_ladder,
               hist_over_ladder=min(t_hist) / min(t_ladder), counters_identical=True,
               values_outside_range=int(table[:, :, 0].sum() + table[:, :, BINS + 1].sum()), kernel=dec.info("last_kernel"))
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
    for budgets, tag in ((TENS, "budgets 10..90"), ((50,), "budget 50")):
        for p in (0.01, 0.05):
            for osd in (False, True):
                work.append((f"[[288,12,18]] p={p} {tag}" + (" +OSD-0" if osd else ""), code.Hx, code.Lx, code.distance,
                             np.full(code.n, p), mc.prior_of(p, code.n), budgets, args.trials, osd))
    H, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.004, 0.004)
    work.append(("phenomenological 864x2592 p=q=0.004 budgets 10..90", H, L, 0, probs, mc.dem_prior(probs), TENS,
                 max(args.trials // 10, 1), False))
    rows = [run_workload(*w, args.baseline_lib, args.reps) for w in work if args.only is None or args.only in w[0]]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_llr_hist.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_ladder: qbp_mc_run_budgets_device of the parent commit's library",
                           merging="runs of equal cells among a lane's own values; no wave-level merge was built or measured",
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
