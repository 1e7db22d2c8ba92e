#!/usr/bin/env python3
"""Iterations, failure fraction, throughput and logical error rate of layered BP (QBP_FLAG_LAYERED) against flooding.

[[144,12,12]] and [[288,12,18]], p in {0.03, 0.05}, sum-product and min-sum (alpha 0.9), BP(50) + OSD-0, 1e6 trials,
device-resident, best of three after a warm-up, the two schedules timed alternately inside each repetition:
  flooding  qbp_mc_run_device | QBP_FLAG_OSD0                    (--baseline-lib: the library of the parent commit)
  layered   qbp_mc_run_device | QBP_FLAG_OSD0 | QBP_FLAG_LAYERED, the default order                    (this build)
Recorded per point: syndromes/s, mean iterations per syndrome (sum_iterations / trials, 0-based as `iters`), the
unconverged fraction and the LER of BP(50) + OSD-0, from the counters of the timed runs (same trials: one seed).
Nobody set a threshold: iterations-to-converge is the claim this tool exists to test; everything is reported.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_layered.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r13_layered.json
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

from qldpc_amd import _lib, bp, codes, layered, mc  # noqa: E402

MAX_ITER, SEED, ALPHA = 50, 2026, 0.9
VARIANTS = (("sum-product", _lib.SUM_PRODUCT, 1.0), ("min-sum", _lib.MIN_SUM, ALPHA))


class BaselineDecoder:
    """qbp_mc_run_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_device", "qbp_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        rc = self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device, C.byref(self.h))
        if rc:
            raise RuntimeError(f"baseline qbp_create: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_run_device(self, L, distance, p, d_prior, begin, end, d_counters, seed=0, max_iter=50, variant=0, alpha=1.0,
                      flags=0, stream=0):
        L = np.ascontiguousarray(L, np.uint8)
        rc = self.lib.qbp_mc_run_device(self.h, L.ctypes.data, L.shape[0], int(distance), float(p), 1, int(seed),
                                        int(begin), int(end), d_prior, int(max_iter), int(variant), float(alpha), 1.0,
                                        20.0, int(flags), d_counters, stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def timed_mc(torch, dec, code, p, trials, variant, alpha, flags):
    """Seconds and counters of one device-resident run of `trials` trials, split by the record limit."""
    dev = torch.device("cuda", 0)
    d_prior = torch.from_numpy(mc.prior_of(p, code.n)).to(dev)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    step = _lib.MC_OSD_MAX_TRIALS
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for a in range(0, trials, step):
        dec.mc_run_device(code.Lx, code.distance, p, d_prior.data_ptr(), a, min(a + step, trials), d_cnt.data_ptr(),
                          seed=SEED, max_iter=MAX_ITER, variant=variant, alpha=alpha, flags=flags, stream=stream)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, d_cnt.cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit for the flooding runs")
    ap.add_argument("--trials", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--codes", nargs="+", default=["[[144, 12, 12]]", "[[288, 12, 18]]"])
    ap.add_argument("--p", type=float, nargs="+", default=[0.03, 0.05])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    result = {"trials": args.trials, "max_iter": MAX_ITER, "seed": SEED, "min_sum_alpha": ALPHA,
              "flooding_library": "parent build" if args.baseline_lib else "this build", "points": []}
    for name in args.codes:
        code = codes.load_code(name)
        dec = bp.decoder_for(code.Hx)
        dec.layered_configure(None)
        _, levels = layered.layered_order(code.Hx)
        base = BaselineDecoder(args.baseline_lib, code.Hx) if args.baseline_lib else dec
        runs = {"flooding": (base, _lib.FLAG_OSD0), "layered": (dec, _lib.FLAG_OSD0 | _lib.FLAG_LAYERED)}
        for p in args.p:
            for vname, variant, alpha in VARIANTS:
                best, cnt = {}, {}
                for d, fl in runs.values():                                  # warm-up
                    timed_mc(torch, d, code, p, min(args.trials, 65536), variant, alpha, fl)
                for _ in range(args.reps):
                    for key, (d, fl) in runs.items():
                        t, c = timed_mc(torch, d, code, p, args.trials, variant, alpha, fl)
                        best[key] = min(best.get(key, t), t)
                        cnt[key] = c
                point = {"code": name, "p": p, "variant": vname, "levels": len(levels)}
                for key in runs:
                    c = cnt[key]
                    point[key] = {"seconds": best[key], "syndromes_per_s": args.trials / best[key],
                                  "mean_iterations": float(c[7]) / float(c[0]),
                                  "unconverged_fraction": float(c[6]) / float(c[0]),
                                  "ler_bp_osd0": float(c[1]) / float(c[0]),
                                  "counters": dict(zip(_lib.COUNTER_NAMES, (int(x) for x in c)))}
                print(json.dumps(point), flush=True)
                result["points"].append(point)
        if base is not dec:
            base.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
