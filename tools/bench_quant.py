#!/usr/bin/env python3
"""Timing and logical error rate of fixed-point min-sum (bp_quant_kernel) against double-precision min-sum.

  1. batch throughput on [[144,12,12]] and [[288,12,18]], forced 50 iterations and with early exit, q in {4, 6, 8, 16},
     against qbp_decode_batch(QBP_MIN_SUM) on the same syndromes;
  2. BP(50) + OSD-0 logical error rate and trials/s at p = 0.03 and 0.05, q in {4, 5, 6, 8} at two scales, against
     double-precision min-sum at the same alpha;
  3. the same on the 864 x 2592 phenomenological matrix.

Best of three.  ``--baseline-lib PATH``: the parent commit's libqbp.so for the double-precision rows (run in a child
process of its own, since a process loads one library); without it they are timed on this build, whose flooding
kernels are the parent's.  Writes profiles/r29_quant.json."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHA = (13, 4)                     # 13 / 16 = 0.8125
ITERS = 50


def best_of(fn, reps=3):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def matrices():
    from qldpc_amd import codes, dem
    out = {}
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        c = codes.load_code(name)
        out[name] = (np.asarray(c.Hx, np.uint8), np.asarray(c.Lx, np.uint8), c.distance, None)
    Hs, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.004)
    out["864x2592"] = (np.asarray(Hs.todense()).astype(np.uint8), np.ascontiguousarray(L, np.uint8), 0, probs)
    return out


def run(args):
    import torch
    from qldpc_amd import _lib, bp, quant
    res = {"alpha": ALPHA[0] / (1 << ALPHA[1]), "iters": ITERS, "library": os.path.basename(_lib.LIB_PATH), "batch": [], "mc": []}
    mats = matrices()
    alpha = ALPHA[0] / (1 << ALPHA[1])
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        H, L, d, _ = mats[name]
        m, n = H.shape
        dec = _lib.Decoder(*bp.csr_from_H(H), 0)
        B, p = args.batch, 0.05
        errors = (np.random.default_rng(1).random((B, n)) < p).astype(np.uint8)
        syn = torch.from_numpy((errors.astype(np.float32) @ H.T.astype(np.float32) % 2).astype(np.uint8)).cuda()
        prior = torch.full((n,), float(np.log((1 - p) / p)), dtype=torch.float64).cuda()
        hard = torch.empty((B, n), dtype=torch.uint8).cuda()
        conv = torch.empty(B, dtype=torch.uint8).cuda()
        its = torch.empty(B, dtype=torch.int32).cuda()
        for forced in (True, False):
            fl = _lib.FLAG_FORCE_FULL if forced else 0

            def dbl():
                dec.decode_device(syn.data_ptr(), prior.data_ptr(), B, ITERS, _lib.MIN_SUM, alpha, 1.0, 20.0, fl,
                                  hard.data_ptr(), conv.data_ptr(), its.data_ptr(), 0)
            dbl()
            t, _ = best_of(dbl)
            res["batch"].append(dict(code=name, forced=forced, decoder="double", seconds=t, per_s=B / t,
                                     converged=float(conv.float().mean().item())))
            if args.baseline_only:
                continue
            for q in (4, 6, 8, 16):
                dec.quant_configure(quant.QuantConfig(q, 2.0 if q < 16 else 64.0, ALPHA))

                def qnt():
                    dec.quant_decode_device(syn.data_ptr(), prior.data_ptr(), B, ITERS, fl, hard.data_ptr(),
                                            conv.data_ptr(), its.data_ptr(), 0, 0)
                qnt()
                t, _ = best_of(qnt)
                res["batch"].append(dict(code=name, forced=forced, decoder=f"q{q}", seconds=t, per_s=B / t,
                                         converged=float(conv.float().mean().item()), slots_lds=dec.info("lds_bytes"),
                                         grid=dec.info("grid")))
    for name, ps in (("[[144, 12, 12]]", (0.03, 0.05)), ("[[288, 12, 18]]", (0.03, 0.05)), ("864x2592", (None,))):
        H, L, d, probs = mats[name]
        n = H.shape[1]
        dec = _lib.Decoder(*bp.csr_from_H(H), 0)
        for p in ps:
            pr = np.full(n, p) if probs is None else probs
            prior = np.log((1 - pr) / pr)
            T = args.trials if probs is None else args.trials // 10

            def mc(flags):
                step = dec.mc_osd_step()
                cnt = np.zeros(12, np.int64)
                for a in range(0, T, step):
                    cnt += dec.mc_run_probs(L, d, pr, prior, a, min(a + step, T), seed=3, max_iter=ITERS,
                                            variant=_lib.MIN_SUM, alpha=alpha, flags=flags | _lib.FLAG_OSD0)
                return cnt
            mc(0)
            t, cnt = best_of(lambda: mc(0))
            res["mc"].append(dict(code=name, p=p, decoder="double", seconds=t, trials_per_s=T / t, trials=int(cnt[0]),
                                  ler=cnt[1] / cnt[0], not_converged=cnt[6] / cnt[0]))
            if args.baseline_only:
                continue
            for q in (4, 5, 6, 8):
                for scale in (1.0, 2.0):
                    dec.quant_configure(quant.QuantConfig(q, scale, ALPHA))
                    mc(_lib.FLAG_QUANT)
                    t, cnt = best_of(lambda: mc(_lib.FLAG_QUANT))
                    res["mc"].append(dict(code=name, p=p, decoder=f"q{q}", scale=scale, seconds=t, trials_per_s=T / t,
                                          trials=int(cnt[0]), ler=cnt[1] / cnt[0], not_converged=cnt[6] / cnt[0]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--trials", type=int, default=1000000)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-only", action="store_true", help="(the child process of --baseline-lib)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_quant.json"))
    args = ap.parse_args()
    if args.baseline_only:
        print(json.dumps(run(args)))
        return
    res = run(args)
    if args.baseline_lib:
        env = dict(os.environ, QBP_LIB_PATH=os.path.abspath(args.baseline_lib))
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--baseline-only", "--batch",
                                       str(args.batch), "--trials", str(args.trials)], env=env, text=True)
        res["parent"] = json.loads(out.strip().splitlines()[-1])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for row in res["batch"] + res["mc"]:
        print(row)


if __name__ == "__main__":
    main()
