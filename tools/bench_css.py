#!/usr/bin/env python3
"""Timing of the two-stage CSS decoder under depolarizing noise -> profiles/r22_css.json.

[[144,12,12]] and [[288,12,18]] at p = 0.01 and 0.03, BP(50) + OSD-0, best of three:
  css_mc_run         qbp_css_mc_run (sample, two syndromes, stage A, conditioned stage B, classify), trials / s;
  two_sector_sum     two qbp_mc_run_errors calls, (Hx, Lx, e_a) and (Hz, Lz, e_b), on the errors the sampler drew: the
                     cost of decoding the two sectors without the correlation (uploads of the stored errors included);
  cond_kernel        bp_cond_kernel alone (qbp_decode_batch_cond_device, sel == 0) against qbp_decode_batch_device on
                     the same syndromes and prior, both with device-resident inputs;
  ler                the joint logical error rate with the conditioned second stage and with the independent baseline.
Nothing here is a pass / fail criterion.

    python tools/bench_css.py [--trials 1000000] [--out profiles/r22_css.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qldpc_amd import _lib, bp, codes, css  # noqa: E402


def best_of(fn, reps=3):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--trials", type=int, default=1000000)
    ap.add_argument("--kernel-batch", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_css.json"))
    args = ap.parse_args()
    import torch
    T, flags = args.trials, _lib.FLAG_OSD0
    rows = []
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        code = codes.load_code(name)
        dec = _lib.CssDecoder(bp.decoder_for(code.Hx), bp.decoder_for(code.Hz))
        for p in (0.01, 0.03):
            rates = (p / 3, p / 3, p / 3)
            pa, b0, b1 = css.pauli_priors(*rates, code.n)
            pb = css.marginal_prior_b(*rates, code.n)
            run = lambda x0, x1: dec.mc_run(code.Lx, code.Lz, code.distance, *rates, pa, x0, x1, 0, T, seed=1, flags=flags)
            corr, base = run(b0, b1), run(pb, pb)
            t_css = best_of(lambda: run(b0, b1))
            ea, eb = dec.sample_errors(*rates, 0, min(T, _lib.MC_OSD_MAX_TRIALS), seed=1)
            t_two = best_of(lambda: (dec.a.mc_run_errors(code.Lx, code.distance, ea, pa, flags=flags),
                                     dec.b.mc_run_errors(code.Lz, code.distance, eb, pb, flags=flags)))
            # the kernel alone, inputs resident on the device
            B = min(args.kernel_batch, len(eb))
            syn = torch.from_numpy((eb[:B].astype(np.float32) @ np.asarray(code.Hz, np.float32).T % 2).astype(np.uint8)).cuda()
            sel = torch.zeros((B, code.n), dtype=torch.uint8, device="cuda")
            d_p0, d_p1 = torch.from_numpy(b0).cuda(), torch.from_numpy(b1).cuda()
            hard = torch.empty((B, code.n), dtype=torch.uint8, device="cuda")
            conv = torch.empty(B, dtype=torch.uint8, device="cuda")
            its = torch.empty(B, dtype=torch.int32, device="cuda")
            s = torch.cuda.current_stream().cuda_stream

            def timed(launch):
                def go():
                    launch()
                    torch.cuda.synchronize()
                go()
                return best_of(go)
            t_cond = timed(lambda: dec.b.decode_cond_device(syn.data_ptr(), sel.data_ptr(), d_p0.data_ptr(), d_p1.data_ptr(), B,
                                                            50, _lib.SUM_PRODUCT, 1.0, 20.0, 0, hard.data_ptr(),
                                                            conv.data_ptr(), its.data_ptr(), 0, s))
            t_plain = timed(lambda: dec.b.decode_device(syn.data_ptr(), d_p0.data_ptr(), B, 50, _lib.SUM_PRODUCT, 1.0, 1.0,
                                                        20.0, 0, hard.data_ptr(), conv.data_ptr(), its.data_ptr(), 0, s))
            rows.append({"code": name, "p": p, "trials": T,
                         "css_mc_run": {"seconds": t_css, "trials_per_s": T / t_css},
                         "two_sector_sum": {"seconds": t_two, "trials": len(ea), "trials_per_s": len(ea) / t_two},
                         "cond_kernel": {"batch": B, "seconds": t_cond, "syndromes_per_s": B / t_cond,
                                         "decode_batch_device_seconds": t_plain, "decode_batch_device_per_s": B / t_plain},
                         "ler": {"correlated": int(corr[2][1]) / T, "independent": int(base[2][1]) / T},
                         "counters": {"correlated": corr.tolist(), "independent": base.tolist()}})
            print(json.dumps(rows[-1]), flush=True)
    result = {"tool": "tools/bench_css.py", "device": torch.cuda.get_device_name(0), "max_iter": 50, "osd": "OSD-0",
              "variant": "sum-product", "best_of": 3, "points": rows}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
