#!/usr/bin/env python3
"""Order-w OSD on one MI355X: batch throughput of OSD-0 / CS-7 / E-8 on BP failures, Monte-Carlo trials/s with
OSD-0 and with CS-7, and the BP(50)+OSD logical error rates of both on [[144,12,12]].

    python tools/bench_osd_order.py [--out profiles/r04_osd_order.json] [--ler-trials 1000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qldpc_amd import _lib, bp, codes, mc  # noqa: E402

METHODS = (("OSD-0", "cs", 0), ("CS-7", "cs", 7), ("E-8", "e", 8))


def batch_rates(name, B, p=0.1, reps=3):
    """Solutions/s of each method on B BP(50) outputs at p (device buffers, best of `reps` launches)."""
    dev = torch.device("cuda", 0)
    code = codes.load_code(name)
    n = code.n
    Ht = torch.from_numpy(code.Hx.T.astype(np.float32)).to(dev)
    g = torch.Generator(device=dev); g.manual_seed(2)
    err = torch.rand((B, n), generator=g, device=dev) < p
    syn = (err.float() @ Ht).remainder_(2).to(torch.uint8)
    prior = torch.full((n,), float(np.log((1 - p) / p)), dtype=torch.float64, device=dev)
    hard = torch.empty((B, n), dtype=torch.uint8, device=dev); conv = torch.empty((B,), dtype=torch.uint8, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev); llr = torch.empty((B, n), dtype=torch.float64, device=dev)
    sol = torch.empty((B, n), dtype=torch.uint8, device=dev)
    dec = bp.decoder_for(code.Hx)
    st = torch.cuda.current_stream(dev)
    dec.decode_device(syn.data_ptr(), prior.data_ptr(), B, 50, 0, 1.0, 1.0, 20.0, 0, hard.data_ptr(),
                      conv.data_ptr(), iters.data_ptr(), llr.data_ptr(), st.cuda_stream)
    out = {"B": B, "p": p, "bp_converged": round(float(conv.float().mean()), 4)}
    for label, method, w in METHODS:
        def run():
            dec.osd_device(syn.data_ptr(), llr.data_ptr(), hard.data_ptr(), B, sol.data_ptr(), method=method,
                           order=w, stream=st.cuda_stream)
        run(); torch.cuda.synchronize()
        best = 1e9
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); run(); b.record(); torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b))
        ok = bool((((sol.float() @ Ht).remainder_(2).to(torch.uint8)) == syn).all())
        out[label] = {"solutions_per_s": round(B / best * 1e3, 1), "ms": round(best, 3), "solutions_match_syndrome": ok,
                      "weight_sum": int(sol.to(torch.int64).sum().item())}
    return out


def mc_rate(name, p, trials, method, order):
    mc.run_sweep(name, [p], min(trials, 65536), osd=True, osd_method=method, osd_order=order, seed=1)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = mc.run_sweep(name, [p], trials, osd=True, osd_method=method, osd_order=order, seed=0)
    dt = time.perf_counter() - t0
    s = mc.summarize(table[0])
    return {"trials": trials, "seconds": round(dt, 4), "trials_per_s": round(trials / dt, 1), "ler": s["ler"],
            "not_converged": s["not_converged"], "osd_invalid": s["osd_invalid"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04_osd_order.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--mc-trials", type=int, default=2000000)
    ap.add_argument("--ler-trials", type=int, default=1000000)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batch": {}, "monte_carlo_p0.05": {}, "ler_144": {}}
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        res["batch"][name] = batch_rates(name, args.batch)
        print(name, json.dumps(res["batch"][name]), flush=True)
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        res["monte_carlo_p0.05"][name] = {label: mc_rate(name, 0.05, args.mc_trials, method, w)
                                         for label, method, w in METHODS[:2]}
        print(name, json.dumps(res["monte_carlo_p0.05"][name]), flush=True)
    name = "[[144, 12, 12]]"
    ps = [0.03, 0.05, 0.07]
    for label, method, w in METHODS[:2]:
        table = mc.run_sweep(name, ps, args.ler_trials, osd=True, osd_method=method, osd_order=w, seed=0)
        res["ler_144"][label] = {str(p): {"ler": mc.summarize(row)["ler"], "logical_errors": int(row[1]),
                                          "not_converged": int(row[6]), "osd_invalid": int(row[10]),
                                          "trials": int(row[0])}
                                 for p, row in zip(ps, table)}
        print(label, json.dumps(res["ler_144"][label]), flush=True)
    res["ler_144"]["config"] = {"max_iter": 50, "draws": 1, "seed": 0, "trials_per_point": args.ler_trials}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
