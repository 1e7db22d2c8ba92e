#!/usr/bin/env python3
"""Monte-Carlo on detector error models (qbp_mc_run_probs), on one GPU:

1. overhead of the per-column threshold table: qbp_mc_run_device(p) and qbp_mc_run_probs_device at all-equal p,
   alternated in timed windows (>= --window s each) on [[288,12,18]] at p = 0.01 (bench.py's mc288_p0.01 leg) and
   on the 864 x 2592 phenomenological matrix of [[144,12,12]];
2. trials/s and logical error rates of BP(50) + OSD-0 at a few (p, q) points of the phenomenological models of
   [[144,12,12]] (12 rounds) and [[288,12,18]] (18 rounds), and of a synthetic DEM of circuit-level size.

    python tools/bench_dem.py --out profiles/r05_bench_dem.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qldpc_amd import bp, codes, dem, mc  # noqa: E402


def synthetic_dem(m=1008, n_target=9000, seed=0):
    """A DEM of circuit-level size: phenomenological [[144,12,12]] columns over 14 rounds (m = 1008) plus
    hyperedges of weight 2-6 among nearby detectors, some flipping observables, until n ~ n_target."""
    rng = np.random.default_rng(seed)
    H, L, probs = dem.phenomenological("[[144, 12, 12]]", 14, 1.0, 1.0)
    H = H.tocsc()
    lines = []
    for v in range(H.shape[1]):
        toks = [f"D{d}" for d in H.indices[H.indptr[v]:H.indptr[v + 1]]] + [f"L{o}" for o in np.flatnonzero(L[:, v])]
        lines.append(f"error({float(rng.uniform(2e-4, 2e-3))!r}) " + " ".join(toks))
    while len(lines) < n_target:
        w = int(rng.integers(2, 7))
        base = int(rng.integers(0, m - 150))
        dets = sorted(set(int(x) for x in base + rng.choice(150, size=w, replace=False)))
        obs = [f"L{o}" for o in np.flatnonzero(rng.random(12) < 0.05)]
        lines.append(f"error({float(rng.uniform(5e-5, 1e-3))!r}) " + " ".join([f"D{d}" for d in dets] + obs))
    return dem.parse_dem("\n".join(lines))


def overhead(dec, L, distance, p, n, T, window, rounds, dev, torch):
    """Median and spread of (probs path rate) / (uniform path rate) over `rounds` alternations."""
    stream = torch.cuda.current_stream(dev)
    prior = torch.from_numpy(mc.prior_of(p, n)).to(dev)
    cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    probs = np.full(n, p)

    def uniform(a, b):
        dec.mc_run_device(L, distance, p, prior.data_ptr(), a, b, cnt.data_ptr(), stream=stream.cuda_stream)

    def table(a, b):
        dec.mc_run_probs_device(L, distance, probs, prior.data_ptr(), a, b, cnt.data_ptr(), stream=stream.cuda_stream)

    def timed(fn, T):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        done = 0
        while True:
            fn(done, done + T)
            done += T
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            if dt >= window:
                return done / dt

    for fn in (uniform, table):          # warm-up: kernel images, thresholds uploaded, clocks up
        timed(fn, T)
    rates = {"uniform": [], "table": []}
    for r in range(rounds):
        order = (uniform, table) if r % 2 == 0 else (table, uniform)
        for fn in order:
            rates["uniform" if fn is uniform else "table"].append(timed(fn, T))
    ratio = np.array(rates["table"]) / np.array(rates["uniform"])
    return {"trials_per_call": T, "window_s": window, "rounds": rounds,
            "uniform_trials_per_s": rates["uniform"], "table_trials_per_s": rates["table"],
            "ratio_median": float(np.median(ratio)), "ratio_min": float(ratio.min()), "ratio_max": float(ratio.max()),
            "uniform_spread": float((max(rates["uniform"]) - min(rates["uniform"])) / np.median(rates["uniform"])),
            "kernel": dec.info("last_kernel")}


def rates(name, H, L, probs, trials, dev, torch):
    dec = bp.decoder_for(H)
    mc.run_dem(H, L, probs, min(trials, 20000), osd=True, device=dev.index)       # warm-up
    t0 = time.perf_counter()
    c = mc.run_dem(H, L, probs, trials, osd=True, device=dev.index)
    dt = time.perf_counter() - t0
    s = mc.summarize(c)
    return {"model": name, "m": int(H.shape[0]), "n": int(H.shape[1]), "trials": trials, "seconds": dt,
            "trials_per_s": trials / dt, "ler_bp_osd0": s["ler"], "ler_bp_only": s["ler_bp_only"],
            "not_converged": s["not_converged"] / trials, "mean_iterations": s["mean_iterations"],
            "kernel": dec.info("last_kernel"), "counters": c.tolist()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--trials", type=int, default=200000, help="trials per rate point")
    ap.add_argument("--skip-rates", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"overhead": {}, "rates": []}
    c288 = codes.load_code("[[288, 12, 18]]")
    out["overhead"]["mc288_p0.01"] = overhead(bp.decoder_for(c288.Hx), c288.Lx, c288.distance, 0.01, c288.n,
                                              1 << 20, args.window, args.rounds, dev, torch)
    print(json.dumps({"mc288_p0.01": {k: v for k, v in out["overhead"]["mc288_p0.01"].items()
                                      if "ratio" in k or "spread" in k}}), flush=True)
    H, L, _ = dem.phenomenological("[[144, 12, 12]]", 12, 0.0)
    out["overhead"]["st144_p0.005"] = overhead(bp.decoder_for(H), L, 12, 0.005, H.shape[1], 1 << 17,
                                               args.window, args.rounds, dev, torch)
    print(json.dumps({"st144_p0.005": {k: v for k, v in out["overhead"]["st144_p0.005"].items()
                                       if "ratio" in k or "spread" in k}}), flush=True)
    if not args.skip_rates:
        for code, T in (("[[144, 12, 12]]", 12), ("[[288, 12, 18]]", 18)):
            for p, q in ((0.002, 0.002), (0.004, 0.004), (0.004, 0.01)):
                H, L, probs = dem.phenomenological(code, T, p, q)
                r = rates(f"{code} phenomenological T={T} p={p} q={q}", H, L, probs, args.trials, dev, torch)
                out["rates"].append(r)
                print(json.dumps({k: v for k, v in r.items() if k != "counters"}), flush=True)
        H, L, probs = synthetic_dem()
        for scale in (1.0, 2.0):
            r = rates(f"synthetic DEM x{scale}", H, L, np.minimum(probs * scale, 0.5), args.trials, dev, torch)
            out["rates"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k != "counters"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
