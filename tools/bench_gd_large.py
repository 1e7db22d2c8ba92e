#!/usr/bin/env python3
"""What BP guided decimation's large build (QBP_OPT_GD_MEM: messages in a per-workgroup global workspace, the working
prior as two bit maps) costs and what it decodes.  Device-resident, best of three after a warm-up, the alternatives
timed alternately inside each repetition.

  (a) the price of global messages: the largest [[72,12,6]] phenomenological matrix that fits both builds of the variant
      (40 rounds for min-sum, 39 for sum-product), p = q = 0.02, 65 536 failures of BP(50, min-sum);
      qbp_gd_decode_batch_device with QBP_OPT_GD_MEM = 1 against the LDS build of --baseline-lib (the library of the
      parent commit; without it, the LDS build of this library, and the row says so).  "ratio" = seconds(large) /
      seconds(baseline LDS); "lds_here" is this library's LDS build on the same records.
  (b) 2592 x 7776 ([[288,12,18]], 18 rounds, p = q = 0.004), 1e5 trials: BP(50) + BPGD (large="auto") against BP(50) +
      OSD-0 and BP(50) + Relay-BP (large; the configuration of tools/bench_relay.py), both from --baseline-lib.
  (c) the same on the synthetic 1008 x 8991 detector error model of tools/bench_dem.py.
Rows (b) and (c) record trials/s, the unconverged share of the first stage, the LER and the records the second stage
leaves unsolved.  BPGD runs rounds of GD_T = 8 min-sum iterations and at most GD_ROUNDS = 32 decimations, chosen before
any run and not tuned on the LER.  Nobody set a threshold: times and rates are reported.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_gd_large.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r25_gd_large.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from qldpc_amd import _lib, bp, dem, gd, mc, relay  # noqa: E402
from bench_relay_large import dense  # noqa: E402
import bench_relay_large as brl  # noqa: E402

MAX_ITER, SEED, ALPHA = 50, 2026, 0.9
GD_T, GD_ROUNDS, GD_LLR = 8, 32, 25.0


class Baseline(brl.BaselineDecoder):
    """The parent library on the same matrix: the Monte-Carlo entry of bench_relay_large, BPGD's LDS build and Relay-BP's
    large build."""

    def __init__(self, path, H, device=0):
        super().__init__(path, H, device)
        for name in ("qbp_gd_configure", "qbp_gd_decode_batch_device", "qbp_relay_configure", "qbp_set_option"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]

    def check(self, rc, what):
        if rc:
            raise RuntimeError(f"baseline {what}: {rc} {self.lib.qbp_last_error().decode()}")

    def gd_configure(self, cfg):
        self.check(self.lib.qbp_gd_configure(self.h, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant,
                                             cfg.alpha, cfg.clip_llr), "qbp_gd_configure")

    def gd_decode_device(self, d_syn, d_prior, B, d_hard, d_conv, d_iters, d_llr, d_rounds, stream=0):
        self.check(self.lib.qbp_gd_decode_batch_device(self.h, d_syn, d_prior, int(B), d_hard or None, d_conv or None,
                                                       d_iters or None, d_llr or None, d_rounds or None, stream or None),
                   "qbp_gd_decode_batch_device")

    def relay_configure(self, cfg):
        self.check(self.lib.qbp_set_option(self.h, _lib.OPT_RELAY_MEM, _lib.RELAY_MEM[cfg.large]), "qbp_set_option")
        self.check(self.lib.qbp_relay_configure(self.h, cfg.gammas.ctypes.data, cfg.gammas.shape[0],
                                                cfg.leg_iters.ctypes.data, cfg.stop_after, cfg.alpha, cfg.clip_llr),
                   "qbp_relay_configure")


def gd_config(variant, large):
    return gd.GDConfig(GD_T, GD_ROUNDS, GD_LLR, variant, ALPHA, 20.0, large=large)


def row_a(torch, variant, records, reps, baseline_lib):
    sp = variant == _lib.SUM_PRODUCT
    T = 39 if sp else 40
    H, _, probs = dem.phenomenological("[[72, 12, 6]]", T, 0.02, 0.02)
    H = dense(H)
    n = H.shape[1]
    prior = mc.dem_prior(probs)
    dec = bp.decoder_for(H)
    rng = np.random.default_rng(SEED)
    fails, have = [], 0
    while have < records:
        err = (rng.random((8192, n)) < probs).astype(np.uint8)
        syn = ((err.astype(np.float32) @ H.T.astype(np.float32)) % 2).astype(np.uint8)
        conv = dec.decode(syn, prior, MAX_ITER, variant=_lib.MIN_SUM, alpha=ALPHA, want_llr=False)[1]
        fails.append(syn[~conv])
        have += len(fails[-1])
    syn = np.concatenate(fails)[:records]
    dev = torch.device("cuda", 0)
    d_syn, d_prior = torch.from_numpy(syn).to(dev), torch.from_numpy(prior).to(dev)
    d_hard = torch.zeros((records, n), dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(records, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dec.gd_configure(gd_config(variant, False))
    base = Baseline(baseline_lib, H) if baseline_lib else None
    if base:
        base.gd_configure(gd_config(variant, False))

    def run(key):
        if key == "baseline":
            d = base
        else:
            d = dec
            dec.set_option(_lib.OPT_GD_MEM, 1 if key == "large" else 0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        d.gd_decode_device(d_syn.data_ptr(), d_prior.data_ptr(), records, d_hard.data_ptr(), d_conv.data_ptr(), 0, 0, 0,
                           stream=stream)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    keys = ["large", "lds_here"] + (["baseline"] if base else [])
    times, geometry, solved, outputs = {k: [] for k in keys}, {}, {}, {}
    for rep in range(reps + 1):
        for key in keys:
            t = run(key)
            if rep:
                times[key].append(t)
            else:
                if key != "baseline":
                    geometry[key] = {k: dec.info(k) for k in ("threads", "grid", "lds_bytes")}
                solved[key] = int(d_conv.sum().item())
                outputs[key] = d_hard.cpu().numpy().copy()
    for key in keys[1:]:
        if not np.array_equal(outputs["large"], outputs[key]) or solved["large"] != solved[key]:
            raise SystemExit(f"row (a): the large build and {key} disagree on the hard decisions")
    ref = "baseline" if base else "lds_here"
    row = {"row": "a", "variant": "sum_product" if sp else "min_sum", "matrix": list(H.shape), "p": 0.02,
           "records": records, "solved": solved["large"], "baseline": "parent library" if base else "this library",
           "ratio": min(times["large"]) / min(times[ref])}
    for key in keys:
        row[key] = {"seconds": min(times[key]), "all_seconds": times[key], "records_per_s": records / min(times[key]),
                    **geometry.get(key, {})}
    if base:
        base.close()
    return row


def row_mc(torch, tag, H, L, probs, distance, trials, reps, baseline_lib):
    H = dense(H)
    L = np.ascontiguousarray(L, np.uint8)
    n = H.shape[1]
    dec = bp.decoder_for(H)
    dec.gd_configure(gd_config(_lib.MIN_SUM, "auto"))
    runs = {"gd_large": (dec, _lib.FLAG_GD)}
    base = None
    if baseline_lib:
        base = Baseline(baseline_lib, H)
        base.relay_configure(relay.RelayConfig(relay.relay_gammas(n, brl.LEGS, brl.GAMMA0, brl.INTERVAL, brl.SEED),
                                               [brl.ITERS] * brl.LEGS, brl.STOP, brl.ALPHA, large=True))
        runs["osd0"] = (base, _lib.FLAG_OSD0)
        runs["relay_large"] = (base, _lib.FLAG_RELAY)
    d_prior = torch.from_numpy(mc.dem_prior(probs)).to(torch.device("cuda", 0))
    for d, fl in runs.values():                                                   # warm-up
        brl.timed_mc(torch, d, L, distance, probs, d_prior, min(trials, 8192), fl)
    geometry = {k: dec.info(k) for k in ("threads", "grid", "lds_bytes")}
    best, cnt = {}, {}
    for _ in range(reps):
        for key, (d, fl) in runs.items():
            t, c = brl.timed_mc(torch, d, L, distance, probs, d_prior, trials, fl)
            best[key] = min(best.get(key, t), t)
            cnt[key] = c
    row = {"row": tag, "matrix": list(H.shape), "trials": trials, "gd_launch": geometry}
    for key in runs:
        row[key] = {"seconds": best[key], "trials_per_s": trials / best[key], "ler": cnt[key][1] / cnt[key][0],
                    "unconverged_share": cnt[key][6] / cnt[key][0], "without_solution": int(cnt[key][10])}
    if base:
        base.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit")
    ap.add_argument("--trials", type=int, default=100_000)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench_dem import synthetic_dem

    result = {"max_iter": MAX_ITER, "gd": dict(iters_per_round=GD_T, max_rounds=GD_ROUNDS, decim_llr=GD_LLR, alpha=ALPHA),
              "baseline_lib": args.baseline_lib, "rows": []}
    for tag in args.rows:
        if tag == "a":
            rows = [row_a(torch, v, args.records, args.reps, args.baseline_lib) for v in (_lib.MIN_SUM, _lib.SUM_PRODUCT)]
        elif tag == "b":
            H, L, probs = dem.phenomenological("[[288, 12, 18]]", 18, 0.004, 0.004)
            rows = [row_mc(torch, "b", H, L, probs, 18, args.trials, args.reps, args.baseline_lib)]
        else:
            H, L, probs = synthetic_dem()
            rows = [row_mc(torch, "c", H, L, probs, 0, args.trials, args.reps, args.baseline_lib)]
        for row in rows:
            print(json.dumps(row), flush=True)
            result["rows"].append(row)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
