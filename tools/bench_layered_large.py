#!/usr/bin/env python3
"""What layered BP's large build (QBP_OPT_LAYERED_MEM: the messages of every slot in a per-workgroup global workspace)
costs and what it decodes.  Device-resident, best of three after a warm-up, the alternatives timed alternately inside
each repetition.

  (a) the price of global messages: 39 rounds of the [[72,12,6]] phenomenological matrix (1404 x 4212, the largest
      that fits both builds), p = q = 0.01, 65 536 syndromes; qbp_decode_batch_device with QBP_FLAG_LAYERED, BP(50),
      both variants, QBP_OPT_LAYERED_MEM = 0 against 1 on the same records.  "ratio" = seconds(1) / seconds(0).
  (b) 2592 x 7776 ([[288,12,18]], 18 rounds, p = q = 0.004), 1e5 trials, both variants: layered BP(50) (large build)
      + OSD-0 against flooding BP(50) + OSD-0 (--baseline-lib: the library of the parent commit; without it the
      flooding pipeline of this build, whose kernels the option does not touch).
  (c) the same on the synthetic 1008 x 8991 detector error model of tools/bench_dem.py.
Rows (b) and (c) record iterations per syndrome, the unconverged share, the LER and trials/s.  Nobody set a threshold:
times and rates are reported.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_layered_large.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r24_layered_large.json
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

from qldpc_amd import _lib, bp, dem, mc  # noqa: E402
from bench_relay_large import BaselineDecoder, dense  # noqa: E402

MAX_ITER, SEED, ALPHA = 50, 2026, 0.8
VARIANTS = {"sum_product": (_lib.SUM_PRODUCT, 1.0), "min_sum": (_lib.MIN_SUM, ALPHA)}
INFO = ("threads", "grid", "lds_bytes")


def row_a(torch, records, reps):
    H, _, probs = dem.phenomenological("[[72, 12, 6]]", 39, 0.01, 0.01)
    H = dense(H)
    m, n = H.shape
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    d_H = torch.from_numpy(H.T.astype(np.float32)).to(dev)
    d_probs = torch.from_numpy(probs).to(dev)
    d_syn = torch.empty((records, m), dtype=torch.uint8, device=dev)
    for a in range(0, records, 8192):
        b = min(a + 8192, records)
        err = (torch.rand((b - a, n), generator=gen, device=dev, dtype=torch.float64) < d_probs).to(torch.float32)
        d_syn[a:b] = torch.remainder(err @ d_H, 2).to(torch.uint8)
    d_prior = torch.from_numpy(mc.dem_prior(probs)).to(dev)
    d_hard = torch.zeros((records, n), dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(records, dtype=torch.uint8, device=dev)
    d_iters = torch.zeros(records, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dec = bp.decoder_for(H)
    dec.layered_configure(None)
    row = {"row": "a", "matrix": [m, n], "p": 0.01, "records": records}
    for name, (variant, alpha) in VARIANTS.items():
        times, geometry, outputs = {0: [], 1: []}, {}, {}
        for rep in range(reps + 1):
            for mem in (0, 1):
                dec.set_option(_lib.OPT_LAYERED_MEM, mem)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                dec.decode_device(d_syn.data_ptr(), d_prior.data_ptr(), records, MAX_ITER, variant, alpha, 1.0, 20.0,
                                  _lib.FLAG_LAYERED, d_hard.data_ptr(), d_conv.data_ptr(), d_iters.data_ptr(), 0, stream)
                torch.cuda.synchronize(dev)
                if rep:
                    times[mem].append(time.perf_counter() - t0)
                else:
                    geometry[mem] = {k: dec.info(k) for k in INFO}
                    outputs[mem] = (d_hard.cpu().numpy().copy(), d_conv.cpu().numpy().copy(), d_iters.cpu().numpy().copy())
        if not all(np.array_equal(x, y) for x, y in zip(outputs[0], outputs[1])):
            raise SystemExit(f"row (a), {name}: the two builds disagree")
        conv, iters = outputs[0][1].astype(bool), outputs[0][2]
        row[name] = {"converged_share": float(conv.mean()), "iterations_per_syndrome": float((iters + 1).mean()),
                     "lds": {"seconds": min(times[0]), "records_per_s": records / min(times[0]), **geometry[0]},
                     "large": {"seconds": min(times[1]), "records_per_s": records / min(times[1]), **geometry[1]},
                     "ratio": min(times[1]) / min(times[0])}
    dec.set_option(_lib.OPT_LAYERED_MEM, 0)
    return row


def timed_mc(torch, dec, L, distance, probs, d_prior, trials, variant, alpha, flags):
    dev = torch.device("cuda", 0)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    step = dec.mc_osd_step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for a in range(0, trials, step):
        if isinstance(dec, BaselineDecoder):
            L8, pr = np.ascontiguousarray(L, np.uint8), np.ascontiguousarray(probs, np.float64)
            rc = dec.lib.qbp_mc_run_probs_device(dec.h, L8.ctypes.data, L8.shape[0], int(distance), pr.ctypes.data, 1, SEED, a,
                                                 min(a + step, trials), d_prior.data_ptr(), MAX_ITER, int(variant),
                                                 float(alpha), 1.0, 20.0, int(flags), d_cnt.data_ptr(), stream or None)
            if rc:
                raise RuntimeError(f"baseline qbp_mc_run_probs_device: {rc} {dec.lib.qbp_last_error().decode()}")
        else:
            dec.mc_run_probs_device(L, distance, probs, d_prior.data_ptr(), a, min(a + step, trials), d_cnt.data_ptr(),
                                    seed=SEED, max_iter=MAX_ITER, variant=variant, alpha=alpha, flags=flags, stream=stream)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, d_cnt.cpu().numpy()


def row_mc(torch, tag, H, L, probs, distance, trials, reps, baseline_lib):
    H = dense(H)
    L = np.ascontiguousarray(L, np.uint8)
    dec = bp.decoder_for(H)
    dec.layered_configure(None, large=True)
    base = BaselineDecoder(baseline_lib, H) if baseline_lib else dec
    d_prior = torch.from_numpy(mc.dem_prior(probs)).to(torch.device("cuda", 0))
    row = {"row": tag, "matrix": list(H.shape), "trials": trials}
    for name, (variant, alpha) in VARIANTS.items():
        runs = {"layered_large": (dec, _lib.FLAG_LAYERED | _lib.FLAG_OSD0), "flooding": (base, _lib.FLAG_OSD0)}
        for d, fl in runs.values():                                                   # warm-up
            timed_mc(torch, d, L, distance, probs, d_prior, min(trials, 8192), variant, alpha, fl)
        timed_mc(torch, dec, L, distance, probs, d_prior, 256, variant, alpha, _lib.FLAG_LAYERED)
        geometry = {k: dec.info(k) for k in INFO}                                     # (the layered launch, not OSD's)
        best, cnt = {}, {}
        for _ in range(reps):
            for key, (d, fl) in runs.items():
                t, c = timed_mc(torch, d, L, distance, probs, d_prior, trials, variant, alpha, fl)
                best[key] = min(best.get(key, t), t)
                cnt[key] = c
        row[name] = {"layered_launch": geometry}
        for key in runs:
            c = cnt[key]
            row[name][key] = {"seconds": best[key], "trials_per_s": trials / best[key], "ler": c[1] / c[0],
                              "unconverged_share": c[6] / c[0], "iterations_per_syndrome": c[7] / c[0] + 1.0,
                              "osd_invalid": int(c[10])}
    if base is not dec:
        base.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit for the flooding pipelines")
    ap.add_argument("--trials", type=int, default=100_000)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench_dem import synthetic_dem

    result = {"max_iter": MAX_ITER, "alpha_min_sum": ALPHA, "baseline_lib": args.baseline_lib, "rows": []}
    for tag in args.rows:
        if tag == "a":
            row = row_a(torch, args.records, args.reps)
        elif tag == "b":
            H, L, probs = dem.phenomenological("[[288, 12, 18]]", 18, 0.004, 0.004)
            row = row_mc(torch, "b", H, L, probs, 18, args.trials, args.reps, args.baseline_lib)
        else:
            H, L, probs = synthetic_dem()
            row = row_mc(torch, "c", H, L, probs, 0, args.trials, args.reps, args.baseline_lib)
        print(json.dumps(row), flush=True)
        result["rows"].append(row)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
