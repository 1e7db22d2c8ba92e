#!/usr/bin/env python3
"""Timing, logical error rate and cluster size of BP(50) + localized statistics decoding (QBP_FLAG_LSD) against BP(50) +
OSD-0.

[[144,12,12]] and [[288,12,18]], p in {0.03, 0.05}, 1e6 trials, device-resident, best of three after a warm-up, the
pipelines timed alternately inside each repetition:
  lsd1    qbp_mc_run_device | QBP_FLAG_LSD, bits_per_step = 1                                        (this build)
  lsd0    qbp_mc_run_device | QBP_FLAG_LSD, bits_per_step = 0 (all neighbours per round)              (this build)
  osd0    qbp_mc_run_device | QBP_FLAG_OSD0                  (--baseline-lib: the library of the parent commit)
and per pipeline the LER, the fraction of trials whose result misses the syndrome and trials/s from the counters of the
timed runs (same trials: one seed).  Then the batch kernel alone: qbp_lsd_batch_device (g = 1 and g = 0) on 65 536 BP
failures of each code at p = 0.05 against qbp_osd0_batch_device on the same records, with the mean of stats[1] (the
variables the clusters absorbed).  Nobody set a threshold: figures are reported.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_lsd.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r16_lsd.json
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

from qldpc_amd import _lib, bp, codes, mc  # noqa: E402

MAX_ITER, SEED = 50, 2026


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

    def mc_run_device(self, L, distance, p, d_prior, begin, end, d_counters, flags=0, stream=0, **kw):
        L = np.ascontiguousarray(L, np.uint8)
        rc = self.lib.qbp_mc_run_device(self.h, L.ctypes.data, L.shape[0], int(distance), float(p), 1, SEED, int(begin),
                                        int(end), d_prior, MAX_ITER, 0, 1.0, 1.0, 20.0, int(flags), d_counters,
                                        stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def timed_mc(torch, dec, code, p, trials, flags, g=None):
    """Seconds and counters of one device-resident run of `trials` trials, split by the record limit."""
    dev = torch.device("cuda", 0)
    if g is not None:
        dec.lsd_configure(g)
    d_prior = torch.from_numpy(mc.prior_of(p, code.n)).to(dev)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    step = _lib.MC_OSD_MAX_TRIALS
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for a in range(0, trials, step):
        dec.mc_run_device(code.Lx, code.distance, p, d_prior.data_ptr(), a, min(a + step, trials), d_cnt.data_ptr(),
                          seed=SEED, max_iter=MAX_ITER, flags=flags, stream=stream)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, d_cnt.cpu().numpy()


def batch_point(torch, name, records, reps):
    """lsd_kernel (g = 1, g = 0) against osd0_kernel on `records` BP(50) failures of the code at p = 0.05."""
    code = codes.load_code(name)
    dec = bp.decoder_for(code.Hx)
    p, prior = 0.05, mc.prior_of(0.05, code.n)
    syn_f, llr_f, hard_f = [], [], []
    rng = np.random.default_rng(SEED)
    while sum(len(s) for s in syn_f) < records:
        err = (rng.random((1 << 18, code.n)) < p).astype(np.uint8)
        syn = (err @ np.asarray(code.Hx).T % 2).astype(np.uint8)
        hard, conv, _, llr = dec.decode(syn, prior, MAX_ITER)
        syn_f.append(syn[~conv]); llr_f.append(llr[~conv]); hard_f.append(hard[~conv])
    syn = np.concatenate(syn_f)[:records]
    dev = torch.device("cuda", 0)
    d_syn = torch.from_numpy(syn).to(dev)
    d_llr = torch.from_numpy(np.concatenate(llr_f)[:records]).to(dev)
    d_hard = torch.from_numpy(np.concatenate(hard_f)[:records]).to(dev)
    d_out = torch.zeros_like(d_hard)
    d_stats = torch.zeros((len(syn), 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {"lsd1_batch": [], "lsd0_batch": [], "osd0_batch": []}
    extra = {}
    for rep in range(reps + 1):
        for key in times:
            if key != "osd0_batch":
                dec.lsd_configure(1 if key == "lsd1_batch" else 0)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if key == "osd0_batch":
                dec.osd0_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(syn), d_out.data_ptr(),
                                stream=stream)
            else:
                dec.lsd_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(syn), d_out.data_ptr(),
                               d_stats.data_ptr(), stream=stream)
            torch.cuda.synchronize(dev)
            if rep:
                times[key].append(time.perf_counter() - t0)
            if key != "osd0_batch":
                st = d_stats.cpu().numpy()
                extra[key] = {"mean_active_variables": float(st[:, 1].mean()), "mean_rounds": float(st[:, 0].mean()),
                              "mean_clusters": float(st[:, 2].mean()), "valid_fraction": float(st[:, 3].mean())}
    return {"code": name, "p": p, "records": len(syn),
            **{k: {"seconds": min(v), "records_per_s": len(syn) / min(v), **extra.get(k, {})} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit for the OSD-0 pipeline")
    ap.add_argument("--trials", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    result = {"max_iter": MAX_ITER, "trials": args.trials, "baseline_lib": args.baseline_lib, "points": [], "batch": []}
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        code = codes.load_code(name)
        dec = bp.decoder_for(code.Hx)
        base = BaselineDecoder(args.baseline_lib, code.Hx) if args.baseline_lib else dec
        runs = {"lsd1": (dec, _lib.FLAG_LSD, 1), "lsd0": (dec, _lib.FLAG_LSD, 0), "osd0": (base, _lib.FLAG_OSD0, None)}
        for p in (0.03, 0.05):
            for d, fl, g in runs.values():                                # warm-up
                timed_mc(torch, d, code, p, min(args.trials, 65536), fl, g)
            best, cnt = {}, {}
            for _ in range(args.reps):
                for key, (d, fl, g) in runs.items():
                    t, c = timed_mc(torch, d, code, p, args.trials, fl, g)
                    if key not in best or t < best[key]:
                        best[key] = t
                    cnt[key] = c
            row = {"code": name, "p": p}
            for key in runs:
                row[key] = {"seconds": best[key], "trials_per_s": args.trials / best[key], "ler": cnt[key][1] / cnt[key][0],
                            "not_converged": int(cnt[key][6]), "invalid_fraction": int(cnt[key][10]) / int(cnt[key][0])}
            print(json.dumps(row))
            result["points"].append(row)
        if base is not dec:
            base.close()
        result["batch"].append(batch_point(torch, name, args.records, args.reps))
        print(json.dumps(result["batch"][-1]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
