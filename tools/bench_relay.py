#!/usr/bin/env python3
"""Timing and logical error rate of BP(50) + Relay-BP (QBP_FLAG_RELAY) against BP(50) + OSD-0 and BP(50) + CS-7.

[[144,12,12]] and [[288,12,18]], p in {0.03, 0.05}, 1e6 trials, device-resident, best of three after a warm-up, the
three pipelines timed alternately inside each repetition:
  relay   qbp_mc_run_device | QBP_FLAG_RELAY, 10 legs x 30 iterations, stop_after = 3, gamma0 = 0.125,
          interval [-0.24, 0.66], alpha = 0.9                                                          (this build)
  osd0    qbp_mc_run_device | QBP_FLAG_OSD0                  (--baseline-lib: the library of the parent commit)
  cs7     qbp_mc_run_device | OSD-CS order 7                                                      (likewise)
and their LERs from the counters of the timed runs (same trials: one seed).  Then the batch kernel alone:
qbp_relay_decode_batch_device on 65 536 BP failures of [[144,12,12]] at p = 0.05 against qbp_osd_batch_device (OSD-0)
on the same records.  Nobody set a threshold: times and LERs are reported.
With --baseline-lib the Relay pipeline and the batch kernel of that library run too (relay_parent, relay_batch_parent),
alternately with this build's, and "vs_parent" has per item the parent's run-to-run spread (max - min) / min, the ratio
of the best times (this build / parent) and whether the ratio stays within 1 + spread.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_relay.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r12_relay.json
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

from qldpc_amd import _lib, bp, codes, mc, relay  # noqa: E402

MAX_ITER, SEED = 50, 2026
LEGS, ITERS, STOP, GAMMA0, INTERVAL, ALPHA = 10, 30, 3, 0.125, (-0.24, 0.66), 0.9


class BaselineDecoder:
    """qbp_mc_run_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_device", "qbp_relay_configure",
                     "qbp_relay_decode_batch_device", "qbp_last_error"):
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

    def relay_configure(self, cfg):
        rc = self.lib.qbp_relay_configure(self.h, cfg.gammas.ctypes.data, cfg.gammas.shape[0], cfg.leg_iters.ctypes.data,
                                          cfg.stop_after, cfg.alpha, cfg.clip_llr)
        if rc:
            raise RuntimeError(f"baseline qbp_relay_configure: {rc} {self.lib.qbp_last_error().decode()}")

    def relay_decode_device(self, d_syn, d_prior, B, d_hard, d_conv, d_iters, d_llr, d_legs, d_sol, stream=0):
        rc = self.lib.qbp_relay_decode_batch_device(self.h, d_syn, d_prior, int(B), d_hard or None, d_conv or None,
                                                    d_iters or None, d_llr or None, d_legs or None, d_sol or None,
                                                    stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_relay_decode_batch_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def vs_parent(new, parent):
    """The parent's spread over its repetitions, the ratio of the best times, and the verdict of the two."""
    spread = (max(parent) - min(parent)) / min(parent)
    ratio = min(new) / min(parent)
    return {"new_seconds": new, "parent_seconds": parent, "parent_spread": spread, "ratio_best": ratio,
            "within_spread": ratio <= 1.0 + spread}


def timed_mc(torch, dec, code, p, trials, flags):
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
                          seed=SEED, max_iter=MAX_ITER, flags=flags, stream=stream)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, d_cnt.cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit for the two OSD pipelines")
    ap.add_argument("--trials", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    result = {"max_iter": MAX_ITER, "trials": args.trials, "relay": dict(legs=LEGS, iters=ITERS, stop_after=STOP,
              gamma0=GAMMA0, interval=INTERVAL, alpha=ALPHA), "baseline_lib": args.baseline_lib, "points": []}
    for name in ("[[144, 12, 12]]", "[[288, 12, 18]]"):
        code = codes.load_code(name)
        dec = bp.decoder_for(code.Hx)
        cfg = relay.RelayConfig(relay.relay_gammas(code.n, LEGS, GAMMA0, INTERVAL, SEED), [ITERS] * LEGS, STOP, ALPHA)
        dec.relay_configure(cfg)
        base = BaselineDecoder(args.baseline_lib, code.Hx) if args.baseline_lib else dec
        runs = {"relay": (dec, _lib.FLAG_RELAY), "osd0": (base, _lib.FLAG_OSD0), "cs7": (base, _lib.osd_flags("cs", 7))}
        if base is not dec:
            base.relay_configure(cfg)
            runs["relay_parent"] = (base, _lib.FLAG_RELAY)
        for p in (0.03, 0.05):
            for d, fl in runs.values():                                   # warm-up
                timed_mc(torch, d, code, p, min(args.trials, 65536), fl)
            best, cnt, raw = {}, {}, {key: [] for key in runs}
            for _ in range(args.reps):
                for key, (d, fl) in runs.items():
                    t, c = timed_mc(torch, d, code, p, args.trials, fl)
                    raw[key].append(t)
                    if key not in best or t < best[key]:
                        best[key] = t
                    cnt[key] = c
            row = {"code": name, "p": p}
            if "relay_parent" in runs:
                row["vs_parent"] = vs_parent(raw["relay"], raw["relay_parent"])
            for key in runs:
                row[key] = {"seconds": best[key], "trials_per_s": args.trials / best[key], "ler": cnt[key][1] / cnt[key][0],
                            "not_converged": int(cnt[key][6]), "without_solution": int(cnt[key][10])}
            print(json.dumps(row))
            result["points"].append(row)
        if base is not dec:
            base.close()

    # the batch kernel alone, against OSD-0 on the same BP failures
    code = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(code.Hx)
    p, prior = 0.05, mc.prior_of(0.05, code.n)
    syn_f, llr_f, hard_f = [], [], []
    rng = np.random.default_rng(SEED)
    while sum(len(s) for s in syn_f) < args.records:
        err = (rng.random((1 << 18, code.n)) < p).astype(np.uint8)
        syn = (err @ np.asarray(code.Hx).T % 2).astype(np.uint8)
        hard, conv, _, llr = dec.decode(syn, prior, MAX_ITER)
        syn_f.append(syn[~conv]); llr_f.append(llr[~conv]); hard_f.append(hard[~conv])
    syn = np.concatenate(syn_f)[:args.records]
    dev = torch.device("cuda", 0)
    d_syn = torch.from_numpy(syn).to(dev)
    d_llr = torch.from_numpy(np.concatenate(llr_f)[:args.records]).to(dev)
    d_hard = torch.from_numpy(np.concatenate(hard_f)[:args.records]).to(dev)
    d_prior = torch.from_numpy(prior).to(dev)
    d_out = torch.zeros_like(d_hard)
    d_conv = torch.zeros(len(syn), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {"relay_batch": [], "osd0_batch": []}
    batch = {"relay_batch": dec}
    if args.baseline_lib:
        batch["relay_batch_parent"] = BaselineDecoder(args.baseline_lib, code.Hx)
        batch["relay_batch_parent"].relay_configure(cfg)
        times["relay_batch_parent"] = []
    for rep in range(args.reps + 1):
        for key in times:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if key in batch:
                batch[key].relay_decode_device(d_syn.data_ptr(), d_prior.data_ptr(), len(syn), d_out.data_ptr(),
                                               d_conv.data_ptr(), 0, 0, 0, 0, stream=stream)
            else:
                dec.osd0_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(syn), d_out.data_ptr(),
                                stream=stream)
            torch.cuda.synchronize(dev)
            if rep:
                times[key].append(time.perf_counter() - t0)
    result["batch"] = {"code": "[[144, 12, 12]]", "p": p, "records": len(syn), "solved_by_relay": int(d_conv.sum().item()),
                       **{k: {"seconds": min(v), "records_per_s": len(syn) / min(v)} for k, v in times.items()}}
    if args.baseline_lib:
        result["batch"]["vs_parent"] = vs_parent(times["relay_batch"], times["relay_batch_parent"])
        batch["relay_batch_parent"].close()
    print(json.dumps(result["batch"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
