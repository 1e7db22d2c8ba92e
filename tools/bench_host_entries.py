#!/usr/bin/env python3
"""Host-array entry points of two builds of libqbp.so against each other on [[288, 12, 18]]: the library of the tree
and --baseline-lib (the parent commit's), alternating in one process, --reps repetitions each after one warm-up.

  a  one-syndrome qbp_decode_batch calls (the drop-in's usage): seconds per call over --calls calls
  b  one qbp_decode_batch of 125 000 syndromes with all outputs
  c  qbp_relay_decode_batch, B = 10 000
  d  qbp_mc_run_probs over 10^6 trials

Per workload: the best time of each build, their ratio, and the parent's spread (max - min) / min over its repetitions;
"within_spread" says whether the ratio lies within that spread of 1.  Whichever library is loaded first measures a few
per cent slower in the one-syndrome workload, the same library against a copy of itself included: --parent-loads-first
gives the other order, and the two ratios bracket the effect of the code.

    python tools/bench_host_entries.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r18_host_entries.json
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

MAX_ITER, P, SEED = 50, 0.02, 2026
ENTRIES = ("qbp_create", "qbp_destroy", "qbp_last_error", "qbp_decode_batch", "qbp_relay_configure",
           "qbp_relay_decode_batch", "qbp_mc_run_probs")


class Build:
    """One build of the library with a handle on H."""

    def __init__(self, path, H, device):
        _lib._preload_hip_runtime()
        self.lib = C.CDLL(path)
        for name in ENTRIES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.rp, self.ci, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        self.ok(self.lib.qbp_create(self.rp.ctypes.data, self.ci.ctypes.data, self.m, self.n, device, C.byref(self.h)))

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"libqbp error {rc}: {self.lib.qbp_last_error().decode()}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--only", default="", help="run the workloads whose name contains this")
    ap.add_argument("--parent-first", action="store_true", help="the parent's build runs first in every pair")
    ap.add_argument("--parent-loads-first", action="store_true",
                    help="the parent's library is loaded, and its handle created, before this build's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    code = codes.load_code("[[288, 12, 18]]")
    H, L = np.ascontiguousarray(code.Hx, np.uint8), np.ascontiguousarray(code.Lx, np.uint8)
    m, n = H.shape
    paths = {"new": _lib.LIB_PATH, "parent": args.baseline_lib}
    builds = {key: Build(paths[key], H, bp.DEVICE) for key in (("parent", "new") if args.parent_loads_first else ("new", "parent"))}
    rng = np.random.default_rng(SEED)
    err = (rng.random((125000, n)) < P).astype(np.uint8)
    syn = ((err.astype(np.float32) @ H.T.astype(np.float32)).astype(np.int64) & 1).astype(np.uint8)
    prior, probs = mc.prior_of(P, n), np.full(n, P)
    cfg = relay.RelayConfig(relay.relay_gammas(n, 10, 0.125, (-0.24, 0.66), SEED), [30] * 10, 3, 0.9)
    for b in builds.values():
        b.ok(b.lib.qbp_relay_configure(b.h, cfg.gammas.ctypes.data, cfg.gammas.shape[0], cfg.leg_iters.ctypes.data,
                                       cfg.stop_after, cfg.alpha, cfg.clip_llr))

    def outputs(B):
        return [np.empty((B, n), np.uint8), np.empty(B, np.uint8), np.empty(B, np.int32), np.empty((B, n), np.float64)]

    def decode(b, B, calls):
        outs = outputs(B)
        t0 = time.perf_counter()
        for i in range(calls):
            b.ok(b.lib.qbp_decode_batch(b.h, syn[i * B:].ctypes.data, prior.ctypes.data, B, MAX_ITER, _lib.SUM_PRODUCT,
                                        1.0, 1.0, 20.0, 0, *(o.ctypes.data for o in outs)))
        return (time.perf_counter() - t0) / calls, outs

    def relay_decode(b):
        B = 10000
        outs = outputs(B) + [np.empty(B, np.int32), np.empty(B, np.int32)]
        t0 = time.perf_counter()
        b.ok(b.lib.qbp_relay_decode_batch(b.h, syn.ctypes.data, prior.ctypes.data, B, *(o.ctypes.data for o in outs)))
        return time.perf_counter() - t0, outs

    def mc_probs(b):
        cnt = np.zeros(_lib.NUM_COUNTERS, np.int64)
        t0 = time.perf_counter()
        b.ok(b.lib.qbp_mc_run_probs(b.h, L.ctypes.data, L.shape[0], code.distance, probs.ctypes.data, 1, SEED, 0, 10**6,
                                    prior.ctypes.data, MAX_ITER, _lib.SUM_PRODUCT, 1.0, 1.0, 20.0, 0, cnt.ctypes.data))
        return time.perf_counter() - t0, [cnt]

    work = {"a_one_syndrome_call": lambda b: decode(b, 1, args.calls), "b_decode_125000": lambda b: decode(b, 125000, 1),
            "c_relay_10000": relay_decode, "d_mc_run_probs_1e6": mc_probs}
    doc = {"code": "[[288, 12, 18]]", "p": P, "max_iter": MAX_ITER, "reps": args.reps, "calls": args.calls,
           "baseline_lib": os.path.basename(os.path.dirname(os.path.abspath(args.baseline_lib))) + "/" + os.path.basename(args.baseline_lib),
           "first_of_a_pair": "parent" if args.parent_first else "new",
           "loaded_first": "parent" if args.parent_loads_first else "new", "workloads": {}}
    order = ("parent", "new") if args.parent_first else ("new", "parent")
    for name, fn in work.items():
        if args.only not in name:
            continue
        times = {"new": [], "parent": []}
        results = {}
        for rep in range(-1, args.reps):                # (rep -1: warm-up, not recorded)
            for key in order:
                seconds, outs = fn(builds[key])
                results[key] = outs
                if rep >= 0:
                    times[key].append(seconds)
        same = all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(results["new"], results["parent"]))
        spread = (max(times["parent"]) - min(times["parent"])) / min(times["parent"])
        ratio = min(times["new"]) / min(times["parent"])
        doc["workloads"][name] = {"new_seconds": times["new"], "parent_seconds": times["parent"], "parent_spread": spread,
                                  "ratio_best": ratio, "within_spread": abs(ratio - 1.0) <= spread,
                                  "same_results": bool(same)}
        print(f"{name}: best new {min(times['new']):.6g} s, best parent {min(times['parent']):.6g} s, ratio {ratio:.4f}, "
              f"parent spread {spread:.4f}, same results {same}", flush=True)
    for b in builds.values():
        b.lib.qbp_destroy(b.h)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
