#!/usr/bin/env python3
"""What Relay-BP's large build (QBP_OPT_RELAY_MEM: messages in a per-workgroup global workspace) costs and what it
decodes.  Device-resident, best of three after a warm-up, the alternatives timed alternately inside each repetition.

  (a) the price of global messages: 33 rounds of the [[72,12,6]] phenomenological matrix (1188 x 3564, the largest
      that fits both builds), p = q = 0.02, 65 536 failures of BP(50, min-sum); qbp_relay_decode_batch_device with
      QBP_OPT_RELAY_MEM = 0 against 1 on the same records.  "ratio" = seconds(1) / seconds(0).
  (b) 2592 x 7776 ([[288,12,18]], 18 rounds, p = q = 0.004), 1e5 trials: BP(50) + Relay-BP (the configuration of
      tools/bench_relay.py, large=True) against BP(50) + OSD-0 (--baseline-lib: the library of the parent commit).
  (c) the same on the synthetic 1008 x 8991 detector error model of tools/bench_dem.py.
Rows (b) and (c) record trials/s, the unconverged share of the first stage, the LER, and the records Relay-BP leaves
without a solution.  Nobody set a threshold: times and rates are reported.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_relay_large.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r23_relay_large.json
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

from qldpc_amd import _lib, bp, dem, mc, relay  # noqa: E402

MAX_ITER, SEED = 50, 2026
LEGS, ITERS, STOP, GAMMA0, INTERVAL, ALPHA = 10, 30, 3, 0.125, (-0.24, 0.66), 0.9


class BaselineDecoder:
    """qbp_mc_run_probs_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_probs_device", "qbp_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        rc = self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device, C.byref(self.h))
        if rc:
            raise RuntimeError(f"baseline qbp_create: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_run_probs_device(self, L, distance, probs, d_prior, begin, end, d_counters, seed=0, max_iter=50, flags=0,
                            stream=0):
        L = np.ascontiguousarray(L, np.uint8)
        probs = np.ascontiguousarray(probs, np.float64)
        rc = self.lib.qbp_mc_run_probs_device(self.h, L.ctypes.data, L.shape[0], int(distance), probs.ctypes.data, 1,
                                              int(seed), int(begin), int(end), d_prior, int(max_iter), 0, 1.0, 1.0, 20.0,
                                              int(flags), d_counters, stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_probs_device: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_osd_step(self):
        return max(1, min(_lib.MC_OSD_MAX_TRIALS, (8 << 30) // (self.m + 10 * self.n)))

    def close(self):
        self.lib.qbp_destroy(self.h)


def config(n, large):
    return relay.RelayConfig(relay.relay_gammas(n, LEGS, GAMMA0, INTERVAL, SEED), [ITERS] * LEGS, STOP, ALPHA, large=large)


def dense(H):
    return np.ascontiguousarray(H.toarray() if hasattr(H, "toarray") else H, dtype=np.uint8)


def row_a(torch, records, reps):
    H, _, probs = dem.phenomenological("[[72, 12, 6]]", 33, 0.02, 0.02)
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
    cfg = config(n, "force")
    dec.relay_configure(cfg)
    times, geometry, solved, outputs = {0: [], 1: []}, {}, {}, {}
    for rep in range(reps + 1):
        for mem in (0, 1):
            dec.set_option(_lib.OPT_RELAY_MEM, mem)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dec.relay_decode_device(d_syn.data_ptr(), d_prior.data_ptr(), records, d_hard.data_ptr(), d_conv.data_ptr(), 0, 0,
                                    0, 0, stream=stream)
            torch.cuda.synchronize(dev)
            if rep:
                times[mem].append(time.perf_counter() - t0)
            else:
                geometry[mem] = {k: dec.info(k) for k in ("threads", "grid", "lds_bytes")}
                solved[mem] = int(d_conv.sum().item())
                outputs[mem] = d_hard.cpu().numpy().copy()
    if not np.array_equal(outputs[0], outputs[1]) or solved[0] != solved[1]:
        raise SystemExit("row (a): the two builds disagree on the hard decisions")
    return {"row": "a", "matrix": list(H.shape), "p": 0.02, "records": records, "solved": solved[0],
            "lds": {"seconds": min(times[0]), "records_per_s": records / min(times[0]), **geometry[0]},
            "large": {"seconds": min(times[1]), "records_per_s": records / min(times[1]), **geometry[1]},
            "ratio": min(times[1]) / min(times[0])}


def timed_mc(torch, dec, L, distance, probs, d_prior, trials, flags):
    dev = torch.device("cuda", 0)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    step = dec.mc_osd_step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for a in range(0, trials, step):
        dec.mc_run_probs_device(L, distance, probs, d_prior.data_ptr(), a, min(a + step, trials), d_cnt.data_ptr(),
                                seed=SEED, max_iter=MAX_ITER, flags=flags, stream=stream)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, d_cnt.cpu().numpy()


def row_mc(torch, tag, H, L, probs, distance, trials, reps, baseline_lib):
    H = dense(H)
    L = np.ascontiguousarray(L, np.uint8)
    n = H.shape[1]
    dec = bp.decoder_for(H)
    dec.relay_configure(config(n, True))
    base = BaselineDecoder(baseline_lib, H) if baseline_lib else dec
    d_prior = torch.from_numpy(mc.dem_prior(probs)).to(torch.device("cuda", 0))
    runs = {"relay_large": (dec, _lib.FLAG_RELAY), "osd0": (base, _lib.FLAG_OSD0)}
    for d, fl in runs.values():                                                   # warm-up
        timed_mc(torch, d, L, distance, probs, d_prior, min(trials, 8192), fl)
    geometry = {k: dec.info(k) for k in ("threads", "grid", "lds_bytes")}
    best, cnt = {}, {}
    for _ in range(reps):
        for key, (d, fl) in runs.items():
            t, c = timed_mc(torch, d, L, distance, probs, d_prior, trials, fl)
            best[key] = min(best.get(key, t), t)
            cnt[key] = c
    row = {"row": tag, "matrix": list(H.shape), "trials": trials, "relay_launch": geometry}
    for key in runs:
        row[key] = {"seconds": best[key], "trials_per_s": trials / best[key], "ler": cnt[key][1] / cnt[key][0],
                    "unconverged_share": cnt[key][6] / cnt[key][0], "without_solution": int(cnt[key][10])}
    if base is not dec:
        base.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit for the OSD-0 pipelines")
    ap.add_argument("--trials", type=int, default=100_000)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench_dem import synthetic_dem

    result = {"max_iter": MAX_ITER, "relay": dict(legs=LEGS, iters=ITERS, stop_after=STOP, gamma0=GAMMA0, interval=INTERVAL,
              alpha=ALPHA), "baseline_lib": args.baseline_lib, "rows": []}
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
