#!/usr/bin/env python3
"""The large build of localized statistics decoding (QBP_OPT_LSD_MEM, lsd_large_kernel) in numbers.  Device buffers,
best of three runs after a warm-up; nobody set a threshold: figures are reported.

1. option 1 against the parent commit's lsd_kernel (--baseline-lib) on 576 x 1728, the largest phenomenological matrix
   of [[72,12,6]] both take: qbp_lsd_batch_device on 65 536 BP(50) failures at p = q = 0.01, g = 1 and g = 0;
2. BP(50) + LSD (large, g = 1; qbp_mc_run_probs_device | QBP_FLAG_LSD) against BP(50) + OSD-0 of the parent commit's
   library on 864 x 2592 and 2592 x 7776 at p = q = 0.004 and on the synthetic 1008 x 8991 model of tools/bench_dem.py,
   1e5 trials: trials/s, LER, the share of unconverged trials, the mean of stats[1] over the LSD records and the count
   of valid = 0;
3. this build's lsd_kernel (option 0) against the parent's on the records of (1), with the parent's spread over its
   three runs: it did not move.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_lsd_large.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r27_lsd_large.json
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

from qldpc_amd import _lib, bp, dem, mc  # noqa: E402

MAX_ITER, SEED = 50, 2027


class Baseline:
    """The entries this tool times, of another build of the library (same C ABI), on the same matrix."""
    NAMES = ("qbp_create", "qbp_destroy", "qbp_last_error", "qbp_lsd_configure", "qbp_lsd_batch_device",
             "qbp_mc_run_probs_device")

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in self.NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        self.check(self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device,
                                       C.byref(self.h)), "qbp_create")

    def check(self, rc, what):
        if rc:
            raise RuntimeError(f"baseline {what}: {rc} {self.lib.qbp_last_error().decode()}")

    def lsd_configure(self, g, large=False):
        self.check(self.lib.qbp_lsd_configure(self.h, int(g)), "qbp_lsd_configure")

    def info(self, what):
        return {"threads": 64}[what]            # (the parent has lsd_kernel alone)

    def lsd_device(self, d_syn, d_llr, d_hard, B, d_sol, d_stats=0, stream=0):
        self.check(self.lib.qbp_lsd_batch_device(self.h, d_syn, d_llr, d_hard, int(B), d_sol, d_stats or None,
                                                 stream or None), "qbp_lsd_batch_device")

    def mc_run_probs_device(self, L, distance, probs, d_prior, begin, end, d_counters, seed=0, max_iter=50, flags=0,
                            stream=0):
        L = np.ascontiguousarray(L, np.uint8)
        probs = np.ascontiguousarray(probs, np.float64)
        self.check(self.lib.qbp_mc_run_probs_device(self.h, L.ctypes.data, L.shape[0], int(distance), probs.ctypes.data, 1,
                                                    int(seed), int(begin), int(end), d_prior, int(max_iter), 0, 1.0, 1.0,
                                                    20.0, int(flags), d_counters, stream or None),
                   "qbp_mc_run_probs_device")

    def close(self):
        self.lib.qbp_destroy(self.h)


def dense(H):
    return np.ascontiguousarray(H.toarray() if hasattr(H, "toarray") else H, dtype=np.uint8)


def bp_failures(torch, dec, H, probs, prior, records):
    """`records` BP(50) failures of errors drawn with `probs` -> device tensors (syn, llr, hard)."""
    rng = np.random.default_rng(SEED)
    out = [[], [], []]
    while sum(len(s) for s in out[0]) < records:
        err = (rng.random((1 << 15, H.shape[1])) < probs).astype(np.uint8)
        syn = (err.astype(np.int32) @ H.T.astype(np.int32) % 2).astype(np.uint8)
        hard, conv, _, llr = dec.decode(syn, prior, MAX_ITER)
        for dst, a in zip(out, (syn, llr, hard)):
            dst.append(a[~conv])
    return tuple(torch.from_numpy(np.ascontiguousarray(np.concatenate(a)[:records])).cuda() for a in out)


def timed_batch(torch, d, rec, g, reps):
    """Seconds of every timed run of one qbp_lsd_batch_device over the records (after a warm-up), and the stats."""
    d_syn, d_llr, d_hard = rec
    B = len(d_syn)
    d_sol = torch.zeros_like(d_hard)
    d_stats = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.lsd_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), B, d_sol.data_ptr(), d_stats.data_ptr(),
                     stream=stream)
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return times, d_stats.cpu().numpy(), d_sol.cpu().numpy()


def part_1_and_3(torch, baseline_lib, records, reps):
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 16, 0.01, 0.01)
    H = dense(H)
    prior = mc.dem_prior(probs)
    dec = bp.decoder_for(H)
    rec = bp_failures(torch, dec, H, probs, prior, records)
    base = Baseline(baseline_lib, H) if baseline_lib else None
    out = {"matrix": list(H.shape), "records": records}
    for g in (1, 0):
        row = {}
        # (Decoder.lsd_configure writes QBP_OPT_LSD_MEM from its `large` on every call: the build is chosen there)
        runs = {"large": (dec, "force", 256), "lds": (dec, False, 64)}
        if base:
            runs["parent_lds"] = (base, False, 64)
        sols = {}
        for key, (d, large, threads) in runs.items():
            d.lsd_configure(g, large=large)
            times, st, sols[key] = timed_batch(torch, d, rec, g, reps)
            if d.info("threads") != threads:
                raise RuntimeError(f"{key}: the launch had {d.info('threads')} threads, not the {threads} of its kernel")
            row[key] = {"threads": threads, "seconds": times, "best": min(times), "records_per_s": records / min(times),
                        "spread": (max(times) - min(times)) / min(times), "mean_active_variables": float(st[:, 1].mean()),
                        "valid_fraction": float(st[:, 3].mean())}
        row["same_bits"] = all(np.array_equal(s, sols["large"]) for s in sols.values())
        out[f"g{g}"] = row
        print(json.dumps({f"g{g}": row}))
    dec.lsd_configure(1, large=False)
    if base:
        base.close()
    return out


def timed_mc(torch, d, L, probs, prior, trials, flags):
    d_prior = torch.from_numpy(prior).cuda()
    d_cnt = torch.zeros(12, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    step = _lib.MC_OSD_MAX_TRIALS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in range(0, trials, step):
        d.mc_run_probs_device(L, 0, probs, d_prior.data_ptr(), a, min(a + step, trials), d_cnt.data_ptr(), seed=SEED,
                              max_iter=MAX_ITER, flags=flags, stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, d_cnt.cpu().numpy()


def part_2(torch, baseline_lib, trials, reps):
    import bench_dem
    models = [("864x2592", dem.phenomenological("[[144, 12, 12]]", 12, 0.004, 0.004)),
              ("2592x7776", dem.phenomenological("[[288, 12, 18]]", 18, 0.004, 0.004)),
              ("1008x8991", bench_dem.synthetic_dem())]
    rows = []
    for name, (H, L, probs) in models:
        H, L = dense(H), np.ascontiguousarray(L, np.uint8)
        prior = mc.dem_prior(probs)
        dec = bp.decoder_for(H)
        dec.lsd_configure(1, large=True)
        base = Baseline(baseline_lib, H) if baseline_lib else dec
        runs = {"lsd_large_g1": (dec, _lib.FLAG_LSD), "osd0": (base, _lib.FLAG_OSD0)}
        row = {"matrix": name}
        for key, (d, fl) in runs.items():
            timed_mc(torch, d, L, probs, prior, min(trials, 8192), fl)              # warm-up
            best, cnt = None, None
            for _ in range(reps):
                t, cnt = timed_mc(torch, d, L, probs, prior, trials, fl)
                best = t if best is None else min(best, t)
            row[key] = {"seconds": best, "trials_per_s": trials / best, "ler": cnt[1] / cnt[0],
                        "not_converged_share": cnt[6] / cnt[0], "valid0": int(cnt[10])}
        # the clusters: stats of the batch kernel on up to 4096 of the BP failures
        rec = bp_failures(torch, dec, H, probs, prior, 4096)
        _, st, _ = timed_batch(torch, dec, rec, 1, 1)
        row["lsd_large_g1"]["threads"] = dec.info("threads")            # (256: lsd_large_kernel; 64: lsd_kernel)
        row["lsd_large_g1"]["mean_active_variables"] = float(st[:, 1].mean())
        row["lsd_large_g1"]["mean_rounds"] = float(st[:, 0].mean())
        if base is not dec:
            base.close()
        print(json.dumps(row))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so of the parent commit (lsd_kernel and OSD-0)")
    ap.add_argument("--trials", type=int, default=100_000)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    result = {"max_iter": MAX_ITER, "baseline_lib": args.baseline_lib, "trials": args.trials,
              "batch_576x1728": part_1_and_3(torch, args.baseline_lib, args.records, args.reps),
              "monte_carlo": part_2(torch, args.baseline_lib, args.trials, args.reps)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
