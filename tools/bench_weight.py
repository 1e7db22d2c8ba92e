#!/usr/bin/env python3
"""Timing of the fixed-weight Monte-Carlo (qbp_mc_run_weight: sample a chunk, then the stored-errors pipeline) against
the Bernoulli loop at the error rate of the same mean weight.

[[288,12,18]], BP(50), device-resident, best of three after a warm-up, the two timings taken alternately inside each
repetition:
  t_weight     qbp_mc_run_weight_device at weight w                                                     (this build)
  t_bernoulli  qbp_mc_run_device at p = w / n, same prior       (--baseline-lib: the library of the parent commit)
for w = 3 and w = 14 (p = 0.0104 and 0.0486), without and with OSD-0.  Nobody set a threshold: t_weight / t_bernoulli
is reported.  The sampler kernel alone comes from a kernel trace taken in a run of its own:

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/wtrace/w3 -o trace -- \\
        python3 tools/bench_weight.py --sampler-only --weights 3            (and likewise w14, --weights 14)
    python tools/bench_weight.py --baseline-lib /tmp/libqbp_parent.so --kernel-stats /tmp/wtrace \\
        --out profiles/r11_weight.json
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qldpc_amd import _lib, bp, codes, mc  # noqa: E402

MAX_ITER = 50
SEED = 2026


class BaselineDecoder:
    """qbp_mc_run_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_device", "qbp_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        rc = self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device,
                                 C.byref(self.h))
        if rc:
            raise RuntimeError(f"baseline qbp_create: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_run_device(self, L, distance, p, d_prior, begin, end, d_counters, flags, stream):
        rc = self.lib.qbp_mc_run_device(self.h, L.ctypes.data, L.shape[0], int(distance), float(p), 1, SEED, int(begin),
                                        int(end), d_prior, MAX_ITER, 0, 1.0, 1.0, 20.0, int(flags), d_counters,
                                        stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def weight_run(dec, code, w, d_prior, trials, osd, dev, stream):
    import torch
    tab = torch.zeros(12, dtype=torch.int64, device=dev)
    step = dec.mc_osd_step() if osd else trials
    for a in range(0, trials, step):
        dec.mc_run_weight_device(code.Lx, code.distance, w, d_prior.data_ptr(), a, min(a + step, trials),
                                 tab.data_ptr(), seed=SEED, max_iter=MAX_ITER, flags=_lib.FLAG_OSD0 if osd else 0,
                                 stream=stream)
    return tab


def run_workload(code, w, trials, osd, baseline_lib, reps):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = np.ascontiguousarray(code.Lx, np.uint8)
    p = w / code.n
    dec = bp.decoder_for(code.Hx)
    base = BaselineDecoder(baseline_lib, code.Hx)
    d_prior = torch.from_numpy(mc.prior_of(p, code.n)).to(dev)
    flags = _lib.FLAG_OSD0 if osd else 0

    def weight():
        return weight_run(dec, code, w, d_prior, trials, osd, dev, stream)

    def bernoulli():
        tab = torch.zeros(12, dtype=torch.int64, device=dev)
        step = dec.mc_osd_step() if osd else trials
        for a in range(0, trials, step):
            base.mc_run_device(L, code.distance, p, d_prior.data_ptr(), a, min(a + step, trials), tab.data_ptr(), flags,
                               stream)
        return tab

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tab = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, tab.cpu().numpy()

    trials_full, trials = trials, min(trials, 20000)      # warm-up: every kernel of the timed window
    timed(weight), timed(bernoulli)
    trials = trials_full
    timed(weight), timed(bernoulli)                        # (buffers at their full size)
    t_w, t_b = [], []
    for _ in range(reps):
        t, got = timed(weight)
        t_w.append(t)
        t, ref = timed(bernoulli)
        t_b.append(t)
        if got[0] != trials or ref[0] != trials:
            raise SystemExit(f"w={w}: {got[0]} / {ref[0]} trials counted, {trials} asked for")
    base.close()
    row = dict(workload=f"[[288,12,18]] w={w} (p={p:.4f})" + (" +OSD-0" if osd else ""), weight=w, p=p, n=code.n,
               trials=trials, max_iter=MAX_ITER, osd=bool(osd), t_weight_s=min(t_w), t_bernoulli_s=min(t_b),
               all_t_weight_s=t_w, all_t_bernoulli_s=t_b, weight_over_bernoulli=min(t_w) / min(t_b),
               weight_trials_per_s=trials / min(t_w), bernoulli_trials_per_s=trials / min(t_b),
               weight_not_converged=int(got[6]), bernoulli_not_converged=int(ref[6]),
               weight_logical_errors=int(got[1]), bernoulli_logical_errors=int(ref[1]))
    print(json.dumps({k: v for k, v in row.items() if not k.startswith("all_")}), flush=True)
    return row


def sampler_only(code, weights, trials, reps):
    """The weight path alone, BP only: what a kernel trace of the sampler is taken from."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dec = bp.decoder_for(code.Hx)
    for w in weights:
        d_prior = torch.from_numpy(mc.prior_of(w / code.n, code.n)).to(dev)
        for _ in range(reps + 1):
            weight_run(dec, code, w, d_prior, trials, False, dev, stream)
            torch.cuda.synchronize(dev)
    print(json.dumps(dict(sampler_only=True, weights=weights, trials=trials, calls_per_weight=reps + 1)))


def kernel_stats(directory, trials_per_call):
    """Sampler rows of the rocprofv3 kernel statistics under `directory`/w<weight>/: kernel time per trial."""
    rows = []
    for sub in sorted(glob.glob(os.path.join(directory, "w*"))):
        for path in glob.glob(os.path.join(sub, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    if "mc_sample_weight_kernel" not in r.get("Name", ""):
                        continue
                    # one call samples trials_per_call trials, in as many launches as it has chunks
                    dflt = max(1, min(1 << 20, (1 << 28) // 288))
                    launches_per_call = -(-trials_per_call // dflt)
                    calls = int(r["Calls"]) / launches_per_call
                    total_s = float(r["TotalDurationNs"]) * 1e-9
                    rows.append(dict(weight=int(os.path.basename(sub)[1:]), kernel="mc_sample_weight_kernel",
                                     launches=int(r["Calls"]), total_kernel_s=total_s,
                                     kernel_s_per_call=total_s / calls, trials_per_call=trials_per_call,
                                     sampler_trials_per_s=trials_per_call * calls / total_s,
                                     note="kernel time only: the buffer's memset is a runtime fill, not in this row"))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trials", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--weights", type=int, nargs="+", default=[3, 14])
    ap.add_argument("--sampler-only", action="store_true", help="run the weight path alone (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR",
                    help="fold the sampler rows of the kernel traces under DIR/w<weight>/ into the output")
    args = ap.parse_args()
    code = codes.load_code("[[288, 12, 18]]")
    if args.sampler_only:
        sampler_only(code, args.weights, args.trials, args.reps)
        return
    if not args.baseline_lib:
        ap.error("--baseline-lib is required (the Bernoulli side runs on the parent commit's library)")
    rows = [run_workload(code, w, args.trials, osd, args.baseline_lib, args.reps)
            for w in args.weights for osd in (False, True)]
    sampler = kernel_stats(args.kernel_stats, args.trials) if args.kernel_stats else []
    for r in sampler:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_weight.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_bernoulli: qbp_mc_run_device of the parent commit's library at p = w / n",
                           rows=rows, sampler=sampler or "not measured"), f, indent=1)


if __name__ == "__main__":
    main()
