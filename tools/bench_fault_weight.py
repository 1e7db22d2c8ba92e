#!/usr/bin/env python3
"""Timing of the fixed-weight circuit-fault Monte-Carlo (qbp_mc_run_fault_weight: sample a chunk of fault sets into error
rows, then the stored-errors pipeline) and one circuit-level LER(p) curve from it.

[[72,12,6]] x 6 rounds, BP(50) + OSD-0, prior at p = 0.001 on every class, device-resident, best of three after a
warm-up, the two timings taken alternately inside each repetition:
  t_fault    mc.run_circuit_weights' device call, qbp_mc_run_fault_weight_device, at weight w              (this build)
  t_weight   qbp_mc_run_weight_device at the same w on the same H, prior and trial count
                                                            (--baseline-lib: the library of the parent commit)
for w = 4 and w = 64.  Nobody set a threshold: t_fault / t_weight is reported.  The curve: weights 0 .. --curve-top at
--curve-trials each, ler_from_weights at p = 1e-4 .. 2e-3, next to run_circuit's Bernoulli value at 2e-3.  The sampler
kernel alone comes from a kernel trace taken in a run of its own:

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/ftrace/w4 -o trace -- \\
        python3 tools/bench_fault_weight.py --sampler-only --weights 4        (and likewise w64, --weights 64)
    python tools/bench_fault_weight.py --baseline-lib /tmp/libqbp_parent.so --kernel-stats /tmp/ftrace \\
        --out profiles/r35_fault_weight.json
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

from qldpc_amd import _lib, bp, circuit, mc  # noqa: E402

CODE, ROUNDS = "[[72, 12, 6]]", 6
MAX_ITER = 50
SEED = 2026
PRIOR_P = 0.001
CURVE_PS = [1e-4, 2e-4, 5e-4, 1e-3, 2e-3]


class BaselineDecoder:
    """qbp_mc_run_weight_device of another build of the library (same C ABI) on the same matrix."""

    def __init__(self, path, H, device=0):
        self.lib = C.CDLL(path)
        for name in ("qbp_create", "qbp_destroy", "qbp_mc_run_weight_device", "qbp_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.row_ptr, self.col_idx, self.m, self.n = bp.csr_from_H(H)
        self.h = C.c_void_p()
        rc = self.lib.qbp_create(self.row_ptr.ctypes.data, self.col_idx.ctypes.data, self.m, self.n, device,
                                 C.byref(self.h))
        if rc:
            raise RuntimeError(f"baseline qbp_create: {rc} {self.lib.qbp_last_error().decode()}")

    def mc_run_weight_device(self, L, w, d_prior, begin, end, d_counters, flags, stream):
        rc = self.lib.qbp_mc_run_weight_device(self.h, L.ctypes.data, L.shape[0], 0, int(w), SEED, int(begin), int(end),
                                               d_prior, MAX_ITER, 0, 1.0, 1.0, 20.0, int(flags), d_counters,
                                               stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_weight_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def model():
    """(CircuitDem, (first_fault, K, N), prior, decoder with the fault table set) of the benchmark's circuit."""
    cir = circuit.memory_experiment(CODE, ROUNDS)
    cdem = circuit.circuit_dem(cir)
    table = circuit.fault_sites(cir)
    prior = mc.dem_prior(cdem.probs(circuit.rates_array(PRIOR_P, cir.n_classes)))
    dec = bp.decoder_for(cdem.H)
    dec.fault_table_set(table[0], table[1], cdem.fault_column)
    return cdem, table, prior, dec


def fault_run(dec, L, w, d_prior, trials, flags, dev, stream):
    import torch
    tab = torch.zeros(12, dtype=torch.int64, device=dev)
    step = dec.mc_step(flags, trials)
    for a in range(0, trials, step):
        dec.mc_run_fault_weight_device(L, 0, w, d_prior.data_ptr(), a, min(a + step, trials), tab.data_ptr(), seed=SEED,
                                       max_iter=MAX_ITER, flags=flags, stream=stream)
    return tab


def run_workload(cdem, prior, dec, w, trials, baseline_lib, reps):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = np.ascontiguousarray(cdem.L, np.uint8)
    base = BaselineDecoder(baseline_lib, cdem.H)
    d_prior = torch.from_numpy(prior).to(dev)
    flags = _lib.FLAG_OSD0

    def fault():
        return fault_run(dec, L, w, d_prior, trials, flags, dev, stream)

    def weight():
        tab = torch.zeros(12, dtype=torch.int64, device=dev)
        step = dec.mc_step(flags, trials)
        for a in range(0, trials, step):
            base.mc_run_weight_device(L, w, d_prior.data_ptr(), a, min(a + step, trials), tab.data_ptr(), flags, stream)
        return tab

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tab = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, tab.cpu().numpy()

    timed(fault), timed(weight)                            # warm-up: every kernel and buffer of the timed window
    t_f, t_w = [], []
    for _ in range(reps):
        t, got = timed(fault)
        t_f.append(t)
        t, ref = timed(weight)
        t_w.append(t)
        if got[0] != trials or ref[0] != trials:
            raise SystemExit(f"w={w}: {got[0]} / {ref[0]} trials counted, {trials} asked for")
    base.close()
    row = dict(workload=f"{CODE} x {ROUNDS} rounds, w={w}, BP({MAX_ITER})+OSD-0", weight=w, n=int(cdem.H.shape[1]),
               m=int(cdem.H.shape[0]), trials=trials, t_fault_s=min(t_f), t_weight_s=min(t_w), all_t_fault_s=t_f,
               all_t_weight_s=t_w, fault_over_weight=min(t_f) / min(t_w), fault_trials_per_s=trials / min(t_f),
               fault_not_converged=int(got[6]), weight_not_converged=int(ref[6]),
               note="the two decode different errors (w sites against w columns): the ratio compares whole calls, "
                    "the sampler's share is in `sampler`")
    print(json.dumps({k: v for k, v in row.items() if not k.startswith("all_")}), flush=True)
    return row


def curve(top, trials):
    t0 = time.perf_counter()
    weights = list(range(top + 1))
    table, N = mc.run_circuit_weights(CODE, ROUNDS, weights, trials, prior_p=PRIOR_P, seed=SEED, max_iter=MAX_ITER, osd=True)
    t_strat = time.perf_counter() - t0
    est = mc.ler_from_weights(table, weights, N, CURVE_PS)
    t0 = time.perf_counter()
    bern = mc.run_circuit(CODE, ROUNDS, [CURVE_PS[-1]], 1000000, seed=SEED, max_iter=MAX_ITER, osd=True)[0]
    out = dict(sites=N, weights=weights, trials_per_weight=trials, prior_p=PRIOR_P, seconds=t_strat,
               f_w=(table[:, 1] / np.maximum(table[:, 0], 1)).tolist(),
               points=[dict(p=p, ler=float(est["ler"][i]), ler_high=float(est["ler_high"][i]),
                            stderr=float(est["stderr"][i]), unsampled_mass=float(est["unsampled_mass"][i]))
                       for i, p in enumerate(CURVE_PS)],
               bernoulli=dict(p=CURVE_PS[-1], shots=int(bern[0]), ler=bern[1] / bern[0], seconds=time.perf_counter() - t0,
                              note="run_circuit at the last p; its prior is built for that p, the curve's for prior_p"))
    print(json.dumps(out), flush=True)
    return out


def sampler_only(weights, trials, reps):
    """The fault-weight path alone, BP only: what a kernel trace of the sampler is taken from."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cdem, _, prior, dec = model()
    d_prior = torch.from_numpy(prior).to(dev)
    L = np.ascontiguousarray(cdem.L, np.uint8)
    for w in weights:
        for _ in range(reps + 1):
            fault_run(dec, L, w, d_prior, trials, 0, dev, stream)
            torch.cuda.synchronize(dev)
    print(json.dumps(dict(sampler_only=True, weights=weights, trials=trials, calls_per_weight=reps + 1)))


def kernel_stats(directory, trials_per_call, calls):
    """Sampler rows of the rocprofv3 kernel statistics under `directory`/w<weight>/: kernel time per 1e6 trials."""
    rows = []
    for sub in sorted(glob.glob(os.path.join(directory, "w*"))):
        for path in glob.glob(os.path.join(sub, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    if "mc_sample_fault_weight_kernel" not in r.get("Name", ""):
                        continue
                    total_s = float(r["TotalDurationNs"]) * 1e-9
                    rows.append(dict(weight=int(os.path.basename(sub)[1:]), kernel="mc_sample_fault_weight_kernel",
                                     launches=int(r["Calls"]), total_kernel_s=total_s, trials_per_call=trials_per_call,
                                     ms_per_1e6_trials=total_s / (calls * trials_per_call) * 1e9,
                                     note="kernel time only: the buffer's memset is a runtime fill, not in this row"))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trials", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--weights", type=int, nargs="+", default=[4, 64])
    ap.add_argument("--curve-top", type=int, default=16)
    ap.add_argument("--curve-trials", type=int, default=200000)
    ap.add_argument("--no-curve", action="store_true")
    ap.add_argument("--sampler-only", action="store_true", help="run the fault-weight path alone (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR",
                    help="fold the sampler rows of the kernel traces under DIR/w<weight>/ into the output")
    args = ap.parse_args()
    if args.sampler_only:
        sampler_only(args.weights, args.trials, args.reps)
        return
    if not args.baseline_lib:
        ap.error("--baseline-lib is required (the fixed-weight side runs on the parent commit's library)")
    cdem, _, prior, dec = model()
    rows = [run_workload(cdem, prior, dec, w, args.trials, args.baseline_lib, args.reps) for w in args.weights]
    sampler = kernel_stats(args.kernel_stats, args.trials, args.reps + 1) if args.kernel_stats else []
    for r in sampler:
        print(json.dumps(r), flush=True)
    ler = None if args.no_curve else curve(args.curve_top, args.curve_trials)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_fault_weight.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_weight: qbp_mc_run_weight_device of the parent commit's library, same H, prior, trials",
                           rows=rows, sampler=sampler or "not measured", curve=ler or "not run"), f, indent=1)


if __name__ == "__main__":
    main()
