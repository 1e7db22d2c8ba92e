#!/usr/bin/env python3
"""Timing of the exhaustive weight-w enumeration (qbp_mc_run_enum, qbp_enum_failures) against the fixed-weight sampler
on the same number of trials.

[[144,12,12]] w = 4 (17 178 876 patterns) and [[288,12,18]] w = 3 (3 939 936), BP(50) at the prior of p = 0.01,
device-resident, best of three after a warm-up, the timings taken alternately inside each repetition:
  t_enum      qbp_mc_run_enum_device over the whole class                                             (this build)
  t_weight    qbp_mc_run_weight_device on as many sampled trials      (--baseline-lib: the parent commit's library)
  t_failures  qbp_enum_failures_device over the whole class, what = 3, up to 2^22 hits kept          (this build)
without and with OSD-0.  Nobody set a threshold: the ratios are reported.  The kernels alone (mc_enum_weight_kernel,
enum_pack_kernel, enum_capture_kernel) come from a kernel trace taken in a run of its own:

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/etrace -o trace -- \\
        python3 tools/bench_enum.py --kernels-only
    python tools/bench_enum.py --baseline-lib /tmp/libqbp_parent.so --kernel-stats /tmp/etrace \\
        --out profiles/r31_enum.json
"""
import argparse
import csv
import ctypes as C
import glob
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qldpc_amd import _lib, bp, codes, mc  # noqa: E402

MAX_ITER = 50
SEED = 2026
PRIOR_P = 0.01
WORKLOADS = (("[[144, 12, 12]]", 4), ("[[288, 12, 18]]", 3))
KERNELS = ("mc_enum_weight_kernel", "enum_pack_kernel", "enum_capture_kernel")


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

    def mc_run_weight_device(self, L, distance, w, d_prior, begin, end, d_counters, flags, stream):
        rc = self.lib.qbp_mc_run_weight_device(self.h, L.ctypes.data, L.shape[0], int(distance), int(w), SEED, int(begin),
                                               int(end), d_prior, MAX_ITER, 0, 1.0, 1.0, 20.0, int(flags), d_counters,
                                               stream or None)
        if rc:
            raise RuntimeError(f"baseline qbp_mc_run_weight_device: {rc} {self.lib.qbp_last_error().decode()}")

    def close(self):
        self.lib.qbp_destroy(self.h)


def run_workload(code_name, w, osd, baseline_lib, reps, limit=None):
    import torch
    code = codes.load_code(code_name)
    total = math.comb(code.n, w) if limit is None else min(limit, math.comb(code.n, w))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = np.ascontiguousarray(code.Lx, np.uint8)
    dec = bp.decoder_for(code.Hx)
    base = BaselineDecoder(baseline_lib, code.Hx) if baseline_lib else None
    d_prior = torch.from_numpy(mc.prior_of(PRIOR_P, code.n)).to(dev)
    flags = _lib.FLAG_OSD0 if osd else 0
    step = dec.mc_osd_step() if osd else total
    d_ranks = torch.zeros(1 << 22, dtype=torch.int64, device=dev)
    d_kinds = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)

    def enum(n):
        tab = torch.zeros(12, dtype=torch.int64, device=dev)
        for a in range(0, n, step):
            dec.mc_run_enum_device(L, code.distance, w, d_prior.data_ptr(), a, min(a + step, n), tab.data_ptr(),
                                   max_iter=MAX_ITER, flags=flags, stream=stream)
        return tab

    def weight(n):
        tab = torch.zeros(12, dtype=torch.int64, device=dev)
        for a in range(0, n, step):
            base.mc_run_weight_device(L, code.distance, w, d_prior.data_ptr(), a, min(a + step, n), tab.data_ptr(), flags,
                                      stream)
        return tab

    def failures(n):
        tab = torch.zeros(13, dtype=torch.int64, device=dev)             # counters, then found
        dec.enum_failures_device(L, w, d_prior.data_ptr(), 0, n, 3, len(d_ranks), d_ranks.data_ptr(), d_kinds.data_ptr(),
                                 tab.data_ptr() + 96, tab.data_ptr(), max_iter=MAX_ITER, flags=flags, stream=stream)
        return tab

    def timed(fn, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tab = fn(n)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, tab.cpu().numpy()

    fns = [("enum", enum), ("failures", failures)] + ([("weight", weight)] if base else [])
    for n in (min(total, 20000), total):               # warm-up: every kernel of the timed window, buffers at full size
        for _, fn in fns:
            timed(fn, n)
    times = {name: [] for name, _ in fns}
    tabs = {}
    for _ in range(reps):
        for name, fn in fns:
            t, tabs[name] = timed(fn, total)
            times[name].append(t)
            if tabs[name][0] != total:
                raise SystemExit(f"{code_name} w={w} {name}: {tabs[name][0]} trials counted, {total} asked for")
    if base:
        base.close()
    e, f = tabs["enum"], tabs["failures"]
    if any(e[i] != f[i] for i in (0, 1, 6)):
        raise SystemExit(f"{code_name} w={w}: counters of enum {e.tolist()} and failures {f.tolist()} differ")
    row = dict(workload=f"{code_name} w={w}" + (" +OSD-0" if osd else ""), n=code.n, weight=w, patterns=total,
               prior_p=PRIOR_P, max_iter=MAX_ITER, osd=bool(osd), t_enum_s=min(times["enum"]),
               t_failures_s=min(times["failures"]), all_t_enum_s=times["enum"], all_t_failures_s=times["failures"],
               failures_over_enum=min(times["failures"]) / min(times["enum"]), enum_patterns_per_s=total / min(times["enum"]),
               logical_failures=int(e[1]), not_converged=int(e[6]), captured=int(f[12]),
               exact_f_w=int(e[1]) / total)
    if base:
        row.update(t_weight_s=min(times["weight"]), all_t_weight_s=times["weight"],
                   enum_over_weight=min(times["enum"]) / min(times["weight"]),
                   weight_trials_per_s=total / min(times["weight"]), weight_logical_errors=int(tabs["weight"][1]))
    print(json.dumps({k: v for k, v in row.items() if not k.startswith("all_")}), flush=True)
    return row


def kernels_only(reps):
    """The enumeration paths alone, BP only: what a kernel trace of the three kernels is taken from."""
    for code_name, w in WORKLOADS:
        run_workload(code_name, w, False, None, reps)
    print(json.dumps(dict(kernels_only=True, calls_per_workload=reps + 2)))


def kernel_stats(directory):
    """Rows of the enumeration kernels in the rocprofv3 kernel statistics under `directory`."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for k in KERNELS:
                    if k in r.get("Name", ""):
                        rows.append(dict(kernel=k, launches=int(r["Calls"]), total_kernel_s=float(r["TotalDurationNs"]) * 1e-9,
                                         mean_kernel_us=float(r["TotalDurationNs"]) * 1e-3 / max(int(r["Calls"]), 1),
                                         share_of_trace_percent=float(r.get("Percentage", "nan")),
                                         note="kernel time only: the buffer's memset is a runtime fill, not in this row"))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=None, help="at most this many patterns per class (a rehearsal)")
    ap.add_argument("--kernels-only", action="store_true", help="run the enumeration paths alone (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR",
                    help="fold the rows of the enumeration kernels of the kernel trace under DIR into the output")
    args = ap.parse_args()
    if args.kernels_only:
        kernels_only(args.reps)
        return
    if not args.baseline_lib:
        ap.error("--baseline-lib is required (the sampled side runs on the parent commit's library)")
    rows = [run_workload(name, w, osd, args.baseline_lib, args.reps, args.limit)
            for name, w in WORKLOADS for osd in (False, True)]
    kernels = kernel_stats(args.kernel_stats) if args.kernel_stats else []
    for r in kernels:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_enum.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_weight: qbp_mc_run_weight_device of the parent commit's library, as many trials",
                           rows=rows, kernels=kernels or "not measured"), f, indent=1)


if __name__ == "__main__":
    main()
