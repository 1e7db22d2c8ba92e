#!/usr/bin/env python3
"""Device-side time of order-w OSD on matrices beyond the one-wavefront kernel (QBP_FLAG_OSD_LARGE,
osd_order_blocked_kernel) -> profiles/r10_osd_order_large.json.

  (a) 864 x 2592 and 2592 x 7776 phenomenological matrices ([[144,12,12]] over 12 rounds, [[288,12,18]] over 18),
      BP(50) failures at p = q = 0.004 and 0.01: OSD-CS-7 and OSD-E-8 on this build, against OSD-0 (the blocked
      kernel) on the same records -- on this build and, with --parent-lib PATH, on another build of libqbp.so (the
      parent commit's) in a fresh child process with the same seeds.  Solutions/s, best of three launches.
  (b) [[288,12,18]] Hx: the new kernel forced with QBP_OPT_OSD_BIG = 1 against osd_order_kernel (CS-7), which with
      --parent-lib is also timed on the parent build.
  (c) mc.run_dem at 1e5 trials with OSD-0 and OSD-CS-7 on the matrices of (a): LER and trials/s.
One JSON line, also written to --out (default profiles/r10_osd_order_large.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", help="libqbp.so of the build to compare with")
ap.add_argument("--parent-child", action="store_true", help="(the child process of --parent-lib: no flag, no (c))")
ap.add_argument("--records", type=int, default=512)
ap.add_argument("--trials", type=int, default=100000,
                help="trials of (c); its CS-7 runs on 2592 x 7776 have not been timed: size the job's time limit, "
                     "or lower this")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_osd_order_large.json"))
args = ap.parse_args()

import torch  # noqa: E402
from qldpc_amd import _lib, bp, codes, dem, mc  # noqa: E402

dev = torch.device("cuda", 0)
MATRICES = (("864x2592", "[[144, 12, 12]]", 12), ("2592x7776", "[[288, 12, 18]]", 18))


def fresh(H):
    row_ptr, col_idx, m, n = bp.csr_from_H(H)
    return _lib.Decoder(row_ptr, col_idx, m, n, 0)


def failures(dec, H, probs, want, seed):
    """The first `want` records BP(50) does not converge on: (syn, llr, hard) host arrays."""
    rng = np.random.default_rng(seed)
    prior = mc.dem_prior(probs)
    keep, have = [], 0
    for _ in range(400):
        err = (rng.random((4096, H.shape[1])) < probs).astype(np.uint8)
        syn = np.asarray((H @ err.T) % 2, np.uint8).T.copy()
        hard, conv, _, llr = dec.decode(syn, prior, 50)
        f = np.flatnonzero(~conv)
        keep.append((syn[f], llr[f], hard[f]))
        have += len(f)
        if have >= want:
            break
    return tuple(np.concatenate(x)[:want] for x in zip(*keep))


def time_osd(dec, recs, method, order, large):
    syn, llr, hard = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in recs)
    sol = torch.empty_like(hard)
    st = torch.cuda.current_stream(dev)
    kw = {"large": True} if large else {}
    ms = []
    for rep in range(4):                                  # (the first launch warms up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        dec.osd_device(syn.data_ptr(), llr.data_ptr(), hard.data_ptr(), len(recs[0]), sol.data_ptr(), method=method,
                       order=order, stream=st.cuda_stream, **kw)
        b.record(st)
        torch.cuda.synchronize(dev)
        if rep:
            ms.append(a.elapsed_time(b))
    return {"records": len(recs[0]), "ms": ms, "solutions_per_s": len(recs[0]) / (min(ms) * 1e-3)}


out = {"tool": "bench_osd_order_large", "library": _lib.load().qbp_version().decode(), "large": {}, "forced_288": {}}
for tag, name, rounds in MATRICES:
    for p in (0.004, 0.01):
        H, L, probs = dem.phenomenological(name, rounds, p)
        dec = fresh(H)
        recs = failures(dec, H, probs, args.records, 7)
        row = {"failures": len(recs[0]), "osd0": time_osd(dec, recs, "cs", 0, False) if len(recs[0]) else None}
        if len(recs[0]) and not args.parent_child:
            row["cs7"] = time_osd(dec, recs, "cs", 7, True)
            row["e8"] = time_osd(dec, recs, "e", 8, True)
        out["large"][f"{tag}@{p}"] = row

code = codes.load_code("[[288, 12, 18]]")
dec = fresh(code.Hx)
rng = np.random.default_rng(3)
err = (rng.random((60000, code.n)) < 0.1).astype(np.uint8)
syn = (err @ code.Hx.T % 2).astype(np.uint8)
hard, conv, _, llr = dec.decode(syn, mc.prior_of(0.1, code.n), 50)
f = np.flatnonzero(~conv)[:8192]
recs = (syn[f], llr[f], hard[f])
out["forced_288"]["osd_order_kernel_cs7"] = time_osd(dec, recs, "cs", 7, False)
if not args.parent_child:
    forced = fresh(code.Hx)
    forced.set_option(_lib.OPT_OSD_BIG, 1)
    out["forced_288"]["osd_order_blocked_kernel_cs7"] = time_osd(forced, recs, "cs", 7, True)
    out["run_dem"] = {}
    for tag, name, rounds in MATRICES:
        for p in (0.004, 0.01):
            H, L, probs = dem.phenomenological(name, rounds, p)
            for label, kw in (("osd0", {}), ("cs7", {"osd_order": 7, "osd_large": True})):
                t0 = time.perf_counter()
                cnt = mc.run_dem(H, L, probs, args.trials, osd=True, **kw)
                dt = time.perf_counter() - t0
                out["run_dem"][f"{tag}@{p}/{label}"] = {"trials": int(cnt[0]), "logical_errors": int(cnt[1]),
                                                        "ler": float(cnt[1]) / max(int(cnt[0]), 1),
                                                        "not_converged": int(cnt[6]), "trials_per_s": int(cnt[0]) / dt}
    if args.parent_lib:
        env = dict(os.environ, QBP_LIB_PATH=os.path.abspath(args.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", "--records", str(args.records),
                            "--out", os.devnull], env=env, capture_output=True, text=True, check=True)
        out["parent"] = json.loads(r.stdout.strip().splitlines()[-1])

line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
