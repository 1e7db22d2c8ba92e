#!/usr/bin/env python3
"""Timing of recorded-shot decoding (qbp_decode_shots) against the two things it sits between.

Per workload, device-resident inputs, the same shots, best of three after a warm-up, the timings taken alternately
inside each repetition:
  t_shots    qbp_decode_shots_device: bit-packed detection events in, predictions + converged + counters out (this build)
  t_compose  the composition that was the only way before: qbp_decode_batch_device (hard, converged, iters, llr to HBM),
             qbp_osd_batch_device on ALL rows (with OSD), the L product in torch         (--baseline-lib: parent commit)
  t_mc       qbp_mc_run_probs_device at the same rates: errors sampled on chip, nothing read, counters only  (parent)
The predictions of t_shots and t_compose must be identical.  Nobody set a threshold: the ratios are reported; the
condition is t_shots <= t_compose on every workload.  Calls are split by the libraries' OSD step where OSD keeps records.

    make -C qldpc_amd/csrc OBJ=/tmp/obj_parent OUT=/tmp/libqbp_parent.so      (in a checkout of the parent commit)
    python tools/bench_shots.py --baseline-lib /tmp/libqbp_parent.so --out profiles/r08_shots.json
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

from bench_budgets import BaselineDecoder  # noqa: E402
from qldpc_amd import _lib, bp, codes, dem, mc, shots  # noqa: E402

MAX_ITER = 50


class Baseline(BaselineDecoder):
    """... plus the decode and OSD entry points of that build."""

    def __init__(self, path, H):
        super().__init__(path, H)
        for name in ("qbp_decode_batch_device", "qbp_osd_batch_device"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]

    def check(self, rc, what):
        if rc:
            raise RuntimeError(f"baseline {what}: {rc} {self.lib.qbp_last_error().decode()}")

    def decode(self, d_syn, d_prior, B, d_hard, d_conv, d_iters, d_llr, stream):
        self.check(self.lib.qbp_decode_batch_device(self.h, d_syn, d_prior, B, MAX_ITER, 0, 1.0, 1.0, 20.0, 0, d_hard,
                                                    d_conv, d_iters, d_llr, stream or None), "qbp_decode_batch_device")

    def osd(self, d_syn, d_llr, d_hard, B, d_sol, stream):
        self.check(self.lib.qbp_osd_batch_device(self.h, 0, d_syn, d_llr, d_hard, B, d_sol, stream or None),
                   "qbp_osd_batch_device")


def run_workload(name, H, L, probs, prior, T, osd, baseline_lib, reps):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = np.ascontiguousarray(L, np.uint8)
    probs = np.ascontiguousarray(probs, np.float64)
    m, n = (int(x) for x in H.shape)
    k = L.shape[0]
    dec = bp.decoder_for(H)
    base = Baseline(baseline_lib, H)
    d_prior = torch.from_numpy(np.ascontiguousarray(prior, np.float64)).to(dev)
    flags = _lib.FLAG_OSD0 if osd else 0
    seed = 2026
    # the shots: the sampler's errors for the same seed and range as t_mc, H e and L e formed on the device
    Ht = torch.from_numpy(np.asarray(H.toarray() if hasattr(H, "toarray") else H, np.float32).T.copy()).to(dev)
    Lt = torch.from_numpy(L.astype(np.float32).T.copy()).to(dev)
    weights = torch.from_numpy((1 << np.arange(k, dtype=np.uint64)).view(np.int64)).to(dev)
    d_syn = torch.empty((T, m), dtype=torch.uint8, device=dev)
    d_act = torch.empty(T, dtype=torch.int64, device=dev)
    for a in range(0, T, 20000):
        e = torch.from_numpy(dec.mc_sample_errors_probs(probs, a, min(20000, T - a), seed=seed)).to(dev).float()
        d_syn[a:a + len(e)] = (e @ Ht).remainder(2).to(torch.uint8)
        d_act[a:a + len(e)] = ((e @ Lt).remainder(2).to(torch.int64) * weights).sum(dim=1)
    d_det = torch.from_numpy(shots.pack_bits(d_syn.cpu().numpy())).to(dev)
    rb = (m + 7) // 8
    d_hard = torch.empty((T, n), dtype=torch.uint8, device=dev)
    d_sol = torch.empty((T, n), dtype=torch.uint8, device=dev) if osd else None
    d_llr = torch.empty((T, n), dtype=torch.float64, device=dev)
    d_conv = torch.empty(T, dtype=torch.uint8, device=dev)
    d_iters = torch.empty(T, dtype=torch.int32, device=dev)

    def run_shots():
        cnt = torch.zeros(12, dtype=torch.int64, device=dev)
        pred = torch.empty(T, dtype=torch.int64, device=dev)
        conv = torch.empty(T, dtype=torch.uint8, device=dev)
        step = dec.mc_osd_step() if osd else T
        for a in range(0, T, step):
            dec.decode_shots_device(L, d_det.data_ptr() + a * rb, d_act.data_ptr() + 8 * a, min(step, T - a),
                                    d_prior.data_ptr(), pred.data_ptr() + 8 * a, conv.data_ptr() + a, cnt.data_ptr(),
                                    max_iter=MAX_ITER, flags=flags, stream=stream)
        return pred, cnt

    def run_compose():
        base.decode(d_syn.data_ptr(), d_prior.data_ptr(), T, d_hard.data_ptr(), d_conv.data_ptr(), d_iters.data_ptr(),
                    d_llr.data_ptr(), stream)
        x = d_hard
        if osd:
            base.osd(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), T, d_sol.data_ptr(), stream)
            x = torch.where(d_conv.bool()[:, None], d_hard, d_sol)
        pred = torch.empty(T, dtype=torch.int64, device=dev)
        for a in range(0, T, 100000):            # (float32 is exact here: row sums stay far below 2^24)
            pred[a:a + 100000] = ((x[a:a + 100000].float() @ Lt).remainder(2).to(torch.int64) * weights).sum(dim=1)
        return pred, None

    def run_mc():
        cnt = torch.zeros(12, dtype=torch.int64, device=dev)
        step = base.mc_osd_step() if osd else T
        for a in range(0, T, step):
            base.mc_run_probs_device(L, 0, probs, d_prior.data_ptr(), a, min(a + step, T), cnt.data_ptr(), seed,
                                     MAX_ITER, flags, stream)
        return None, cnt

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pred, cnt = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, pred, cnt

    for fn in (run_shots, run_compose, run_mc):             # warm-up: every kernel and buffer of the timed window
        timed(fn)
    ts = {"shots": [], "compose": [], "mc": []}
    for _ in range(reps):
        t, pred, cnt = timed(run_shots)
        ts["shots"].append(t)
        t, want, _ = timed(run_compose)
        ts["compose"].append(t)
        t, _, cnt_mc = timed(run_mc)
        ts["mc"].append(t)
        if not torch.equal(pred, want):
            raise SystemExit(f"{name}: predictions of decode_shots differ from the composition's")
        cnt, cnt_mc = cnt.cpu().numpy(), cnt_mc.cpu().numpy()
        if [cnt[i] for i in (0, 1, 6, 7, 8, 10)] != [cnt_mc[i] for i in (0, 1, 6, 7, 8, 10)]:
            raise SystemExit(f"{name}: counters differ from qbp_mc_run_probs on the same errors\n{cnt}\n{cnt_mc}")
    base.close()
    best = {key: min(v) for key, v in ts.items()}
    row = dict(workload=name, m=m, n=n, k=int(k), shots=T, max_iter=MAX_ITER, osd=bool(osd), t_shots_s=best["shots"],
               t_compose_s=best["compose"], t_mc_s=best["mc"], all_s=ts, compose_over_shots=best["compose"] / best["shots"],
               shots_over_mc=best["shots"] / best["mc"], shots_per_s=T / best["shots"], predictions_identical=True,
               not_converged=int(cnt[6]), wrong=int(cnt[1]), kernel=dec.info("last_kernel"))
    print(json.dumps({key: v for key, v in row.items() if key != "all_s"}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", required=True, help="libqbp.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shots", type=int, default=1000000, help="[[288,12,18]] workloads (the DEM ones run a tenth)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring of the workload names to run")
    args = ap.parse_args()
    code = codes.load_code("[[288, 12, 18]]")
    work = []
    for p in (0.01, 0.05):
        for osd in (False, True):
            work.append((f"[[288,12,18]] p={p}" + (" +OSD-0" if osd else ""), code.Hx, code.Lx, np.full(code.n, p),
                         mc.prior_of(p, code.n), args.shots, osd))
    for label, cname, rounds in (("864x2592", "[[144, 12, 12]]", 12), ("2592x7776", "[[288, 12, 18]]", 18)):
        H, L, probs = dem.phenomenological(cname, rounds, 0.004, 0.004)
        assert f"{H.shape[0]}x{H.shape[1]}" == label, H.shape
        for osd in (False, True):
            work.append((f"phenomenological {label} p=q=0.004" + (" +OSD-0" if osd else ""), H, L, probs,
                         mc.dem_prior(probs), max(args.shots // 10, 1), osd))
    rows = [run_workload(*w, args.baseline_lib, args.reps) for w in work if args.only is None or args.only in w[0]]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_shots.py", device="MI355X (gfx950)", reps=args.reps,
                           timing="host clock around enqueue + device synchronise, best of reps, alternating",
                           baseline="t_compose and t_mc: the parent commit's library", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
