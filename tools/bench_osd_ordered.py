#!/usr/bin/env python3
"""Device-side time of OSD-0 with and without a caller-supplied column order (qbp_osd_batch_ordered_device).

  (a) qbp_osd_batch_device, unordered -- on this build and, with --parent-lib PATH, on another build of libqbp.so
      (the parent commit's) in a fresh child process on the same inputs (same seeds);
  (b) qbp_osd_batch_ordered_device with the (|llr|, column) sort as the order -- the same solutions (checked), without
      the kernel's sort but with 4 n more bytes read per record.

Inputs: 65 536 BP(50) failures at p = 0.1 of [[144,12,12]] and [[288,12,18]] (one-wavefront kernel), and BP(12)
failures at p = 0.03 of the 1 728 x 5 184 space-time matrix (blocked kernel).  Device buffers, three repeats each:
all three are reported, `ms` is the best, `spread` the range of the three over the best.  One JSON line."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", help="libqbp.so of the build to compare (a) with")
ap.add_argument("--unordered-only", action="store_true", help="(the child process of --parent-lib)")
ap.add_argument("--out", help="also write the JSON here")
args = ap.parse_args()

import torch  # noqa: E402
from qldpc_amd import _lib, bp, codes  # noqa: E402

if args.unordered_only:                      # a build from before the ordered entry points
    for name in ("qbp_osd_batch_ordered", "qbp_osd_batch_ordered_device"):
        _lib.SIGNATURES.pop(name, None)

dev = torch.device("cuda", 0)


def big_matrix():
    from scipy.sparse import block_diag, csr_matrix
    H144 = codes.load_code("[[144, 12, 12]]").Hx
    mm, T = H144.shape[0], 12
    st = np.hstack([np.kron(np.eye(T, dtype=np.int64), H144),
                    (np.eye(mm * T, dtype=np.int64) + np.eye(mm * T, k=-mm, dtype=np.int64)) % 2])
    return block_diag([csr_matrix(st), csr_matrix(st)]).tocsr()


def failures(H, p, max_iter, want, chunk, seed):
    """(decoder, syn, llr, hard) on the device: the first `want` records BP(max_iter) does not converge on."""
    from scipy.sparse import issparse
    dense = np.asarray(H.todense()) if issparse(H) else np.asarray(H)
    m, n = dense.shape
    dec = bp.decoder_for(H)
    Ht = torch.from_numpy(dense.T.astype(np.float32)).to(dev)
    prior = torch.full((n,), float(np.log((1 - p) / p)), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    st = torch.cuda.current_stream(dev)
    keep, have = [], 0
    for _ in range(64):
        err = torch.rand((chunk, n), generator=g, device=dev) < p
        syn = (err.float() @ Ht).remainder_(2).to(torch.uint8)
        hard = torch.empty((chunk, n), dtype=torch.uint8, device=dev)
        conv = torch.empty((chunk,), dtype=torch.uint8, device=dev)
        iters = torch.empty((chunk,), dtype=torch.int32, device=dev)
        llr = torch.empty((chunk, n), dtype=torch.float64, device=dev)
        dec.decode_device(syn.data_ptr(), prior.data_ptr(), chunk, max_iter, 0, 1.0, 1.0, 20.0, 0, hard.data_ptr(),
                          conv.data_ptr(), iters.data_ptr(), llr.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        f = torch.nonzero(conv == 0).flatten()
        keep.append((syn[f], llr[f], hard[f]))
        have += len(f)
        if have >= want:
            break
    syn, llr, hard = (torch.cat(x)[:want].contiguous() for x in zip(*keep))
    return dec, syn, llr, hard, Ht


def sort_order(llr):
    """The device's own rule: ascending (bit pattern of |llr|, column) -- a stable sort of the keys (no NaN here)."""
    key = llr.abs().view(torch.int64)
    return torch.argsort(key, dim=1, stable=True).to(torch.int32).contiguous()


def timed(run):
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(min(ms), 3), "repeats_ms": [round(x, 3) for x in ms],
            "spread": round((max(ms) - min(ms)) / min(ms), 4)}


CASES = (("[[144, 12, 12]]", lambda: codes.load_code("[[144, 12, 12]]").Hx, 0.1, 50, 65536, 98304),
         ("[[288, 12, 18]]", lambda: codes.load_code("[[288, 12, 18]]").Hx, 0.1, 50, 65536, 98304),
         ("space-time 1728 x 5184", big_matrix, 0.03, 12, 256, 512))
out = {}
for name, make, p, max_iter, want, chunk in CASES:
    dec, syn, llr, hard, Ht = failures(make(), p, max_iter, want, chunk, seed=2)
    B = len(syn)
    sol = torch.empty_like(hard)
    st = torch.cuda.current_stream(dev)
    row = {"records": B}
    row["unordered"] = timed(lambda: dec.osd_device(syn.data_ptr(), llr.data_ptr(), hard.data_ptr(), B,
                                                    sol.data_ptr(), order=0, stream=st.cuda_stream))
    row["checksum"] = int(sol.to(torch.int64).sum().item())
    row["all_solutions_match_syndrome"] = bool(((sol.float() @ Ht).remainder_(2).to(torch.uint8) == syn).all())
    if not args.unordered_only:
        order = sort_order(llr)
        sol2 = torch.empty_like(hard)
        row["ordered"] = timed(lambda: dec.osd_device(syn.data_ptr(), llr.data_ptr(), hard.data_ptr(), B,
                                                      sol2.data_ptr(), order=0, stream=st.cuda_stream,
                                                      d_order=order.data_ptr()))
        row["ordered_equals_unordered"] = bool((sol2 == sol).all())
        row["ordered_over_unordered"] = round(row["ordered"]["ms"] / row["unordered"]["ms"], 4)
    out[name] = row

if args.parent_lib and not args.unordered_only:
    env = dict(os.environ, QBP_LIB_PATH=os.path.abspath(args.parent_lib))
    line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--unordered-only"], env=env,
                                   text=True).strip().splitlines()[-1]
    parent = json.loads(line)
    for name, row in out.items():
        pr = parent[name]
        row["parent_unordered"] = pr["unordered"]
        row["same_inputs_and_solutions_as_parent"] = pr["checksum"] == row["checksum"] and pr["records"] == row["records"]
        row["unordered_over_parent"] = round(row["unordered"]["ms"] / pr["unordered"]["ms"], 4)
        # (a) holds when this build's best lies within the parent's own run-to-run range of its best
        row["within_parent_spread"] = row["unordered"]["ms"] <= max(pr["unordered"]["repeats_ms"])

text = json.dumps(out)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
