#!/usr/bin/env python3
"""Register / scratch / occupancy table of every kernel of libqbp.so, from the compiler's
kernel-resource-usage remarks (`make -C qldpc_amd/csrc resources` runs this)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qldpc_amd", "csrc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math".split()
UNITS = [("qbp_tu_fused.hip", []), ("qbp_tu_generic.hip", ["-DQBP_GENERIC_MEM=0"]),
         ("qbp_tu_generic.hip", ["-DQBP_GENERIC_MEM=1"]), ("qbp_tu_generic.hip", ["-DQBP_GENERIC_MEM=2"]),
         ("qbp_tu_stream.hip", []), ("qbp_tu_osd.hip", []),
         # Monte-Carlo with a sampler threshold per qubit (qbp_mc_run_probs): bp_fused_cols_kernel, bp_generic_cols_kernel
         ("qbp_tu_fused.hip", ["-DQBP_COLS_TU"])] + [("qbp_tu_generic.hip", ["-DQBP_COLS_TU", f"-DQBP_GENERIC_MEM={i}"])
                                                      for i in range(3)]
# Monte-Carlo over a ladder of iteration budgets (qbp_mc_run_budgets): bp_fused_budgets_kernel, bp_generic_budgets_kernel
UNITS += [("qbp_tu_fused.hip", ["-DQBP_BUDGETS_TU"])] + [("qbp_tu_generic.hip", ["-DQBP_BUDGETS_TU", f"-DQBP_GENERIC_MEM={i}"])
                                                         for i in range(3)]
# Monte-Carlo with residual-weight and iteration tables (qbp_mc_run_spectrum): bp_fused_spectrum_kernel,
# bp_generic_spectrum_kernel, and the OSD kernels that add to the table (osd*_spectrum_kernel)
UNITS += ([("qbp_tu_fused.hip", ["-DQBP_SPECTRUM_TU"])] +
          [("qbp_tu_generic.hip", ["-DQBP_SPECTRUM_TU", f"-DQBP_GENERIC_MEM={i}"]) for i in range(3)] +
          [("qbp_tu_osd.hip", ["-DQBP_SPECTRUM_TU"])])
# Recorded shots in, observable predictions out (qbp_decode_shots): bp_fused_shots_kernel, bp_generic_shots_kernel,
# and the OSD kernels that predict their records (osd*_shots_kernel)
UNITS += ([("qbp_tu_fused.hip", ["-DQBP_SHOTS_TU"])] +
          [("qbp_tu_generic.hip", ["-DQBP_SHOTS_TU", f"-DQBP_GENERIC_MEM={i}"]) for i in range(3)] +
          [("qbp_tu_osd.hip", ["-DQBP_SHOTS_TU"])])
# OSD in a column order the caller gives (qbp_osd_batch_ordered): the OSD kernels without their sort (osd*_ordered_kernel)
UNITS += [("qbp_tu_osd.hip", ["-DQBP_ORDERED_TU"])]
# Relay-BP (qbp_relay_decode_batch, QBP_FLAG_RELAY): bp_relay_kernel, batch and records builds
UNITS += [("qbp_tu_relay.hip", [])]
# Layered BP (QBP_FLAG_LAYERED): bp_layered_kernel<variant, mc, large>
UNITS += [("qbp_tu_layered.hip", [])]
# BP guided decimation (qbp_gd_decode_batch, QBP_FLAG_GD): bp_gd_kernel<variant, records, large>
UNITS += [("qbp_tu_gd.hip", [])]
# Sliding-window decoding (qbp_window_*): window_*_kernel, the glue between the windows of one call
UNITS += [("qbp_tu_window.hip", [])]
# Localized statistics decoding (qbp_lsd_batch, QBP_FLAG_LSD): lsd_kernel<records>, lsd_large_kernel<records>
UNITS += [("qbp_tu_lsd.hip", [])]
# BP with a prior per record (qbp_decode_batch_cond): bp_cond_kernel<variant>, and the glue kernels of qbp_css_*
UNITS += [("qbp_tu_cond.hip", [])]
# Monte-Carlo with posterior-LLR histograms per iteration budget (qbp_mc_run_llr_hist): bp_fused_llrhist_kernel,
# bp_generic_llrhist_kernel (last, so that the rows before them are the earlier tables')
UNITS += [("qbp_tu_fused.hip", ["-DQBP_LLRHIST_TU"])] + [("qbp_tu_generic.hip", ["-DQBP_LLRHIST_TU", f"-DQBP_GENERIC_MEM={i}"])
                                                         for i in range(3)]
# Fixed-point min-sum (qbp_quant_decode_batch, QBP_FLAG_QUANT): bp_quant_kernel<message type, mc> (after them, for the
# same reason)
UNITS += [("qbp_tu_quant.hip", [])]
# Distance upper bound (qbp_distance_search): dist_search_kernel<capture> (after them, for the same reason)
UNITS += [("qbp_tu_distance.hip", [])]
# Pauli-frame simulation (qbp_frame_*): frame_sim_kernel<sample> and frame_assemble_kernel (after them, for the same reason)
UNITS += [("qbp_tu_frame.hip", [])]


def demangle(sym):
    try:
        return subprocess.check_output(["c++filt", sym], text=True).strip()
    except Exception:
        return sym


rows = []
for src, extra in UNITS:
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + sys.argv[1:] +
                         ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", src],
                         cwd=CSRC, capture_output=True, text=True).stderr
    cur = None
    for ln in out.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = {"name": demangle(m.group(1))}
            rows.append(cur)
            continue
        for key, pat in (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
print(f"{'kernel':78s} {'SGPR':>5s} {'VGPR':>5s} {'scratch B/lane':>15s} {'waves/SIMD':>11s}")
for r in rows:
    name = re.sub(r"\(qbp::\w+(, qbp::\w+)?\)$|^void ", "", r["name"])
    print(f"{name[:78]:78s} {r.get('sgpr', 0):5d} {r.get('vgpr', 0):5d} {r.get('scratch', 0):15d} {r.get('occ', 0):11d}")
