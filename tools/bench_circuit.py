#!/usr/bin/env python3
"""Timings of the circuit-level path on one GPU, best of three (no threshold is set: the figures are written down).

  python tools/bench_circuit.py [--cases 72:6 144:12 288:18] [--shots 1000000] [--oracle] [--out profiles/r34_circuit.json]

Per case: circuit_dem end to end and the propagation of every fault alone (qbp_frame_faults_device into device
buffers); the sampler's shots/s alone at p = 0.001 and 0.01; mc.run_circuit against mc.run_dem on the same matrix,
BP(50) + OSD-0; with --baseline-lib run_dem is timed once more in a child process that loads that library (a build of the
parent commit) through QBP_LIB_PATH.  --oracle also times tests/circuit_oracle.py on the same host (the baseline of the enumeration)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return min(out)


def dem_child(path, shots):
    """--dem-child: run_dem on the model stored in ``path`` with whatever library QBP_LIB_PATH names; one JSON line."""
    from qldpc_amd import _lib, bp, mc
    from scipy.sparse import csr_matrix
    with np.load(path) as z:
        H, L, probs = csr_matrix(z["H"]), z["L"], z["probs"]
    mc.run_dem(H, L, probs, 1000, osd=True, device=bp.DEVICE)
    out = {}
    t = best(lambda: out.update(d=mc.run_dem(H, L, probs, shots, osd=True, seed=1, device=bp.DEVICE)))
    print(json.dumps(dict(lib=_lib.LIB_PATH, run_dem_s=t, ler=float(out["d"][1] / shots))))


def main():
    if "--dem-child" in sys.argv:
        i = sys.argv.index("--dem-child")
        return dem_child(sys.argv[i + 1], int(sys.argv[i + 2]))
    import torch

    from qldpc_amd import bp, circuit, codes, mc
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["72:6", "144:12", "288:18"])
    ap.add_argument("--shots", type=int, default=1000000)
    ap.add_argument("--mc-cases", nargs="*", default=["72:6"])
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--baseline-lib", default=None, help="libqbp.so built from the parent commit: run_dem is timed on it too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", bp.DEVICE)
    rows = []
    for case in args.cases:
        name, rounds = case.split(":")
        code, rounds = codes.load_code(name), int(rounds)
        cir = circuit.memory_experiment(code, rounds)
        sim = cir.simulator(bp.DEVICE)
        F, m = cir.n_faults, len(cir.detectors)
        row = dict(code=code.name, rounds=rounds, qubits=cir.nq, cnots=cir.count("CX"), sites=cir.n_sites, faults=F,
                   records=cir.n_records, detectors=m)
        d_det = torch.zeros((F, (m + 7) // 8), dtype=torch.uint8, device=dev)
        d_obs = torch.zeros(F, dtype=torch.int64, device=dev)

        def propagate():
            sim.faults_device(0, F, d_det.data_ptr(), d_obs.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        propagate()
        row["faults_kernels_s"] = best(propagate)
        row["circuit_dem_s"] = best(lambda: circuit.circuit_dem(cir, device=bp.DEVICE))
        d = circuit.circuit_dem(cir, device=bp.DEVICE)
        row["dem_shape"] = list(d.H.shape)
        row["workspace_bytes"], row["chunks_faults"] = sim.info("workspace_bytes"), sim.info("chunks")
        if args.oracle:
            import circuit_oracle as co
            row["oracle_faults_s"] = best(lambda: co.faults(cir), reps=1)
        T = args.shots
        s_det = torch.zeros((T, (m + 7) // 8), dtype=torch.uint8, device=dev)
        s_obs = torch.zeros(T, dtype=torch.int64, device=dev)
        for p in (0.001, 0.01):
            r = circuit.rates_array(p, cir.n_classes)

            def sample():
                sim.sample_device(r, T, s_det.data_ptr(), s_obs.data_ptr(), seed=1,
                                  stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
            sample()
            row[f"sampler_shots_per_s_p{p}"] = T / best(sample)
        del s_det, s_obs, d_det, d_obs
        if case in args.mc_cases:
            p = 0.002
            mc.run_circuit(code, rounds, [p], 1000, osd=True, device=bp.DEVICE)
            mc.run_dem(d.H, d.L, d.probs(p), 1000, osd=True, device=bp.DEVICE)
            out = {}
            row["run_circuit_s"] = best(lambda: out.update(c=mc.run_circuit(code, rounds, [p], T, osd=True, seed=1,
                                                                            device=bp.DEVICE)[0]))
            row["run_dem_s"] = best(lambda: out.update(d=mc.run_dem(d.H, d.L, d.probs(p), T, osd=True, seed=1,
                                                                    device=bp.DEVICE)))
            row.update(mc_p=p, mc_shots=T, ler_run_circuit=float(out["c"][1] / T), ler_run_dem=float(out["d"][1] / T),
                       ratio_run_circuit_over_run_dem=row["run_circuit_s"] / row["run_dem_s"])
            if args.baseline_lib:
                import subprocess
                import tempfile
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "dem.npz")
                    np.savez(path, H=d.H.toarray(), L=d.L, probs=d.probs(p))
                    env = dict(os.environ, QBP_LIB_PATH=os.path.abspath(args.baseline_lib))
                    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--dem-child", path, str(T)], env=env,
                                           capture_output=True, text=True, timeout=300)
                if child.returncode:
                    raise RuntimeError(f"run_dem on {args.baseline_lib} failed:\n{child.stderr[-2000:]}")
                base = json.loads(child.stdout.strip().splitlines()[-1])
                row.update(run_dem_parent_lib_s=base["run_dem_s"], ler_run_dem_parent_lib=base["ler"],
                           ratio_run_circuit_over_run_dem_parent_lib=row["run_circuit_s"] / base["run_dem_s"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_circuit.py", device=torch.cuda.get_device_name(dev), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
