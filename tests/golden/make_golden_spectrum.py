#!/usr/bin/env python3
"""Reference-executed fixture for the residual-weight spectra and the iteration list: tests/golden/spectrum.npz.

The rule lives in the loop body of the reference's rework/main.py:78-112.  This generator, run where a checkout of the
reference is at hand (QLDPC_REFERENCE=<its directory>), reads that file AT GENERATION TIME, compiles the text of those
lines into a function and runs it on seeded error patterns with the reference's own rework/decoding.py (loaded by
path): performBeliefPropagationFast and performOSD_enhanced(order=0).  Nothing of the loop body is stored: the fixture
holds per case the bit-packed error patterns, the four weight lists as histograms [4, n + 1] (weights_found_BP,
weights_found_OSD, weights_found_BP_error, weights_found_OSD_error) and the per-trial iteration list.

Cases: "bp" fills the loop's performOSD_enhanced call with the identity (BP only: what the spectrum run classifies
without an OSD flag), "osd0" leaves the reference's call.  The matrix is handed to the reference C-ordered: its dense
column sums then add row by row, the order of the Monte-Carlo kernels (oracle.colsum_flags).

The OSD-0 order of exactly tied |LLR| is not restated by this project (ties go by column index; the reference's
np.argsort is unstable there).  So every pattern is also run through tests/spectrum_oracle.py on the CPU: a pattern on
which the two differ is replaced by the next draw and counted in "<case>/replaced"; more than 2 % of replaced draws
aborts the generation.

    QLDPC_REFERENCE=<reference checkout> MPLBACKEND=Agg python tests/golden/make_golden_spectrum.py
"""
import importlib.util
import os
import sys
import textwrap
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from spectrum_oracle import spectrum_of_errors  # noqa: E402

REF = os.environ["QLDPC_REFERENCE"]
FIRST, LAST = 78, 112           # 1-based, inclusive: the per-trial body of rework/main.py after the error is drawn
LISTS = ("weights_found_BP", "weights_found_OSD", "weights_found_BP_error", "weights_found_OSD_error")


def load_decoding():
    spec = importlib.util.spec_from_file_location("ref_rework_decoding", os.path.join(REF, "rework", "decoding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_loop_body():
    lines = open(os.path.join(REF, "rework", "main.py")).read().splitlines()[FIRST - 1:LAST]
    assert lines[0].strip() == "syndrome = (error @ code.T) % 2", lines[0]
    assert lines[-1].strip() == "if is_valid_osd: degenerateErrors += 1", lines[-1]
    body = textwrap.indent(textwrap.dedent("\n".join(lines)), "    ")
    src = ("def trial(error, code, Lx, initialBeliefs, BP_maxIter, OSD_order, performBeliefPropagationFast,\n"
           "          performOSD_enhanced):\n"
           "    logicalError = 0; OSD_invocations = 0; degenerateErrors = 0; OSD_invocation_AND_logicalError = 0\n"
           "    weights_found_BP = []; weights_found_OSD = []; iterations = []\n"
           "    weights_found_BP_error = []; weights_found_OSD_error = []\n"
           + body + "\n"
           "    return (weights_found_BP, weights_found_OSD, weights_found_BP_error, weights_found_OSD_error), iterations\n")
    ns = {"np": np}
    exec(compile(src, "<rework/main.py:78-112>", "exec"), ns)
    return ns["trial"]


def main():
    dec = load_decoding()
    trial = compile_loop_body()
    cases = [  # name, code file, p, maxIter, OSD, patterns
        ("72_bp", "[[72, 12, 6]]", 0.06, 50, False, 1500),
        ("144_osd0", "[[144, 12, 12]]", 0.06, 20, True, 1500),
    ]
    rng = np.random.default_rng(20261017)
    out = {}
    for name, fname, p, max_iter, osd, count in cases:
        d = np.load(os.path.join(REF, "codes", f"{fname}.npz"))
        code, Lx, distance = np.ascontiguousarray(d["Hx"]), np.ascontiguousarray(d["Lx"]), int(d["distance"])
        n = code.shape[1]
        beliefs = [np.log((1 - p) / p)] * n
        fill = dec.performOSD_enhanced if osd else (lambda code_, syndrome, llrs, detection, order=0: detection)
        weights = np.zeros((4, n + 1), np.int64)
        errors, iterations, replaced, t0 = [], [], 0, time.time()
        while len(errors) < count:
            error = (rng.random(n) < p).astype(int)
            lists, its = trial(error, code, Lx, beliefs, max_iter, 0, dec.performBeliefPropagationFast, fill)
            ref = np.zeros((4, n + 1), np.int64)
            for r, lst in enumerate(lists):
                for w in lst:
                    ref[r, int(w)] += 1
            cnt, spec, hist = spectrum_of_errors(code, Lx, distance, error[None, :].astype(np.uint8),
                                                 np.asarray(beliefs), max_iter, osd=osd)
            it_ok = hist[int(its[0]) if cnt[6] == 0 else max_iter] == 1 and (cnt[6] == 0 or int(its[0]) == max_iter - 1)
            if not np.array_equal(spec, ref) or not it_ok:
                replaced += 1
                assert replaced <= 0.02 * (len(errors) + replaced) + 1, (name, replaced, len(errors))
                continue
            weights += ref
            errors.append(error)
            iterations.append(int(its[0]))
        assert replaced <= 0.02 * (count + replaced), (name, replaced)
        E = np.asarray(errors, np.uint8)
        cnt, spec, hist = spectrum_of_errors(code, Lx, distance, E, np.asarray(beliefs), max_iter, osd=osd)
        assert np.array_equal(spec, weights) and cnt[7] == sum(iterations), name
        out[f"{name}/code"] = np.array(fname)
        out[f"{name}/meta"] = np.array([p, max_iter, int(osd), distance], np.float64)
        out[f"{name}/errors"] = np.packbits(E, axis=1)
        out[f"{name}/weights"] = weights
        out[f"{name}/iterations"] = np.asarray(iterations, np.int32)
        out[f"{name}/replaced"] = np.array(replaced, np.int64)
        print(f"{name}: {count} patterns, {replaced} replaced, {int(cnt[6])} not converged, lists "
              f"{dict(zip(LISTS, weights.sum(axis=1).tolist()))}  [{time.time() - t0:.0f} s]", flush=True)
    out["names"] = np.array([c[0] for c in cases])
    path = os.path.join(HERE, "spectrum.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
