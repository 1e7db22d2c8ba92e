#!/usr/bin/env python3
"""Reference-executed fixture for the posterior-LLR histograms: tests/golden/llr_hist.npz.

The lists live in two of the reference's scripts: BP_per_Iteration.py:52-60 extends ``iter_llrs`` with every posterior
of every trial and ``iter_llrs_after_OSD`` with those of the trials BP left unconverged, per iteration limit;
rework/Alvarado.py:159-162 splits a trial's posteriors by the TRUE value of the bit (``llr_data[...]["true_0"]`` /
``["true_1"]``).  This generator, run where a checkout of the reference is at hand (QLDPC_REFERENCE=<its directory>),
reads those files AT GENERATION TIME, compiles the text of those lines into a function and runs it on seeded error
patterns with the reference's own decoding/beliefPropagation.py.  Nothing of the loop bodies is stored: the fixture holds
the bit-packed error patterns and, per iteration limit and list, the ``np.histogram`` counts of the list over ``bins``
bins of ``[lo, hi]`` and the number of its values below and above that range.

The matrix is handed to the reference C-ordered: its dense column sums then add row by row, the order of the
Monte-Carlo kernels (oracle.colsum_flags).

    QLDPC_REFERENCE=<reference checkout> MPLBACKEND=Agg python tests/golden/make_golden_llr_hist.py
"""
import contextlib
import io
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["QLDPC_REFERENCE"]
LISTS = ("iter_llrs", "iter_llrs_after_OSD", "true_0", "true_1")
CODE, P, LIMITS, TRIALS = "[[72, 12, 6]]", 0.05, (2, 5, 10), 400
BINS, LO, HI = 48, -12.0, 12.0


def compile_trial():
    per_iter = open(os.path.join(REF, "BP_per_Iteration.py")).read().splitlines()[52 - 1:60]
    assert per_iter[0].strip() == "syndrome = (error @ code.T) % 2", per_iter[0]
    assert per_iter[-1].strip() == "iter_llrs_after_OSD.extend(llrs)", per_iter[-1]
    split = open(os.path.join(REF, "rework", "Alvarado.py")).read().splitlines()[159 - 1:162]
    assert split[0].strip() == "if collect_stats:" and split[-1].strip().startswith('llr_data[code_name]["true_1"]'), split
    src = ("def trial(error, code, initialBeliefs, max_iter, performBeliefPropagationFast, iter_llrs,\n"
           "          iter_llrs_after_OSD, llr_data, code_name, collect_stats=True):\n"
           + textwrap.indent(textwrap.dedent("\n".join(per_iter)), "    ") + "\n"
           + textwrap.indent(textwrap.dedent("\n".join(split)), "    ") + "\n")
    ns = {"np": np}
    exec(compile(src, "<BP_per_Iteration.py:52-60 + rework/Alvarado.py:159-162>", "exec"), ns)
    return ns["trial"]


def main():
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        from decoding.beliefPropagation import performBeliefPropagationFast
    trial = compile_trial()
    d = np.load(os.path.join(REF, "codes", f"{CODE}.npz"))
    code = np.ascontiguousarray(d["Hx"])
    n = code.shape[1]
    beliefs = [np.log((1 - P) / P)] * n
    rng = np.random.default_rng(20261020)
    errors = (rng.random((TRIALS, n)) < P).astype(int)
    out = {"code": np.array(CODE), "p": np.array(P), "limits": np.array(LIMITS, np.int32), "bins": np.array(BINS, np.int32),
           "range": np.array([LO, HI]), "errors": np.packbits(errors.astype(np.uint8), axis=1),
           "lists": np.array(LISTS)}
    counts = np.zeros((len(LIMITS), len(LISTS), BINS), np.int64)
    outside = np.zeros((len(LIMITS), len(LISTS), 2), np.int64)        # below lo, above hi
    for j, max_iter in enumerate(LIMITS):
        iter_llrs, after = [], []
        llr_data = {CODE: {"true_0": [], "true_1": []}}
        for error in errors:
            trial(error, code, beliefs, max_iter, performBeliefPropagationFast, iter_llrs, after, llr_data, CODE)
        for r, lst in enumerate((iter_llrs, after, llr_data[CODE]["true_0"], llr_data[CODE]["true_1"])):
            x = np.asarray(lst, np.float64)
            assert not np.isnan(x).any()
            counts[j, r] = np.histogram(x, BINS, range=(LO, HI))[0]
            outside[j, r] = ((x < LO).sum(), (x > HI).sum())
            assert counts[j, r].sum() + outside[j, r].sum() == len(x)
        assert len(iter_llrs) == TRIALS * n and len(after) % n == 0
        print(f"maxIter {max_iter}: {len(after) // n} of {TRIALS} trials unconverged, {int(outside[j, 0].sum())} values "
              f"outside [{LO}, {HI}], {int((counts[j, 0] > 0).sum())} of {BINS} bins in use", flush=True)
    out["counts"], out["outside"] = counts, outside
    path = os.path.join(HERE, "llr_hist.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
