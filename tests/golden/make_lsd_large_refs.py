#!/usr/bin/env python3
"""Writes tests/golden/lsd_large_refs.npz: the outputs of the numpy statement of localized statistics decoding
(tests/lsd_oracle.py, lsd_decode_batch) on the two cases of tests/test_gpu_lsd_large.py that cost it more than about
five seconds -- 612 x 1836 (one record runs 720 rounds at g = 1) and 2049 x 384 -- at g = 1 and g = 0, with the records
they were computed from (make_inputs of that file), which the test reads from here as well.

    python tests/golden/make_lsd_large_refs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import lsd_oracle as lo  # noqa: E402
import test_gpu_lsd_large as T  # noqa: E402


def main():
    out = {}
    for tag in T.GOLDEN_TAGS:
        H, syn, llr, hard = T.make_inputs(tag)
        out[f"{tag}_syn"], out[f"{tag}_llr"], out[f"{tag}_hard"] = syn, llr, hard
        for g in (1, 0):
            r = lo.lsd_decode_batch(H, syn, llr, hard, g)
            for k in T.GOLDEN_KEYS:
                out[f"{tag}_g{g}_{k}"] = r[k]
            print(tag, g, lo.presence(r))
    np.savez_compressed(T.GOLDEN_PATH, **out)


if __name__ == "__main__":
    main()
