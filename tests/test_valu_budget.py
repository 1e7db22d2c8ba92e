"""Static vector-instruction budget of the headline kernel's loop (tools/valu_mix.py on the built library): the
integer work of the check update was cut, the FP64 work -- numpy's own operation sequence -- must not move.
Skips when the library has not been built."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "qldpc_amd", "csrc", "libqbp.so")
HEADLINE = "bp_fused_kernelILi6ELi3ELi0ELb0ELb1ELi1024ELi1ELb1EE"

# per BP iteration (the one-barrier loop holds two): the FP64 classes of the numpy-exact arithmetic
FP64_PER_ITERATION = {"fma_f64": 264, "add_f64": 132, "mul_f64": 29, "trans_f64": 6,
                      "minmax_f64": 12, "cmp_f64": 8, "cvt_f64": 6}
# 656 before the integer rewrite of the check update
MAX_PER_ITERATION = 621


@pytest.fixture(scope="module")
def mix():
    if not os.path.exists(LIB):
        pytest.skip("libqbp.so not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import valu_mix
    res = valu_mix.analyse(LIB, [HEADLINE])
    assert len(res) == 1
    return next(iter(res.values()))


def test_fp64_classes_unchanged(mix):
    per = {c: n / 2 for c, n in mix["valu_by_class"].items() if c.endswith("_f64")}
    assert per == FP64_PER_ITERATION


def test_vector_instructions_per_iteration(mix):
    assert mix["valu_total"] / 2 <= MAX_PER_ITERATION, mix["valu_by_class"]
