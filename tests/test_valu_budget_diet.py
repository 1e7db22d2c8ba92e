"""Static vector-instruction budget of the headline loop after the second diet (tools/valu_mix.py on the built
library): 607.5 per BP iteration -- tests/test_valu_budget.py keeps the 621 of the diet before
and the FP64 classes, which did not move.
Skips when the library has not been built."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "qldpc_amd", "csrc", "libqbp.so")
HEADLINE = "bp_fused_kernelILi6ELi3ELi0ELb0ELb1ELi1024ELi1ELb1EE"


def test_vector_instructions_per_iteration_after_the_second_diet():
    if not os.path.exists(LIB):
        pytest.skip("libqbp.so not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import valu_mix
    res = valu_mix.analyse(LIB, [HEADLINE])
    assert len(res) == 1
    mix = next(iter(res.values()))
    assert mix["valu_total"] / 2 <= 608, mix["valu_by_class"]
    # 32-bit side: 164 before; the two reciprocal-table offsets (12) and the per-slot iteration counter went
    assert (mix["valu_by_class"].get("alu_b32", 0) + mix["valu_by_class"].get("lane_b32", 0)) / 2 <= 151
