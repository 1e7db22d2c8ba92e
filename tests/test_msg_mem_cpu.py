"""CPU: the one statement of the LDS-or-workspace choice of Relay-BP, layered BP and BP guided decimation
(qldpc_amd/csrc/qbp_msg_mem.hpp: msg_mem_choose), built for the host by tests/_shim/msg_mem_shim.cpp -- its truth table
at and one byte past 160 KiB, and the build it chooses for the [[72,12,6]] phenomenological matrices around the limit
of each family's LDS build."""
import ctypes as C
import os
import subprocess

import pytest

import large_util as lu
import record_kernel_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
AT, PAST = 163840, 163841                    # 160 KiB and one byte more
BEYOND = 200000                              # (an LDS build's size that differs from the large build's PAST)


def _shim():
    src = os.path.join(HERE, "_shim", "msg_mem_shim.cpp")
    so = os.path.join(HERE, "_shim", "libmsgmemshim.so")
    deps = [src, os.path.join(HERE, "..", "qldpc_amd", "csrc", "qbp_msg_mem.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.msg_mem_limit.restype = C.c_ulonglong
    lib.msg_mem_choose.restype = None
    lib.msg_mem_choose.argtypes = [C.c_int, C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    return lib


def choose(mode, lds_need, large_need):
    """-> ("large" | "lds", None) of a launch, or ("refused", (the build blamed, its bytes))"""
    out = (C.c_ulonglong * 5)(7, 7, 7, 7, 7)
    _shim().msg_mem_choose(mode, lds_need, large_need, out)
    ok, large, calls, blamed_large, blamed_need = (int(v) for v in out)
    assert ok in (0, 1) and large in (0, 1) and calls == 1 - ok         # the formatter runs once, for a refusal only
    if ok:
        return ("large" if large else "lds"), None
    assert blamed_large == large
    return "refused", ("large" if blamed_large else "lds", blamed_need)


def test_the_limit_is_160_kib():
    assert _shim().msg_mem_limit() == AT == ru.LDS_LIMIT == 160 * 1024
    assert (lu.MEM_LDS, lu.MEM_LARGE, lu.MEM_AUTO) == (0, 1, 2)


FITS_LDS, FITS_LARGE_ONLY, FITS_NEITHER = (AT, AT), (PAST, AT), (BEYOND, PAST)     # (LDS build, large build) bytes
TRUTH = {
    (0, FITS_LDS): ("lds", None), (0, FITS_LARGE_ONLY): ("refused", ("lds", PAST)),
    (0, FITS_NEITHER): ("refused", ("lds", BEYOND)),
    (1, FITS_LDS): ("large", None), (1, FITS_LARGE_ONLY): ("large", None),
    (1, FITS_NEITHER): ("refused", ("large", PAST)),
    (2, FITS_LDS): ("lds", None), (2, FITS_LARGE_ONLY): ("large", None),
    (2, FITS_NEITHER): ("refused", ("large", PAST)),
}


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["lds_only", "workspace", "automatic"])
@pytest.mark.parametrize("sizes", [FITS_LDS, FITS_LARGE_ONLY, FITS_NEITHER], ids=["fits_lds", "fits_large_only", "fits_neither"])
def test_truth_table_at_and_one_byte_past_the_limit(mode, sizes):
    assert choose(mode, *sizes) == TRUTH[mode, sizes]
    # the boundary is `>`: a build of exactly 160 KiB runs, one byte more does not
    assert choose(mode, AT, AT)[0] != "refused" and choose(mode, PAST, PAST)[0] == "refused"
    assert choose(mode, PAST, PAST)[1] == (("large" if mode else "lds"), PAST)


# the family's byte counts (LDS build, large build) of a shape, as qbp.hip feeds them, and the rounds T of the
# [[72,12,6]] phenomenological matrix at which the LDS build stops fitting
FAMILIES = {
    "relay": (lambda sh: (ru.relay_lds_bytes(sh.m, sh.n, sh.E), lu.relay_large_lds_bytes(sh.m, sh.n)), 34),
    "gd_min_sum": (lambda sh: (ru.gd_lds_bytes(sh.m, sh.n, sh.E, False), lu.gd_large_lds_bytes(sh.m, sh.n, False)), 41),
    "gd_sum_product": (lambda sh: (ru.gd_lds_bytes(sh.m, sh.n, sh.E, True), lu.gd_large_lds_bytes(sh.m, sh.n, True)), 40),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_real_shapes_around_the_limit_of_the_lds_build(family):
    sizes, T = FAMILIES[family]
    before, beyond = sizes(ru.ph_shape(T - 1)), sizes(ru.ph_shape(T))
    assert before[0] <= AT < beyond[0] and before[1] < beyond[1] <= AT       # (what the rounds were chosen for)
    assert choose(lu.MEM_LDS, *before) == ("lds", None)
    assert choose(lu.MEM_LDS, *beyond) == ("refused", ("lds", beyond[0]))
    assert choose(lu.MEM_LARGE, *before) == choose(lu.MEM_LARGE, *beyond) == ("large", None)
    assert choose(lu.MEM_AUTO, *before) == ("lds", None)
    assert choose(lu.MEM_AUTO, *beyond) == ("large", None)
