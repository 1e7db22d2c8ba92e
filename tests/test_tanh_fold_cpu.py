"""CPU: np.tanh(q * 0.5) of the kernels (qbp_math.hpp: np_tanh_half) and the candidate that never forms the product --
r = fma(min(|q|, 64), 0.5, -midpoint), row and sign from q -- return the same bits as each other and as numpy on every
class of input: the fold is exact.  (It is not in the kernels: it moves six instructions per iteration between the
FP64 classes that tests/test_valu_budget.py pins; DESIGN.md section 4.  The candidate lives in
tests/_shim/tanh_fold_shim.cpp.)  And the reciprocal-table readers, whose byte offset now comes out of the shifted
operand by a byte select, return what the shift-and-mask forms returned.

References: the committed np.tanh vectors; the oracle's restatement of numpy's kernel (pinned to numpy by
tests/test_np_math.py); and np.tanh itself where this host's numpy runs the kernel the vectors come from.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_util
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "np_math.npz"))
DBL_MIN = np.finfo(np.float64).tiny
SUB_MIN = np.nextafter(0.0, 1.0)
SUB_MAX = np.nextafter(DBL_MIN, 0.0)


def _shim():
    src = os.path.join(HERE, "_shim", "tanh_fold_shim.cpp")
    so = os.path.join(HERE, "_shim", "libtanhfoldshim.so")
    deps = [src] + [os.path.join(HERE, "..", "qldpc_amd", "csrc", f) for f in ("qbp_math.hpp", "qbp_np_tables.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                               "-o", so, src])
    lib = C.CDLL(so)
    lib.fold_row_midpoint.restype = C.c_double
    return lib


def _tanh(which, q):
    q = np.ascontiguousarray(q, np.float64)
    y = np.empty_like(q)
    _shim().fold_tanh_half(C.c_int(which), q.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_long(q.size))
    return y


def _oracle_tanh(x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.empty_like(x)
    oracle.lib().oracle_np_tanh(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_int64(x.size))
    return y


def _numpy_uses_svml():
    from numpy._core._multiarray_umath import __cpu_features__ as feat
    return bool(feat.get("AVX512_SKX"))


def _neighbours(x):
    """x and its +-1, +-2 ulp neighbours"""
    out = [x]
    for direction in (-np.inf, np.inf):
        y = x
        for _ in range(2):
            y = np.nextafter(y, direction)
            out.append(y)
    return out


def _boundaries():
    # the interval of |x| is its exponent and top mantissa bit, clamped: rows change at high dwords e << 19,
    # e = 0x7f9 (0.1875) .. 0x807 (24.0); 0x7f8 (0.125, inside row 0) and 0x808 (32.0, the clamp) ride along
    hi = (np.arange(0x7f8, 0x809, dtype=np.uint64) << np.uint64(19 + 32))
    return hi.view(np.float64)


def _input_classes():
    with np.errstate(all="ignore"):
        gold = 2.0 * GOLD["tanh_x"]
    gold = gold[~np.isnan(gold)]                       # (NaN: its own test below)
    xb = np.array([v for b in _boundaries() for v in _neighbours(b)])
    edge = np.array([0.0, SUB_MIN, SUB_MAX, DBL_MIN, 2 * DBL_MIN, np.nextafter(DBL_MIN, 1.0), 3 * SUB_MIN,
                     np.nextafter(2 * DBL_MIN, 0.0), np.inf,
                     np.nextafter(48.0, 0.0), 48.0, 64.0, np.nextafter(64.0, np.inf), 1e300])
    rng = np.random.default_rng(20)
    draw = 10.0 ** rng.uniform(-320, 3, 1_000_000) * rng.choice([-1.0, 1.0], 1_000_000)
    return {"golden": gold, "boundaries": np.concatenate([2.0 * xb, -2.0 * xb]),
            "edge": np.concatenate([edge, -edge]), "log-uniform": draw}


CLASSES = _input_classes()


@pytest.mark.parametrize("name", list(CLASSES))
def test_bits_of_the_folded_form_and_of_numpy(name):
    q = CLASSES[name]
    got = _tanh(0, q)
    folded = _tanh(1, q)
    assert golden_util.same_bits(got, folded).all(), f"{name}: the folded form differs at {q[~golden_util.same_bits(got, folded)][:5]}"
    x = q * 0.5
    assert golden_util.same_bits(got, _oracle_tanh(x)).all(), f"{name}: differs from the oracle's np.tanh"
    if _numpy_uses_svml():
        with np.errstate(all="ignore"):
            assert golden_util.same_bits(got, np.tanh(x)).all(), f"{name}: differs from np.tanh(q * 0.5)"
    if name == "golden":
        gx, gy = GOLD["tanh_x"], GOLD["tanh_y"]
        gx, gy = gx[~np.isnan(gx)], gy[~np.isnan(gx)]
        keep = x == gx                                 # (all but where the doubling overflowed)
        assert keep.sum() > 0.9 * keep.size
        assert golden_util.same_bits(got[keep], gy[keep]).all()


def test_nan_and_the_nan_preserving_wrap():
    """np_tanh_half maps a NaN to +-1, and so does the folded form (bit for bit, the sign of the NaN);
    tanh_half_msg<1> hands the NaN itself on."""
    nan = np.array([np.nan, -np.nan, np.float64(np.nan), 1.5, -np.inf])
    nan[1] = np.copysign(np.nan, -1.0)
    got, folded = _tanh(0, nan), _tanh(1, nan)
    assert np.array_equal(got.view(np.uint64), folded.view(np.uint64))
    assert np.array_equal(got[:2], [1.0, -1.0])
    y = np.empty_like(nan)
    _shim().fold_tanh_half_msg1(nan.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_long(nan.size))
    assert np.isnan(y[:3]).all() and np.array_equal(y[3:], got[3:])


def test_subnormal_halves_need_row_zero_midpoint_zero():
    """The one place where q * 0.5 rounds: the half is subnormal.  Both forms are in row 0 there, and agree because
    its midpoint is 0.0; here: the table says so, and the odd subnormals (whose halves are
    ties) come out as RN(q / 2)."""
    assert _shim().fold_row_midpoint(0) == 0.0 and np.signbit(_shim().fold_row_midpoint(0)) == False  # noqa: E712
    odd = (np.arange(1, 4001, 2, dtype=np.uint64)).view(np.float64)
    near = (np.arange(1, 4001, 2, dtype=np.uint64) + (np.uint64(1) << np.uint64(52))).view(np.float64)   # [DBL_MIN, 2 DBL_MIN)
    for q in (odd, -odd, near, -near):
        assert np.array_equal(_tanh(0, q).view(np.uint64), _tanh(1, q).view(np.uint64))
        assert np.array_equal(_tanh(0, q), q * 0.5)          # tanh(x) = x to the last bit down there


@pytest.mark.parametrize("form", [0, 1])
def test_reciprocal_offsets_exhaustive(form):
    """np_rcp14 / np_rcp14_12 against the earlier shift-and-mask offsets: all 2^16 top-mantissa patterns, the other
    mantissa bits random, the exponents the kernels meet (1 + a: 0; 1 - a: 0 down to 2^-24)."""
    rng = np.random.default_rng(3)
    m16 = np.arange(65536, dtype=np.uint32)
    shim = _shim()
    for e in ((0,) if form == 1 else (0, -1, -2, -7, -23, -24)):
        v_hi = ((np.uint32(1023 + e) << np.uint32(20)) | (m16 << np.uint32(4)) |
                rng.integers(0, 16, 65536).astype(np.uint32)).astype(np.uint32)
        out = []
        for which in (0, 1):
            r_hi = np.empty_like(v_hi)
            shim.fold_rcp14_hi(C.c_int(which), C.c_int(form), v_hi.ctypes.data_as(C.c_void_p),
                               r_hi.ctypes.data_as(C.c_void_p), C.c_long(v_hi.size))
            out.append(r_hi)
        assert np.array_equal(out[0], out[1]), f"form {form}, exponent {e}"
