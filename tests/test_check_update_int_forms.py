"""Integer side of the check update (qbp_math.hpp), host build: every rewritten integer expression equals the form it
replaced over its whole input domain, and the per-row syndrome sign gives numpy's bits.

* reciprocal table (np_rcp14 / np_rcp14_12): 32 bins of 2^11 mantissa values with the entry in the high dword of a
  zero low dword, the operand's exponent subtracted together with its mantissa bits -- against the 64-bin form
  ((ent - m16) & 0xffff0000) - (hi & 0x7ff00000) for every high dword of P in [1, 2) and of M in [2^-24, 1];
* log-table offset (np_log_row): one bit-field extract against (r_hi >> 12) & 0xf0 on every reciprocal it can see;
* sign: check_message_signed of a quotient whose dividend carries the syndrome sign against check_message, and
  against numpy's np.arctanh (the oracle), on all four sign combinations, +-0, +-inf and NaN."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "qldpc_amd", "csrc")

SHIM = r'''
#include "qbp_math.hpp"
using namespace qbp;
alignas(16) static const NpImage img = np_make_image();
static NpT tab() { return reinterpret_cast<const double*>(&img); }
extern "C" {
void rcp_m(const unsigned* v, unsigned* hi, unsigned* lo, long n)
{ for (long i = 0; i < n; ++i) { const double r = np_rcp14(v[i], tab()); hi[i] = np_hi(r); lo[i] = np_lo(r); } }
void rcp_p(const unsigned* v, unsigned* hi, unsigned* lo, long n)
{ for (long i = 0; i < n; ++i) { const double r = np_rcp14_12(v[i], tab()); hi[i] = np_hi(r); lo[i] = np_lo(r); } }
void log_row(const unsigned* r, unsigned* o, long n) { for (long i = 0; i < n; ++i) o[i] = np_log_row(r[i]); }
void div_q(const double* a, const double* b, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = div_nr(a[i], b[i]); }
void msg(const double* x, const unsigned char* s, double* old_, double* new_, long n, int variant)
{
    for (long i = 0; i < n; ++i) {
        if (variant == 1) {
            old_[i] = check_message<1, true>(x[i], s[i], tab());
            new_[i] = check_message_signed<1>(with_syndrome_sign(x[i], s[i]), tab());
        } else {
            old_[i] = check_message<0, true>(x[i], s[i], tab());
            new_[i] = check_message_signed<0>(with_syndrome_sign(x[i], s[i]), tab());
        }
    }
}
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("intforms")
    src, so = d / "shim.cpp", d / "libintforms.so"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                           "-I", CSRC, "-o", str(so), str(src)])
    return C.CDLL(str(so))


def _thresholds():
    txt = open(os.path.join(CSRC, "qbp_np_tables.hpp")).read()
    thr = [int(v, 16) for v in re.search(r"NP_RCP14_THR16\[16\] = \{([^}]*)\}", txt).group(1).split(",")]
    assert len(thr) == 16 and thr == sorted(thr)
    return thr


def _old_luts():
    """The 64-entry tables of the form this one replaced (bins of 2^10 mantissa values)."""
    thr = _thresholds()
    lut, lut_p = [], []
    for b in range(64):
        k_left = sum(1 for t in thr if t <= b << 10)
        inside = [t for t in thr if (b << 10) < t < ((b + 1) << 10)]
        t = inside[0] if inside else 0x10000
        ent = (0x3ff0ffff - (k_left << 16) - (0x10000 - t)) & 0xffffffff
        lut.append((ent + 0x3ff00000) & 0xffffffff)
        lut_p.append((ent + 0x03ff0000) & 0xffffffff)
    return np.array(lut, np.uint64), np.array(lut_p, np.uint64)


def _old_rcp_m(v):
    lut, _ = _old_luts()
    v = v.astype(np.uint64)
    ent = lut[(v >> 14) & 63]
    r = ((ent - ((v >> 4) & 0xffff)) & 0xffff0000) - (v & 0x7ff00000)
    return (r & 0xffffffff).astype(np.uint32)


def _old_rcp_p(v):
    _, lut_p = _old_luts()
    v = v.astype(np.uint64)
    r = (lut_p[(v >> 14) & 63] - (v >> 4)) & 0xffff0000
    return (r & 0xffffffff).astype(np.uint32)


def _run2(fn, v):
    v = np.ascontiguousarray(v, np.uint32)
    hi, lo = np.empty_like(v), np.empty_like(v)
    fn(v.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), C.c_long(v.size))
    return hi, lo


def _log_row(shim, r):
    r = np.ascontiguousarray(r, np.uint32)
    o = np.empty_like(r)
    shim.log_row(r.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), C.c_long(r.size))
    return o


MANT = np.arange(1 << 20, dtype=np.uint32)


def test_reciprocal_of_P_every_high_dword(shim):
    """P = 1 + a in [1, 2): all 2^20 high dwords (the low dword does not enter)."""
    v = np.uint32(0x3ff00000) | MANT
    hi, lo = _run2(shim.rcp_p, v)
    assert (lo == 0).all()
    assert np.array_equal(hi, _old_rcp_p(v))
    assert np.array_equal(_log_row(shim, hi), (hi >> np.uint32(12)) & np.uint32(0xf0))


def test_reciprocal_of_M_every_high_dword(shim):
    """M = 1 - a in [1e-7, 1]: every high dword of exponents 2^-24 .. 2^-1, and M = 1."""
    for e in range(-24, 0):
        v = np.uint32((1023 + e) << 20) | MANT
        hi, lo = _run2(shim.rcp_m, v)
        assert (lo == 0).all(), e
        assert np.array_equal(hi, _old_rcp_m(v)), e
        assert np.array_equal(_log_row(shim, hi), (hi >> np.uint32(12)) & np.uint32(0xf0)), e
    v = np.array([0x3ff00000], np.uint32)
    hi, lo = _run2(shim.rcp_m, v)
    assert hi[0] == _old_rcp_m(v)[0] == 0x3ff00000 and lo[0] == 0


def test_reciprocal_of_M_outside_the_domain(shim):
    """Off the domain (a NaN message: M is NaN, the result is discarded by the arithmetic) the new form still
    equals the old one bit for bit, negative sign bit included."""
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                        np.uint32(0x7ff00000) | MANT, np.uint32(0xfff00000) | MANT])
    hi, lo = _run2(shim.rcp_m, v)
    assert (lo == 0).all()
    assert np.array_equal(hi, _old_rcp_m(v))


def test_division_is_odd_in_both_operands(shim):
    """div_nr(+-a, +-b) = +-div_nr(a, b), the sign the XOR of the operands' signs, over the operand range of the
    check step (1e-15 <= |prod| <= |t| <= 1)."""
    rng = np.random.default_rng(5)
    t = 10.0 ** rng.uniform(-15, 0, 200000)
    p = t * 10.0 ** rng.uniform(-15, 0, t.size)
    p = np.maximum(p, 1e-15)
    out = {}
    for sa in (1.0, -1.0):
        for sb in (1.0, -1.0):
            a, b = sa * p, sb * t
            y = np.empty_like(a)
            shim.div_q(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p),
                     C.c_long(a.size))
            out[sa, sb] = y
    base = out[1.0, 1.0]
    for (sa, sb), y in out.items():
        assert golden_util.same_bits(y, sa * sb * base).all(), (sa, sb)


def test_syndrome_sign_on_the_row_product(shim):
    """check_message_signed(x * syndrome_sign) == check_message(x, syndrome bit) bit for bit -- both signs of x,
    both syndrome bits, +-0, +-inf, subnormals, NaN of either sign -- and equals numpy's 2 * arctanh(clip(.))."""
    from oracle import oracle
    rng = np.random.default_rng(9)
    mag = np.concatenate([10.0 ** rng.uniform(-15, 0, 40000), 1 - 10.0 ** rng.uniform(-9, 0, 20000),
                          [0.0, 1e-310, 1e-15, 0.9999999, 1.0, 7.0, np.inf]])
    x = np.concatenate([mag, -mag])
    nan = np.array([np.nan, -np.nan])
    for variant in (0, 1):
        xs = np.concatenate([x, x, nan, nan])
        sb = np.concatenate([np.zeros(x.size), np.ones(x.size), [0, 0], [1, 1]]).astype(np.uint8)
        old, new = np.empty_like(xs), np.empty_like(xs)
        shim.msg(xs.ctypes.data_as(C.c_void_p), sb.ctypes.data_as(C.c_void_p), old.ctypes.data_as(C.c_void_p),
                 new.ctypes.data_as(C.c_void_p), C.c_long(xs.size), C.c_int(variant))
        # bit for bit, NaN payload and sign included
        assert np.array_equal(old.view(np.uint64), new.view(np.uint64)), variant
        fin = ~np.isnan(xs)
        y = np.clip(xs[fin] * (1.0 - 2.0 * sb[fin]), -0.9999999, 0.9999999)
        want = np.empty_like(y)
        oracle.lib().oracle_np_arctanh(y.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p),
                                       C.c_int64(y.size))
        # (the kernels' NORMAL form skips the 0.5 / 2.0 round trip, which only subnormal results notice)
        keep = (np.abs(y) >= 1e-300) | (y == 0)
        assert golden_util.same_bits(new[fin][keep], 2.0 * want[keep]).all(), variant
