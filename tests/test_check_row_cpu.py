"""CPU: the row update of qldpc_amd/csrc/qbp_check.hpp (host build) returns the oracle's bits.

A 1 x D matrix decoded for one check step: at iteration 0 the variable->check messages are the priors, so the
oracle's message dump (`oracle.check_messages`, the reference's alpha_estimation output) is exactly the row
update of the vector passed as prior.  Checked: `check_row`, the update of rows of weight 1 .. 8 that all three
kernel families run, and the two-pass form of the general-H and streaming kernels' rows of weight > 8
(minsum_row / minsum_message / sp_message), with rows on both sides of the t_safe threshold.

On the device `check_row` takes sp_message for the whole wavefront when one lane's product is below 1e-15; on
the host each row decides alone.  Both paths are exact for products of at least 1e-15, so the per-lane bits
checked here are the device's either way.

Two known differences from the oracle, both of div_nr (qbp_math.hpp) and shared by every kernel, are kept
out of the main comparison and pinned by strict xfail tests: the sign of a zero message of a row whose product
is zero, and the last bit of quotients below div_nr's exact range (products below about 1e-280)."""
import ctypes as C

import numpy as np
import pytest

from golden_util import same_bits
from oracle import oracle
from test_math_cpu import _build


@pytest.fixture(scope="module", params=["", "_p", "_m"])
def shim(request):
    extra = {"": [], "_p": ["-DQBP_TEST_SEED_ERR=5e-8"], "_m": ["-DQBP_TEST_SEED_ERR=-5e-8"]}
    return _build(request.param, extra[request.param])


def _rows(D, nan, rng):
    """Messages of many rows of weight D: ordinary, tied, signed zeros, infinities, NaN, tiny, huge."""
    rows = [rng.normal(0, 5, D) for _ in range(12)]
    rows += [rng.choice([-1, 1], D) * 10.0 ** rng.uniform(-16, 2, D) for _ in range(12)]
    for _ in range(6):                               # exact ties in |q| (argmin: first occurrence)
        v = rng.choice([0.5, 1.25, 3.0, 1e-14], D) * rng.choice([-1, 1], D)
        rows.append(v)
    rows.append(np.full(D, 2.0))
    rows.append(np.full(D, -0.75))
    for _ in range(4):                               # +-0, +-inf
        v = rng.normal(0, 3, D)
        v[rng.random(D) < 0.4] = 0.0
        v[rng.random(D) < 0.3] = -0.0
        v[rng.random(D) < 0.25] = np.inf
        v[rng.random(D) < 0.25] = -np.inf
        rows.append(v)
    rows.append(np.full(D, np.inf))
    rows.append(np.full(D, -0.0))
    rows.append(np.full(D, 0.0))
    for _ in range(4):                               # very large and saturating
        rows.append(rng.choice([-1, 1], D) * rng.choice([1e300, 40.0, 38.2, 1e16, 700.0], D))
    for _ in range(6):                               # |prod| < 1e-15: the t_safe clamp
        v = rng.normal(0, 3, D)
        v[rng.integers(D)] = rng.choice([-1, 1]) * rng.choice([1e-14, 2e-15, 1e-200, 1e-300, 5e-320])
        rows.append(v)
        rows.append(rng.choice([-1, 1], D) * rng.uniform(0.002, 0.013, D))    # many messages near 0.006
    if nan:
        for _ in range(4):
            v = rng.normal(0, 3, D)
            v[rng.integers(D)] = np.nan
            rows.append(v)
        rows.append(np.full(D, np.nan))
    return [np.ascontiguousarray(r, np.float64) for r in rows]


def _oracle(q, sbit, variant, alpha):
    """R of the row: unscaled for sum-product, R / alpha for min-sum (the dump's conventions)."""
    H = np.ones((1, len(q)), np.int64)
    return oracle.check_messages(H, [[sbit]], q, variant, alpha=alpha, clip_llr=np.inf, iteration=0)[0]


def _device(fn, variant, q, sbit, alpha, scale):
    out = np.empty_like(q)
    rc = fn(C.c_int(variant), C.c_int(len(q)), q.ctypes.data_as(C.c_void_p), C.c_uint(sbit), C.c_double(alpha),
            C.c_int(int(scale)), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def _sp_cases(rows):
    """(q, prod) of the sum-product rows: (regular, zero product, product below div_nr's exact range)."""
    reg, zero, tiny = [], [], []
    for q in rows:
        with np.errstate(all="ignore"):
            prod = np.prod(np.tanh(q * 0.5))
        (zero if prod == 0.0 else tiny if abs(prod) < 1e-280 else reg).append(q)
    return reg, zero, tiny


def _compare_sp(fn, variant, q, sbit):
    """Both outputs (alpha_estimation dump and scaled) against the oracle; False at the first difference."""
    # the oracle's sum-product dump is variant 1's R before the alpha scaling; variant 0 differs from it only
    # on NaN messages, which it never sees (undamped R is finite, so Q = value - R is never inf - inf)
    want = _oracle(q, sbit, 1, 1.0)
    if not same_bits(_device(fn, variant, q, sbit, 0.7, False), want).all():
        return False
    return bool(same_bits(_device(fn, variant, q, sbit, 0.7, True), want * 0.7 if variant == 1 else want).all())


def _all_rows(degrees):
    rng = np.random.default_rng(20261016)
    for D in degrees:
        for variant in (0, 1, 2):
            yield D, variant, _rows(D, variant != 0, rng)


def _check(fn, degrees):
    cold = 0
    for D, variant, rows in _all_rows(degrees):
        if variant == 2:
            for q in rows:
                for sbit in (0, 1):
                    for alpha in (1.0, 0.8):
                        got = _device(fn, 2, q, sbit, alpha, True)
                        want = _oracle(q, sbit, 2, alpha)
                        what = f"variant 2 D {D} sbit {sbit} alpha {alpha} q {q.tolist()}"
                        assert same_bits(got / alpha, want).all(), f"{what}: {got} {want * alpha}"
                        if alpha == 1.0:
                            assert same_bits(got, want).all(), what
            continue
        reg, _, _ = _sp_cases(rows)
        for q in reg:
            with np.errstate(all="ignore"):
                cold += bool(abs(np.prod(np.tanh(q * 0.5))) < 1e-15)
            for sbit in (0, 1):
                assert _compare_sp(fn, variant, q, sbit), f"variant {variant} D {D} sbit {sbit} q {q.tolist()}"
    assert cold > 0


FORMS = {"row": ("shim_check_row", range(1, 9)), "long": ("shim_check_long", list(range(1, 13)) + [16, 23, 31, 40])}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_row_update_matches_oracle(shim, form):
    name, degrees = FORMS[form]
    _check(getattr(shim, name), degrees)


def _known_cases(kind):
    out = []
    for form, (name, degrees) in sorted(FORMS.items()):
        for D, variant, rows in _all_rows(degrees):
            if variant != 2:
                out += [(name, variant, q) for q in _sp_cases(rows)[kind]]
    return out


@pytest.mark.xfail(strict=True, reason="div_nr(+-0, t) rounds its residual step to +0: the sign of a zero "
                                       "message of a zero-product row can differ from numpy's")
def test_zero_product_rows_match_oracle(shim):
    cases = _known_cases(1)
    assert cases
    for name, variant, q in cases:
        for sbit in (0, 1):
            assert _compare_sp(getattr(shim, name), variant, q, sbit), f"{name} variant {variant} q {q.tolist()}"


@pytest.mark.xfail(strict=True, reason="div_nr is correctly rounded down to quotients of about 2^-1000 only "
                                       "(qbp_math.hpp): products below ~1e-280 can differ in the last bit")
def test_tiny_product_rows_match_oracle(shim):
    cases = _known_cases(2)
    assert cases
    for name, variant, q in cases:
        for sbit in (0, 1):
            assert _compare_sp(getattr(shim, name), variant, q, sbit), f"{name} variant {variant} q {q.tolist()}"
