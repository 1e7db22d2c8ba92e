"""CPU: fixed-weight Monte-Carlo (qbp_mc_run_weight, mc.run_weights, mc.ler_from_weights) -- the numpy statement of
the sampler (exact weight, uniformity), the weight-stratified LER against exact rational arithmetic, sharding of the
driver with an injected runner, and the argument checks that need no device."""
import itertools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from qldpc_amd import _lib, codes, mc
from weight_oracle import errors_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the statement of the sampler -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 37])
def test_statement_rows_have_exact_weight(n):
    for w in (0, 1, 5, n - 1, n):
        for seed, begin in ((0, 0), (0x1234567890, 2 ** 32 - 50)):
            e = errors_weight(n, w, seed, begin, 200)
            assert e.shape == (200, n) and e.dtype == np.uint8 and e.max(initial=0) <= 1
            assert np.array_equal(e.sum(axis=1), np.full(200, w)), (n, w, seed, begin)
    with pytest.raises(ValueError):
        errors_weight(n, n + 1, 0, 0, 1)


def test_statement_does_not_depend_on_the_split():
    whole = errors_weight(37, 9, 5, 2 ** 32 - 100, 257)
    parts = np.concatenate([errors_weight(37, 9, 5, 2 ** 32 - 100, 60), errors_weight(37, 9, 5, 2 ** 32 - 40, 197)])
    assert np.array_equal(whole, parts)
    assert not np.array_equal(whole, errors_weight(37, 9, 6, 2 ** 32 - 100, 257))      # (the seed matters)
    assert len({r.tobytes() for r in whole}) > 250                                      # (so does the trial)


def test_statement_is_uniform_over_subsets():
    # n = 7, w = 3: 35 subsets, 35 000 trials -> each count is Binomial(35 000, 1 / 35): mean 1000, sigma 31.2
    T = 35000
    e = errors_weight(7, 3, 0, 0, T)
    keys = e @ (1 << np.arange(7))
    subsets = [sum(1 << v for v in c) for c in itertools.combinations(range(7), 3)]
    counts = np.array([(keys == s).sum() for s in subsets])
    assert counts.sum() == T
    sigma = math.sqrt(T * (1 / 35) * (34 / 35))
    print("subset counts: min", counts.min(), "max", counts.max(), "5 sigma", 5 * sigma)
    assert np.all(np.abs(counts - 1000) <= 5 * sigma)


def test_statement_column_frequencies():
    # n = 72, w = 6: a column is in the subset with probability w / n; its count is Binomial(T, 1 / 12)
    n, w, T = 72, 6, 20000
    col = errors_weight(n, w, 0, 0, T).sum(axis=0)
    sigma = math.sqrt(T * (w / n) * (1 - w / n))
    print("column counts: min", col.min(), "max", col.max(), "mean", T * w / n, "5 sigma", 5 * sigma)
    assert np.all(np.abs(col - T * w / n) <= 5 * sigma)


# ---- 2. ler_from_weights ---------------------------------------------------------------------------------------------
def table_of(trials, errors):
    t = np.zeros((len(trials), mc.NUM_COUNTERS), np.int64)
    t[:, 0], t[:, 1] = trials, errors
    return t


def test_ler_equals_exact_rational_evaluation():
    n = 23
    weights = [0, 1, 2, 3, 5, 8, 13, 23]
    trials = [10, 1000, 1000, 777, 50, 12345, 3, 1]
    errors = [0, 0, 13, 77, 25, 12345, 2, 1]
    ps = [Fraction(1, 1000), Fraction(1, 20), Fraction(3, 10), Fraction(1, 2), Fraction(9, 10)]
    got = mc.ler_from_weights(table_of(trials, errors), weights, n, [float(p) for p in ps])
    for i, p in enumerate(ps):
        B = [math.comb(n, w) * p ** w * (1 - p) ** (n - w) for w in range(n + 1)]
        assert sum(B) == 1
        ler = sum(B[w] * Fraction(e, t) for w, t, e in zip(weights, trials, errors))
        miss = sum(B[w] for w in range(n + 1) if w not in weights)
        var = sum(B[w] ** 2 * Fraction(e, t) * (1 - Fraction(e, t)) / t for w, t, e in zip(weights, trials, errors))
        # lgamma is good to a few ulp of a logarithm of size <= 40: relative 1e-13; 1e-10 leaves room for the sums
        assert got["ler"][i] == pytest.approx(float(ler), rel=1e-10, abs=0)
        assert got["unsampled_mass"][i] == pytest.approx(float(miss), rel=1e-10, abs=0)
        assert got["ler_high"][i] == pytest.approx(float(ler + miss), rel=1e-10, abs=0)
        assert got["stderr"][i] == pytest.approx(math.sqrt(float(var)), rel=1e-10, abs=0)
    assert np.array_equal(got["p"], [float(p) for p in ps])


def test_ler_all_weights_failing_is_one():
    n = 31
    w = list(range(n + 1))
    got = mc.ler_from_weights(table_of([100] * (n + 1), [100] * (n + 1)), w, n, [0.0, 1e-3, 0.1, 0.5, 0.97, 1.0])
    assert got["ler"] == pytest.approx(1.0, rel=1e-12)
    assert got["ler_high"] == pytest.approx(1.0, rel=1e-12)
    assert np.all(got["unsampled_mass"] == 0) and np.all(got["stderr"] == 0)


def test_ler_high_adds_the_unsampled_mass():
    n = 144
    weights = [4, 6, 8, 10, 12]
    got = mc.ler_from_weights(table_of([1000] * 5, [0, 1, 10, 100, 500]), weights, n, [1e-3, 1e-2, 0.05, 0.2])
    assert np.all(got["ler"] <= got["ler_high"])
    for i, p in enumerate(got["p"]):
        B = mc.binomial_weights(n, p)
        assert B.sum() == pytest.approx(1.0, rel=1e-12)
        miss = B.sum() - B[weights].sum()
        assert got["ler_high"][i] - got["ler"][i] == pytest.approx(miss, rel=1e-9, abs=1e-15)
        assert got["unsampled_mass"][i] == pytest.approx(miss, rel=1e-9, abs=1e-15)
    # a weight without trials is unknown too, not a zero
    t = table_of([1000, 0], [10, 0])
    a = mc.ler_from_weights(t, [2, 3], 10, [0.1])
    b = mc.ler_from_weights(t[:1], [2], 10, [0.1])
    assert a["ler"][0] == b["ler"][0] and a["ler_high"][0] == b["ler_high"][0]


def test_ler_large_n_is_finite():
    n = 7776
    weights = [0, 5, 40, 78, 400, 7776]
    got = mc.ler_from_weights(table_of([1000] * 6, [0, 1, 30, 500, 1000, 1000]), weights, n, [1e-4, 1e-3, 0.01, 0.5])
    for k in ("ler", "ler_high", "stderr", "unsampled_mass"):
        assert np.all(np.isfinite(got[k])) and np.all(got[k] >= 0) and np.all(got[k] <= 1 + 1e-9), k
    assert mc.binomial_weights(n, 0.01).sum() == pytest.approx(1.0, rel=1e-9)
    assert got["ler"][2] > 0        # (p = 0.01: the mass sits around w = 78)


def test_ler_argument_errors():
    t = table_of([10, 10], [1, 1])
    for bad in ([1, 1], [1, 8], [-1, 2], [1.5, 2]):
        with pytest.raises(ValueError):
            mc.ler_from_weights(t, bad, 7, [0.1])
    with pytest.raises(ValueError):
        mc.ler_from_weights(t, [1, 2, 3], 7, [0.1])
    with pytest.raises(ValueError):
        mc.ler_from_weights(t, [1, 2], 7, [1.5])


# ---- 3. the drivers, with an injected runner ----------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 8])
def test_run_weights_shards_cover_the_range_once(world):
    trials, weights = 1003, [0, 3, 7, 72]
    code = codes.load_code("[[72, 12, 6]]")
    seen = {w: [] for w in weights}

    def runner_code(c, w, begin, end):
        assert c.n == 72
        seen[w].append((begin, end))
        return np.array([end - begin, w] + [0] * 10, np.int64)

    def runner_matrix(H, L, w, prior, begin, end):
        assert H.shape == code.Hx.shape and prior.shape == (72,)
        return runner_code(code, w, begin, end)

    for run in (lambda r, red: mc.run_weights("[[72, 12, 6]]", weights, trials, prior_p=0.01, rank=r, world=world,
                                              runner=runner_code, all_reduce=red),
                lambda r, red: mc.run_weights_matrix(code.Hx, code.Lx, weights, trials, prior=mc.prior_of(0.01, 72),
                                                     rank=r, world=world, runner=runner_matrix, all_reduce=red)):
        for w in weights:
            seen[w].clear()
        reduced = []
        tables = [run(r, lambda t: (reduced.append(t.copy()), t)[1]) for r in range(world)]
        assert len(reduced) == world
        total = np.sum(tables, axis=0)
        assert total.shape == (len(weights), mc.NUM_COUNTERS)
        assert np.array_equal(total[:, 0], [trials] * len(weights))
        assert np.array_equal(total[:, 1], [w * world for w in weights])
        for w in weights:
            ranges = sorted(seen[w])
            assert ranges[0][0] == 0 and ranges[-1][1] == trials and len(ranges) == world
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def _never(*a):
    raise AssertionError("the runner must not be reached")


def test_bad_arguments_raise_before_any_device_work():
    code = codes.load_code("[[72, 12, 6]]")
    for runner in (_never, None):       # (no runner: the default path would need a GPU, and must not get that far)
        for bad in ([-1], [73], [1.5], [[1, 2]]):
            with pytest.raises(ValueError):
                mc.run_weights("[[72, 12, 6]]", bad, 100, prior_p=0.01, runner=runner)
            with pytest.raises(ValueError):
                mc.run_weights_matrix(code.Hx, code.Lx, bad, 100, prior=mc.prior_of(0.01, 72), runner=runner)
        with pytest.raises(ValueError):
            mc.run_weights("[[72, 12, 6]]", [3], 100, prior_p=0.01, osd_order=3, runner=runner)
        with pytest.raises(ValueError):
            mc.run_weights_matrix(code.Hx, code.Lx, [3], 100, prior=np.zeros(71), runner=runner)
        with pytest.raises(ValueError):
            mc.run_weights_matrix(code.Hx, code.Lx[:, :70], [3], 100, prior=np.zeros(72), runner=runner)


@pytest.mark.parametrize("argv", [["--weights", "3"], ["--weights", "3", "--prior-p", "0"],
                                  ["--weights", "3", "300", "--prior-p", "0.01"],
                                  ["--weights", "3", "3", "--prior-p", "0.01"],
                                  ["--weights", "3", "--prior-p", "0.01", "--budgets", "10", "20"],
                                  ["--weights", "3", "--prior-p", "0.01", "--ler-at", "1.5"],
                                  ["--prior-p", "0.01"], ["--ler-at", "0.01"]])
def test_cli_refuses_bad_weight_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--weights" in err or "--ler-at" in err


# ---- 4. the C ABI without a device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    return _lib.load()


def test_null_handle_is_invalid(lib):
    counters = np.full(12, 7, np.int64)
    prior = np.zeros(4)
    errors = np.zeros((2, 4), np.uint8)
    # (h, Lx, k, distance, weight, seed, trial_begin, trial_end, prior, max_iter, variant, alpha, damping, clip_llr,
    #  flags, counters[, stream])
    args = (None, None, 0, 0, 2, 0, 0, 100, prior.ctypes.data, 10, 0, 1.0, 1.0, 20.0, 0, counters.ctypes.data)
    assert lib.qbp_mc_run_weight(*args) == -1
    assert b"null handle" in lib.qbp_last_error()
    assert lib.qbp_mc_run_weight_device(*args, None) == -1
    assert lib.qbp_mc_sample_errors_weight(None, 2, 0, 0, 2, errors.ctypes.data) == -1
    assert np.all(counters == 7)


def test_header_binding_and_option_agree():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for name, nargs in (("qbp_mc_run_weight", 16), ("qbp_mc_run_weight_device", 17),
                        ("qbp_mc_sample_errors_weight", 6)):
        assert f"int {name}(" in header
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert f"QBP_OPT_MC_WEIGHT_CHUNK = {_lib.OPT_MC_WEIGHT_CHUNK}," in header
    assert "(j + 1) / 2^32" in header       # (the bias bound is part of the specification)
