"""CPU: the weight-w enumeration (qbp_mc_run_enum, qbp_enum_failures, qldpc_amd/enumerate.py) -- the Python statement
of the pattern order against itertools.combinations and an independent unranker, the class sizes, the exact weights of
ler_from_weights, the sharding of run_enumerate with an injected runner, and the C ABI where it needs no device."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from qldpc_amd import _lib, codes, enumerate as en, mc
import enum_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the order --------------------------------------------------------------------------------------------------
def test_statement_equals_itertools_on_every_small_class():
    for n in range(0, 13):
        for w in range(0, n + 1):
            combos = list(itertools.combinations(range(n), w))
            ranks = list(range(len(combos)))
            assert en.count(n, w) == len(combos) == math.comb(n, w)
            cols = en.unrank(n, w, ranks)
            assert cols.shape == (len(combos), w) and cols.dtype == np.int64
            assert np.array_equal(cols, np.asarray(combos, np.int64).reshape(len(combos), w)), (n, w)
            assert en.rank(n, w, cols) == ranks, (n, w)
            rows = en.patterns(n, w, ranks)
            assert rows.dtype == np.uint8 and np.array_equal(rows, enum_oracle.patterns(n, w)), (n, w)


def successor(cols, n):
    """The lexicographic successor of an ascending tuple: bump the last column that has room, reset those behind it."""
    cols = list(cols)
    w = len(cols)
    for i in reversed(range(w)):
        if cols[i] < n - (w - i):
            cols[i] += 1
            for j in range(i + 1, w):
                cols[j] = cols[j - 1] + 1
            return cols
    raise AssertionError("the last tuple has no successor")


def test_large_ranks_invert_and_step():
    n, w = 288, 5
    total = math.comb(n, w)
    assert total > 2 ** 33
    rng = np.random.default_rng(288)
    ranks = [0, 1, total - 1] + list(range(2 ** 32 - 2, 2 ** 32 + 3)) + [int(r) for r in rng.integers(0, total - 1, 200)]
    cols = en.unrank(n, w, ranks)
    assert en.rank(n, w, cols) == ranks
    for r, c in zip(ranks, cols):
        assert list(c) == enum_oracle.unrank_int(n, w, r)
        if r + 1 < total:
            assert list(en.unrank(n, w, [r + 1])[0]) == successor(c, n), r
    assert list(cols[0]) == [0, 1, 2, 3, 4] and list(cols[2]) == [283, 284, 285, 286, 287]
    with pytest.raises(ValueError):
        en.unrank(n, w, [total])
    with pytest.raises(ValueError):
        en.rank(n, w, [[0, 1, 2, 4, 3]])


def test_count():
    for n, w in ((7, 3), (72, 3), (144, 4), (288, 3), (288, 0), (288, 288), (7776, 5), (62, 31)):
        assert en.count(n, w) == math.comb(n, w)
    assert (en.count(72, 3), en.count(144, 4), en.count(288, 3)) == (59640, 17178876, 3939936)
    assert math.comb(7776, 6) > 2 ** 62 > math.comb(7776, 5)
    for n, w in ((7776, 6), (288, 40), (7, 8), (7, -1)):
        with pytest.raises(ValueError):
            en.count(n, w)


# ---- 2. ler_from_weights -------------------------------------------------------------------------------------------
def recorded_table():
    t = np.zeros((6, mc.NUM_COUNTERS), np.int64)
    t[:, 0] = [1, 72, 2556, 59640, 100000, 100000]
    t[:, 1] = [0, 0, 0, 36, 431, 2977]
    return t, [0, 1, 2, 3, 4, 5], 72, [1e-4, 1e-3, 0.01, 0.05]


# mc.ler_from_weights(*recorded_table()) before the keyword existed, digit for digit
RECORDED = {
    "ler": ['0x1.3e645c5c1569fp-35', '0x1.478a03c00369fp-25', '0x1.0277c865881ccp-14', '0x1.52849f2e73550p-8'],
    "ler_high": ['0x1.3e64b5eacfbe8p-35', '0x1.48ceb190b7c6ap-25', '0x1.3b8481f614a24p-13', '0x1.3f89e8d3b2a3cp-3'],
    "stderr": ['0x1.a32f667affad0p-38', '0x1.80f0bfc89082bp-28', '0x1.ae9e7c407c415p-19', '0x1.738a08aa54783p-14'],
    "unsampled_mass": ['0x1.663ae95234d61p-53', '0x1.44add0b45cb55p-33', '0x1.74913b86a127bp-14', '0x1.34f5c3da3f091p-3'],
}


def test_ler_default_is_unchanged():
    got = mc.ler_from_weights(*recorded_table())
    for k, want in RECORDED.items():
        assert [float(x).hex() for x in got[k]] == want, k
    again = mc.ler_from_weights(*recorded_table(), exact_weights=())
    for k in RECORDED:
        assert np.array_equal(got[k], again[k])


def test_exact_weights_carry_no_variance():
    table, weights, n, ps = recorded_table()
    base = mc.ler_from_weights(table, weights, n, ps)
    exact = mc.ler_from_weights(table, weights, n, ps, exact_weights=[0, 1, 2, 3])
    for k in ("ler", "ler_high", "unsampled_mass"):
        assert np.array_equal(base[k], exact[k]), k
    for i, p in enumerate(ps):
        B = mc.binomial_weights(n, p)
        var = sum(B[w] ** 2 * (e / t) * (1 - e / t) / t for w, t, e in zip(weights, table[:, 0], table[:, 1]) if w >= 4)
        assert exact["stderr"][i] == pytest.approx(math.sqrt(var), rel=1e-12, abs=0)
        assert exact["stderr"][i] < base["stderr"][i]
    all_exact = mc.ler_from_weights(table[:4], weights[:4], n, ps, exact_weights=weights[:4])
    assert np.all(all_exact["stderr"] == 0)


def test_exact_weights_must_be_whole_classes():
    table, weights, n, ps = recorded_table()
    with pytest.raises(ValueError):
        mc.ler_from_weights(table, weights, n, ps, exact_weights=[4])        # 100 000 trials, not C(72, 4)
    short = table.copy()
    short[3, 0] -= 1
    with pytest.raises(ValueError):
        mc.ler_from_weights(short, weights, n, ps, exact_weights=[3])
    with pytest.raises(ValueError):
        mc.ler_from_weights(table, weights, n, ps, exact_weights=[6])        # not a row of the table


def test_merge_weight_tables():
    table, weights, n, ps = recorded_table()
    merged, w = mc.merge_weight_tables(table[:4], weights[:4], table[4:], weights[4:])
    assert np.array_equal(merged, table) and w == weights
    a = mc.ler_from_weights(merged, w, n, ps, exact_weights=weights[:4])
    b = mc.ler_from_weights(table, weights, n, ps, exact_weights=weights[:4])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        mc.merge_weight_tables(table[:4], weights[:4], table[3:], weights[3:])
    with pytest.raises(ValueError):
        mc.merge_weight_tables(table[:4], weights[:3], table[4:], weights[4:])


# ---- 3. the drivers, with an injected runner ------------------------------------------------------------------------
def test_run_enumerate_shards_cover_every_class_once():
    weights = [0, 1, 3, 71, 72]
    code = codes.load_code("[[72, 12, 6]]")
    seen = {}

    def runner_code(c, w, begin, end):
        assert c.n == 72
        seen.setdefault(w, []).append((begin, end))
        # (a count that depends on the ranks themselves: the sum of the ranks)
        return np.array([end - begin, (begin + end - 1) * (end - begin) // 2] + [0] * 10, np.int64)

    def runner_matrix(H, L, w, prior, begin, end):
        assert H.shape == code.Hx.shape and prior.shape == (72,)
        return runner_code(code, w, begin, end)

    results = []
    for world in (1, 2, 8):
        for run in (lambda r, red: mc.run_enumerate("[[72, 12, 6]]", weights, prior_p=0.01, rank=r, world=world,
                                                    runner=runner_code, all_reduce=red),
                    lambda r, red: mc.run_enumerate_matrix(code.Hx, code.Lx, weights, prior=mc.prior_of(0.01, 72), rank=r,
                                                           world=world, runner=runner_matrix, all_reduce=red)):
            seen.clear()
            reduced = []
            total = np.sum([run(r, lambda t: (reduced.append(t.copy()), t)[1]) for r in range(world)], axis=0)
            assert len(reduced) == world
            assert total.shape == (len(weights), mc.NUM_COUNTERS)
            assert [int(x) for x in total[:, 0]] == [math.comb(72, w) for w in weights]
            for w in weights:
                ranges = sorted(seen[w])
                assert len(ranges) == world and ranges[0][0] == 0 and ranges[-1][1] == math.comb(72, w)
                assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            results.append(total)
    assert all(np.array_equal(results[0], t) for t in results[1:])          # (independent of world)


def _never(*a):
    raise AssertionError("the runner must not be reached")


def test_run_enumerate_refuses_before_any_device_work():
    code = codes.load_code("[[288, 12, 18]]")
    for runner in (_never, None):
        for bad in ([-1], [289], [1.5], [40]):          # (C(288, 40) is far beyond 2^62)
            with pytest.raises(ValueError):
                mc.run_enumerate("[[288, 12, 18]]", bad, prior_p=0.01, runner=runner)
            with pytest.raises(ValueError):
                mc.run_enumerate_matrix(code.Hx, code.Lx, bad, prior=mc.prior_of(0.01, 288), runner=runner)


@pytest.mark.parametrize("argv", [["--enumerate", "3"], ["--enumerate", "3", "--prior-p", "0"],
                                  ["--enumerate", "3", "300", "--prior-p", "0.01"],
                                  ["--enumerate", "3", "--weights", "3", "--prior-p", "0.01"],
                                  ["--enumerate", "36", "--prior-p", "0.01"],
                                  ["--enumerate", "3", "--prior-p", "0.01", "--budgets", "10", "20"],
                                  ["--enumerate", "3", "--prior-p", "0.01", "--failures", "x.npz", "--failures-cap", "-1"],
                                  ["--weights", "3", "--prior-p", "0.01", "--failures", "x.npz"],
                                  ["--failures", "x.npz"]])
def test_cli_refuses_bad_enumerate_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--enumerate" in err or "--failures" in err


# ---- 4. the C ABI without a device ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    return _lib.load()


def test_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for name, nargs in (("qbp_mc_run_enum", 15), ("qbp_mc_run_enum_device", 16), ("qbp_mc_sample_errors_enum", 5),
                        ("qbp_enum_count", 3), ("qbp_enum_failures", 19), ("qbp_enum_failures_device", 20)):
        assert f"int {name}(" in header
        assert len(_lib.SIGNATURES[name][1]) == nargs
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") == nargs - 1, name
    assert "itertools.combinations(range(n), w)" in header      # (the order is part of the specification)


def test_null_handle_is_invalid(lib):
    counters = np.full(12, 7, np.int64)
    ranks = np.full(4, 7, np.int64)
    kinds = np.full(4, 7, np.uint8)
    found = np.full(1, 7, np.int64)
    prior = np.zeros(4)
    errors = np.full((2, 4), 7, np.uint8)
    # (h, Lx, k, distance, weight, rank_begin, rank_end, prior, max_iter, variant, alpha, damping, clip_llr, flags,
    #  counters[, stream])
    args = (None, None, 0, 0, 2, 0, 6, prior.ctypes.data, 10, 0, 1.0, 1.0, 20.0, 0, counters.ctypes.data)
    assert lib.qbp_mc_run_enum(*args) == -1
    assert b"null handle" in lib.qbp_last_error()
    assert lib.qbp_mc_run_enum_device(*args, None) == -1
    assert lib.qbp_mc_sample_errors_enum(None, 2, 0, 2, errors.ctypes.data) == -1
    # (h, Lx, k, weight, rank_begin, rank_end, prior, max_iter, variant, alpha, damping, clip_llr, flags, what, cap,
    #  ranks, kinds, found, counters[, stream])
    fargs = (None, None, 1, 2, 0, 6, prior.ctypes.data, 10, 0, 1.0, 1.0, 20.0, 0, 1, 4, ranks.ctypes.data,
             kinds.ctypes.data, found.ctypes.data, counters.ctypes.data)
    assert lib.qbp_enum_failures(*fargs) == -1
    assert b"null handle" in lib.qbp_last_error()
    assert lib.qbp_enum_failures_device(*fargs, None) == -1
    for a in (counters, ranks, kinds, found, errors):
        assert np.all(a == 7)


def test_enum_count_needs_no_device(lib):
    c = np.full(1, -5, np.int64)
    for n, w in ((7, 3), (72, 3), (144, 4), (288, 3), (288, 0), (288, 288), (7776, 5), (62, 31), (0, 0)):
        assert lib.qbp_enum_count(n, w, c.ctypes.data) == 0 and c[0] == math.comb(n, w), (n, w)
    c[0] = -5
    for n, w in ((7776, 6), (288, 40), (288, 144), (7, 8), (7, -1), (-1, 0)):
        assert lib.qbp_enum_count(n, w, c.ctypes.data) == -1, (n, w)
        assert c[0] == -5
    assert lib.qbp_enum_count(7, 3, None) == -1
