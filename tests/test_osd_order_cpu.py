"""CPU: the numpy statement of order-w OSD (tests/osd_order_oracle.py) against OSD-0, a brute-force search and
hand-built selection cases; the flag encoding of _lib against include/qbp.h; argument checks of the drivers."""
import itertools
import os
import re

import numpy as np
import pytest

import osd_order_oracle as ordo
from oracle import oracle
from qldpc_amd import _lib, mc, paper_results
from test_oracle_osd import TAGS, load_osd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("cs", 1), ("cs", 2), ("cs", 7), ("cs", 64), ("e", 1), ("e", 4), ("e", 8)]


def seq_cost(x, llr):
    c = 0.0
    for i in range(len(x)):             # ascending column, left to right
        if x[i]:
            c += abs(float(llr[i]))
    return c


@pytest.mark.parametrize("tag", TAGS)
def test_order0_is_osd0(tag):
    c = load_osd(tag)
    H = c["H"].astype(np.int64)
    for s, l, h, want in zip(c["syndromes"], c["llr"], c["hard"], c["solution"]):
        red = ordo.reduce(H, s, l, h)
        assert red.consistent
        assert np.array_equal(red.x0, oracle.osd0(H, s, l, h))
        assert np.array_equal(red.x0, want)
        for method in ("cs", "e"):
            assert np.array_equal(ordo.osd_order(H, s, l, h, 0, method, red=red), want)


@pytest.mark.parametrize("tag", ("steane", "72"))
def test_choice_is_the_brute_force_minimum(tag):
    c = load_osd(tag)
    H = c["H"].astype(np.int64)
    n = H.shape[1]
    for s, l, h in zip(c["syndromes"], c["llr"], c["hard"]):
        red = ordo.reduce(H, s, l, h)
        kp = len(red.T)
        assert kp + len(red.S) == n
        for method, w in CONFIGS:
            wp = min(w, kp)
            sets = ordo.flip_sets(method, w, kp)
            if method == "cs":
                assert len(sets) == kp + wp * (wp - 1) // 2
            else:
                assert len(sets) == 2 ** wp - 1
                assert [len(F) for F in sets] == sorted(len(F) for F in sets)
            X = ordo.candidates(red, method, w)
            assert np.array_equal(X[0], red.x0)
            best, best_cost = 0, seq_cost(X[0], l)
            for i, x in enumerate(X):
                assert np.array_equal((x.astype(np.int64) @ H.T) % 2, s)       # every candidate is a solution
                if i:
                    flipped = np.flatnonzero(x[red.T] ^ red.x0[red.T])
                    assert tuple(flipped) == sets[i - 1]                       # flips exactly F within T
                cost = seq_cost(x, l)
                vec = ordo.costs(x[None, :], np.abs(l))[0]
                assert cost == vec or (np.isnan(cost) and np.isnan(vec))
                if cost < best_cost:                                           # the sequential rule
                    best, best_cost = i, cost
            got = ordo.osd_order(H, s, l, h, w, method, red=red)
            assert np.array_equal(got, X[best])
            assert seq_cost(got, l) <= seq_cost(red.x0, l)


def test_selection_rule():
    nan, inf = float("nan"), float("inf")
    assert ordo.select(np.array([nan, 1.0, 0.0])) == 0                  # OSD-0 NaN: OSD-0
    assert ordo.select(np.array([3.0, nan, 2.0, 2.0])) == 2             # NaN never wins; ties: lowest index
    assert ordo.select(np.array([inf, inf, inf])) == 0                  # inf ties
    assert ordo.select(np.array([inf, nan, 7.0])) == 2
    assert ordo.select(np.array([5.0, 5.0, nan, 4.0, 4.0])) == 3
    assert ordo.select(np.array([0.0, 0.0])) == 0


def _steane():
    from qldpc_amd import codes
    return codes.load_code("steane").Hx.astype(np.int64)


def test_hand_built_records():
    H = _steane()
    n = H.shape[1]
    e = np.zeros(n, np.uint8); e[[0, 1]] = 1
    s = (e.astype(np.int64) @ H.T) % 2
    hard = np.zeros(n, np.uint8)
    # all |llr| NaN: every cost is NaN -> OSD-0
    l = np.full(n, np.nan)
    red = ordo.reduce(H, s, l, hard)
    for method, w in CONFIGS:
        assert np.array_equal(ordo.osd_order(H, s, l, hard, w, method), red.x0)
    # equal reliabilities: the weight-minimal solution of lowest index wins
    l = np.ones(n)
    for method, w in (("cs", 7), ("e", 4)):
        got = ordo.osd_order(H, s, l, hard, w, method)
        assert np.array_equal((got.astype(np.int64) @ H.T) % 2, s)
        assert got.sum() <= ordo.reduce(H, s, l, hard).x0.sum()
    # a NaN in one column: candidates through it are NaN and never win
    l = np.linspace(1.0, 2.0, n); l[3] = np.nan
    red = ordo.reduce(H, s, l, hard)
    X = ordo.candidates(red, "e", 4)
    c = ordo.costs(X, red.absl)
    got = ordo.osd_order(H, s, l, hard, 4, "e")
    if np.isnan(c[0]):
        assert np.array_equal(got, red.x0)
    else:
        assert not np.isnan(seq_cost(got, l)) and got[3] == 0
    # +-inf and +-0.0
    l = np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 2.0])
    red = ordo.reduce(H, s, l, hard)
    X = ordo.candidates(red, "e", 4)
    c = ordo.costs(X, red.absl)
    assert not np.isnan(c).any() and ordo.select(c) == int(np.flatnonzero(c == c.min())[0])


def test_flag_encoding_equals_the_header():
    text = open(os.path.join(ROOT, "include", "qbp.h")).read()
    enum = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"\b(QBP_[A-Z0-9_]+)\s*=\s*(-?(?:0x[0-9a-fA-F]+|\d+)u?)", text)}
    assert _lib.FLAG_OSD_CS == enum["QBP_FLAG_OSD_CS"] and _lib.FLAG_OSD_E == enum["QBP_FLAG_OSD_E"]
    m = re.search(r"#define\s+QBP_OSD_ORDER_FLAGS\(w\)\s+\(\(uint32_t\)\(w\)\s*<<\s*(\d+)\)", text)
    assert m and int(m.group(1)) == _lib.OSD_ORDER_SHIFT == 16
    # the order field does not overlap any flag bit
    assert all(v < (1 << _lib.OSD_ORDER_SHIFT) for k, v in enum.items() if k.startswith("QBP_FLAG_"))
    assert _lib.osd_flags("cs", 0) == _lib.FLAG_OSD0
    assert _lib.osd_flags("cs", 7) == _lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | (7 << 16)
    assert _lib.osd_flags("e", 12) == _lib.FLAG_OSD0 | _lib.FLAG_OSD_E | (12 << 16)
    assert _lib.osd_flags("CS", 64) == _lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | (64 << 16)
    for method, w in (("cs", 65), ("e", 13), ("cs", -1), ("x", 3), ("e", 2.5), ("cs", True)):
        with pytest.raises(ValueError):
            _lib.osd_flags(method, w)


def test_run_sweep_rejects_bad_osd_arguments():
    calls = []

    def runner(code, p, begin, end):
        calls.append((p, begin, end))
        return np.zeros(_lib.NUM_COUNTERS, np.int64)

    for kw in (dict(osd=False, osd_order=7), dict(osd=True, osd_method="x", osd_order=3),
               dict(osd=True, osd_method="cs", osd_order=65), dict(osd=True, osd_method="e", osd_order=13),
               dict(osd=True, osd_order=-1)):
        with pytest.raises(ValueError):
            mc.run_sweep("[[72, 12, 6]]", [0.05], 100, runner=runner, **kw)
    assert calls == []
    for kw in (dict(osd=True, osd_method="cs", osd_order=7), dict(osd=True, osd_method="e", osd_order=8),
               dict(osd=True), dict(osd=False)):
        mc.run_sweep("[[72, 12, 6]]", [0.05], 100, runner=runner, **kw)
    assert len(calls) == 4
    assert mc.osd_run_flags(True, "e", 8) == _lib.osd_flags("e", 8)
    assert mc.osd_run_flags(True) == _lib.FLAG_OSD0 and mc.osd_run_flags(False) == 0


@pytest.mark.parametrize("argv", [["--osd-order", "7"], ["--osd", "--osd-method", "e", "--osd-order", "13"],
                                  ["--osd", "--osd-order", "65"], ["--osd", "--osd-method", "x", "--osd-order", "2"]])
def test_mc_cli_rejects_bad_osd_arguments(argv):
    with pytest.raises(SystemExit) as e:
        mc.main(argv)
    assert e.value.code == 2


@pytest.mark.parametrize("argv", [["--osd", "-1", "--osd-order", "7"], ["--osd-method", "e", "--osd-order", "13"],
                                  ["--osd-order", "0", "--osd-method", "y"], ["--osd-order", "99"]])
def test_paper_results_cli_rejects_bad_osd_arguments(argv):
    with pytest.raises(SystemExit) as e:
        paper_results.main(argv)
    assert e.value.code == 2


def test_flip_set_enumeration_order():
    assert ordo.flip_sets("cs", 3, 5) == [(0,), (1,), (2,), (3,), (4,), (0, 1), (0, 2), (1, 2)]
    assert ordo.flip_sets("e", 3, 5) == [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
    assert ordo.flip_sets("e", 9, 2) == [(0,), (1,), (0, 1)]
    assert ordo.flip_sets("cs", 64, 3) == [(0,), (1,), (2,)] + list(itertools.combinations(range(3), 2))
