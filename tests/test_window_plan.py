"""CPU: qbp_window_plan against the numpy statement of the window partition (tests/window_oracle.py), the properties of
the partition, every QBP_E_INVALID case, and the statement itself run with the CPU oracle -- W >= R is the plain decode,
and H x == s exactly where `converged` says so."""
import numpy as np
import pytest

import window_oracle as wo
from oracle import oracle
from qldpc_amd import _lib, bp, codes

MATRICES = ["steane", "72", "irregular"]
P_OF = {"steane": 0.04, "72": 0.02, "irregular": 0.04}


def matrix(name):
    if name == "irregular":
        return wo.irregular()
    return wo.spacetime(codes.load_code({"steane": "steane", "72": "[[72, 12, 6]]"}[name]).Hx, 6)


def window_sizes(R):
    return [(3, 1), (4, 2), (2, 2), (R, R), (R + 3, 1)]


def test_matrices_are_what_the_tests_need():
    for name, shape in (("steane", (18, 60)), ("72", (216, 648)), ("irregular", (24, 50))):
        assert matrix(name)[0].shape == shape
    H, cr = wo.irregular()
    assert int(cr.max()) + 1 == 6 and 2 not in cr and not np.array_equal(cr, np.sort(cr))
    P = wo.plan(H, cr, 3, 1)
    span = [len(set(cr[H[:, v] != 0])) for v in range(50)]
    assert max(span) == 3 and (H.sum(axis=0) == 0).sum() == 1
    commits = [int(P["commit"][a:b].sum()) for a, b in zip(P["var_ptr"][:-1], P["var_ptr"][1:])]
    assert 0 in commits                                        # a window whose commit set is empty


@pytest.mark.parametrize("name", MATRICES)
def test_plan_equals_statement(name):
    H, cr = matrix(name)
    R = int(cr.max()) + 1
    rp, ci, m, n = bp.csr_from_H(H)
    for W, F in window_sizes(R):
        got = _lib.window_plan(rp, ci, m, n, cr, W, F)
        want = wo.plan(H, cr, W, F)
        for key in ("K", "check_ptr", "checks", "var_ptr", "vars", "commit", "cls"):
            assert np.array_equal(got[key], want[key]), (name, W, F, key)
        # every variable is committed exactly once: the M_k partition the columns
        committed = got["vars"][got["commit"] != 0]
        assert np.array_equal(np.sort(committed), np.arange(n)), (name, W, F)
        for k in range(got["K"]):
            for ptr, arr in (("check_ptr", "checks"), ("var_ptr", "vars")):
                part = got[arr][got[ptr][k]:got[ptr][k + 1]]
                assert np.all(np.diff(part) > 0)
        if name != "irregular":
            classes = int(got["cls"].max()) + 1
            assert classes == (2 if W < R and (R - W) % F else 1), (name, W, F, got["cls"])
            assert np.array_equal(got["cls"][:-1], np.zeros(got["K"] - 1, np.int32))


def test_plan_refuses():
    H, cr = matrix("steane")
    rp, ci, m, n = bp.csr_from_H(H)
    lib = _lib.load()
    sizes = np.zeros(3, np.int32)

    def call(rp_=rp, ci_=ci, cr_=cr, W=3, F=1, sizes_=sizes, m_=m, n_=n):
        return lib.qbp_window_plan(_lib._ptr(rp_), _lib._ptr(ci_), m_, n_, _lib._ptr(cr_), W, F, _lib._ptr(sizes_),
                                   None, None, None, None, None, None)
    assert call() == 0
    bad_round = cr.copy()
    bad_round[5] = -1
    bad_ptr = rp.copy()
    bad_ptr[3] = bad_ptr[2] - 1
    bad_col = ci.copy()
    bad_col[0] = n
    unsorted = ci.copy()
    unsorted[[0, 1]] = unsorted[[1, 0]]
    for kwargs in (dict(rp_=None), dict(ci_=None), dict(cr_=None), dict(sizes_=None), dict(cr_=bad_round),
                   dict(rp_=bad_ptr), dict(ci_=bad_col), dict(ci_=unsorted), dict(W=0), dict(W=-1), dict(F=0),
                   dict(W=3, F=4), dict(m_=0)):
        assert call(**kwargs) == _lib.E_INVALID, kwargs
        assert lib.qbp_last_error()
    with pytest.raises(_lib.QbpError):
        _lib.window_plan(rp, ci, m, n, cr, 2, 3)


@pytest.mark.parametrize("name", MATRICES)
def test_statement_on_the_cpu(name):
    H, cr = matrix(name)
    R = int(cr.max()) + 1
    p = P_OF[name]
    B = 48 if name == "72" else 96
    errors = (np.random.default_rng(11).random((B, H.shape[1])) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(H.shape[1], np.log((1 - p) / p))
    for variant in (_lib.SUM_PRODUCT, _lib.MIN_SUM):
        def decode(Hk, s, pr):
            return oracle.decode_batch(Hk, s, pr, 8, variant, 0.9, 0.75, 20.0)

        def osd(Hk, s, llr, hard):
            return np.array([oracle.osd0(Hk, s[i], llr[i], hard[i]) for i in range(s.shape[0])], np.uint8)
        whole = decode(H, syn, prior)
        for W, F in window_sizes(R):
            for second in (None, osd):
                x, conv, iters, llr, fails = wo.decode(H, cr, W, F, syn, prior, decode, second)
                valid = ~((x.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8) ^ syn).any(axis=1)
                assert np.array_equal(valid, conv), (name, variant, W, F)
                assert np.all(conv[fails == 0])
                if W >= R and second is None:
                    assert np.array_equal(x, whole[0]) and np.array_equal(conv, whole[1])
                    assert np.array_equal(iters, whole[2]) and np.array_equal(llr, whole[3], equal_nan=True)


def shifted_irregular():
    """The irregular matrix with every round one later: round 0 has no check, so window 0 of (1, 1) holds nothing but
    the empty column -- a skipped window that still commits a variable."""
    H, cr = wo.irregular()
    return H, (cr + 1).astype(np.int32)


@pytest.mark.parametrize("make", [wo.irregular, shifted_irregular])
def test_windows_without_checks_are_skipped(make):
    H, cr = make()
    rp, ci, m, n = bp.csr_from_H(H)
    R = int(cr.max()) + 1
    for W, F in ((1, 1), (2, 1), (2, 2)):
        got = _lib.window_plan(rp, ci, m, n, cr, W, F)
        want = wo.plan(H, cr, W, F)
        for key in ("K", "check_ptr", "checks", "var_ptr", "vars", "commit", "cls"):
            assert np.array_equal(got[key], want[key]), (W, F, key)
        assert np.array_equal(np.sort(got["vars"][got["commit"] != 0]), np.arange(n))
    one = _lib.window_plan(rp, ci, m, n, cr, 1, 1)
    assert one["K"] == R and -1 in one["cls"]
    # the statement on it: nothing decoded in a skipped window, H x == s where converged says so
    p = P_OF["irregular"]
    errors = (np.random.default_rng(4).random((64, n)) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.linspace(1.0, 4.0, n)
    x, conv, iters, llr, fails = wo.decode(H, cr, 1, 1, syn, prior,
                                           lambda Hk, s, pr: oracle.decode_batch(Hk, s, pr, 8, 0, 1.0, 1.0, 20.0))
    assert np.array_equal(~((x.astype(np.int64) @ H.T % 2).astype(np.uint8) ^ syn).any(axis=1), conv)
    assert (x[:, 49] == 0).all() and (llr[:, 49] == prior[49]).all()


def test_plan_bounds_the_rounds():
    """Rounds need not be contiguous: a large round number costs nothing, and beyond 2^20 it is refused at once."""
    rp, ci = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    far = _lib.window_plan(rp, ci, 2, 2, np.array([0, (1 << 20) - 1], np.int32), 3, 2)
    assert far["K"] == ((1 << 20) - 3 + 1) // 2 + 1 and far["checks"].tolist() == [0, 1]
    assert (far["cls"] >= 0).sum() == 2 and np.array_equal(np.sort(far["vars"][far["commit"] != 0]), [0, 1])
    for big in (1 << 20, np.iinfo(np.int32).max):
        with pytest.raises(_lib.QbpError) as e:
            _lib.window_plan(rp, ci, 2, 2, np.array([0, big], np.int32), 3, 2)
        assert e.value.code == _lib.E_INVALID


def test_run_dem_passes_the_window_to_a_runner():
    from qldpc_amd import mc
    H, cr = matrix("steane")
    L = np.ones((1, H.shape[1]), np.uint8)
    seen = {}

    def runner(H_, L_, probs, prior, begin, end, **kw):
        seen.update(kw, begin=begin, end=end)
        return np.arange(12)
    out = mc.run_dem(H, L, np.full(H.shape[1], 0.01), 100, window=(3, 1), check_round=cr, runner=runner, rank=1, world=2)
    assert seen["window"] == (3, 1) and np.array_equal(seen["check_round"], cr) and (seen["begin"], seen["end"]) == (50, 100)
    assert np.array_equal(out, np.arange(12))
    seen.clear()
    mc.run_dem(H, L, np.full(H.shape[1], 0.01), 100, runner=lambda *a: np.zeros(12))      # (the plain path: six arguments)
    with pytest.raises(ValueError):
        mc.run_dem(H, L, np.full(H.shape[1], 0.01), 100, window=(3, 1), runner=runner)
    with pytest.raises(ValueError):
        mc.run_dem(H, L, np.full(H.shape[1], 0.01), 100, window=(3, 1), check_round=cr, layered=True, runner=runner)


CLI = ["--phenomenological", "[[72, 12, 6]]", "6", "--p", "0.02", "--trials", "10"]


@pytest.mark.parametrize("argv", [
    ["--window", "3", "1"],                                             # no --phenomenological
    ["--dem", "x.dem", "--window", "3", "1"],
    CLI + ["--window", "3", "1", "--relay", "2", "5"],
    CLI + ["--window", "3", "1", "--gd", "5", "2"],
    CLI + ["--window", "3", "1", "--layered"],
    CLI + ["--window", "3", "1", "--budgets", "5", "10"],
    CLI + ["--window", "3", "1", "--spectrum", "out.npz"],
    CLI + ["--window", "3", "1", "--weights", "2", "--prior-p", "0.01"],
    CLI + ["--window", "3", "1", "--shots", "x.b8"],
    CLI + ["--window", "0", "1"],
    CLI + ["--window", "3", "4"],
    CLI + ["--window", "3"],
    CLI + ["--p", "0.01", "0.02"],                                      # one --p
    ["--phenomenological", "[[72, 12, 6]]", "six"],
    ["--phenomenological", "[[72, 12, 6]]", "0", "--p", "0.01"],
    ["--phenomenological", "no such code", "6", "--p", "0.01"],
    ["--phenomenological", "steane", "6", "--p", "0.01"],                # (no logical operators)
])
def test_cli_refuses(argv, capsys):
    from qldpc_amd import mc
    with pytest.raises(SystemExit) as e:
        mc.main(argv)
    assert e.value.code == 2 and "error" in capsys.readouterr().err
