"""The host GF(2) layer (qldpc_amd/gf2.py) and the open front door of qldpc_amd/codes.py: css_logicals, bb_code,
from_matrices, register and load_code of registered names and .npz paths.  No GPU."""
import numpy as np
import pytest

import css_oracle as co
from qldpc_amd import codes, gf2, mc

NEW_BB = (6, 6, [(1, 0), (0, 2), (0, 3)], [(0, 1), (2, 0), (3, 0)])        # k = 4; none of the shipped pairs


def mod2(A):
    return np.asarray(A).astype(np.int64) % 2


def check_logicals(Hx, Hz, Lx, Lz, k):
    Hx, Hz = mod2(Hx), mod2(Hz)
    n = Hx.shape[1]
    assert Lx.shape == Lz.shape == (k, n) and Lx.dtype == Lz.dtype == np.uint8
    assert k == n - gf2.rank(Hx) - gf2.rank(Hz)
    assert not (Hz @ mod2(Lx).T % 2).any() and not (Hx @ mod2(Lz).T % 2).any()
    assert np.array_equal(mod2(Lx) @ mod2(Lz).T % 2, np.eye(k, dtype=np.int64))
    # independent modulo the stabilizers
    assert gf2.rank(np.vstack([Hx, Lx])) == gf2.rank(Hx) + k and gf2.rank(np.vstack([Hz, Lz])) == gf2.rank(Hz) + k


# ---- gf2 ---------------------------------------------------------------------------------------------------------------
def test_gf2_on_random_matrices():
    rng = np.random.default_rng(5)
    for m, n in ((1, 1), (3, 7), (7, 3), (20, 37), (33, 64), (64, 65), (40, 40)):
        A = (rng.random((m, n)) < 0.3).astype(np.int64)
        A[m // 2] = A[0]                                 # a dependent row
        rk = gf2.rank(A)
        R, piv = gf2.row_reduce(A)
        N = gf2.nullspace(A)
        assert R.shape == (rk, n) and N.shape == (n - rk, n) and N.dtype == np.uint8
        assert np.all(np.diff(piv) > 0)
        assert np.array_equal(R[:, piv], np.eye(rk, dtype=np.uint8))
        assert gf2.rank(np.vstack([A, R])) == rk                          # the same row space
        assert not (A @ N.T.astype(np.int64) % 2).any() and gf2.rank(N) == n - rk
        # the stated rule: one vector per free column, ascending, the unit vector there
        free = np.setdiff1d(np.arange(n), piv)
        assert np.array_equal(N[:, free], np.eye(len(free), dtype=np.uint8))
        assert np.array_equal(gf2.nullspace(A), N)                        # deterministic


def test_gf2_pivot_rule_by_hand():
    A = np.array([[0, 1, 1, 0], [1, 1, 0, 0], [1, 0, 1, 0]])
    R, piv = gf2.row_reduce(A)
    assert piv.tolist() == [0, 1] and R.tolist() == [[1, 0, 1, 0], [0, 1, 1, 0]]
    assert gf2.nullspace(A).tolist() == [[1, 1, 1, 0], [0, 0, 0, 1]]
    assert gf2.rank(np.zeros((3, 5))) == 0 and gf2.nullspace(np.zeros((0, 3))).tolist() == np.eye(3).tolist()


# ---- css_logicals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", codes.code_names())
def test_css_logicals_span_the_fixture_logicals(name):
    c = codes.load_code(name)
    Lx, Lz = codes.css_logicals(c.Hx, c.Hz)
    k = c.Lx.shape[0]
    check_logicals(c.Hx, c.Hz, Lx, Lz, k)
    for H, new, old in ((c.Hx, Lx, c.Lx), (c.Hz, Lz, c.Lz)):
        H = mod2(H)
        assert gf2.rank(np.vstack([H, new])) == gf2.rank(np.vstack([H, old])) == gf2.rank(np.vstack([H, new, old]))


def test_css_logicals_steane_hgp_and_k0():
    Lx, Lz = codes.css_logicals(codes.STEANE_H, codes.STEANE_H)
    check_logicals(codes.STEANE_H, codes.STEANE_H, Lx, Lz, 1)
    for tag in ("wide_a", "wide_b"):                     # 15 x 47 / 28 x 47 and the reverse
        Hx, Hz, Lx_o, Lz_o = co.hgp_asymmetric(tag)
        Lx, Lz = codes.css_logicals(Hx, Hz)
        check_logicals(Hx, Hz, Lx, Lz, 4)
        assert gf2.rank(np.vstack([Hx, Lx, Lx_o])) == gf2.rank(Hx) + 4
    # k = 0: the [[4, 0]] pair XXXX, ZZII, IIZZ, ZIZI has no logical qubit
    Hx, Hz = np.array([[1, 1, 1, 1]]), np.array([[1, 1, 0, 0], [0, 0, 1, 1], [1, 0, 1, 0]])
    Lx, Lz = codes.css_logicals(Hx, Hz)
    assert Lx.shape == Lz.shape == (0, 4) and Lx.dtype == np.uint8


def test_css_logicals_refuses_a_non_commuting_pair():
    with pytest.raises(ValueError, match="commute"):
        codes.css_logicals(np.array([[1, 1, 0]]), np.array([[1, 0, 0]]))
    with pytest.raises(ValueError):
        codes.css_logicals(np.array([[1, 1, 0]]), np.array([[1, 1]]))


# ---- bb_code, from_matrices, register, load_code -------------------------------------------------------------------------
def test_bb_code_reproduces_bb_matrices():
    name = "[[144, 12, 12]]"
    c = codes.bb_code(*codes.BB_CODES[name])
    Hx, Hz = codes.bb_matrices(name)
    assert np.array_equal(c.Hx, Hx) and np.array_equal(c.Hz, Hz) and c.distance is None
    check_logicals(Hx, Hz, c.Lx, c.Lz, 12)
    assert "l=12" in c.name and codes.bb_code(*codes.BB_CODES[name], name="mine").name == "mine"


def test_register_round_trip_and_npz(tmp_path):
    c = codes.bb_code(*NEW_BB, name="test_codes_cpu bb 6x6")
    assert c.n == 72 and c.Lx.shape == (4, 72) and c.distance is None
    with pytest.raises(KeyError):
        codes.load_code(c.name)
    assert codes.register(c) is c and codes.load_code(c.name) is c
    # the Monte-Carlo entries name distance.estimate instead of failing inside int(None) ...
    for run in (lambda: mc.run_sweep(c.name, [0.01], 10, runner=lambda *a: np.zeros(12, np.int64)),
                lambda: mc.run_weights(c.name, [1], 10, prior_p=0.01), lambda: mc.run_enumerate(c.name, [1], prior_p=0.01),
                lambda: mc.run_budgets(c.name, 0.01, 10, [5]), lambda: mc.run_spectrum(c.name, [0.01], 10),
                lambda: mc.run_llr_hist(c.name, 0.01, 10, [5], 8, (-20.0, 20.0)),
                lambda: mc.run_depolarizing(c.name, [0.01], 10)):
        with pytest.raises(ValueError, match="distance.estimate"):
            run()
    # ... and run once it is set (the object load_code returns is the registered one)
    c.distance = 4
    table = mc.run_sweep(c.name, [0.01], 10, runner=lambda code, p, a, b: np.full(12, code.distance, np.int64))
    assert table.tolist() == [[4] * 12]
    # .npz paths, the reference's layout: with and without logicals and distance
    bare, full = str(tmp_path / "bare.npz"), str(tmp_path / "full.npz")
    np.savez(bare, Hx=c.Hx, Hz=c.Hz)
    np.savez(full, Hx=c.Hx, Hz=c.Hz, Lx=c.Lz, Lz=c.Lx, distance=4)       # (its own logicals, not css_logicals')
    b, f = codes.load_code(bare), codes.load_code(full)
    assert b.name == bare and b.distance is None and np.array_equal(b.Lx, c.Lx) and np.array_equal(b.Lz, c.Lz)
    assert f.distance == 4 and np.array_equal(f.Lx, c.Lz) and np.array_equal(f.Hx, c.Hx) and f.Lx.dtype == np.uint8
    with pytest.raises(ValueError):
        np.savez(str(tmp_path / "half.npz"), Hx=c.Hx)
        codes.load_code(str(tmp_path / "half.npz"))
    # from_matrices with a distance
    d = codes.from_matrices(c.Hx, c.Hz, "test_codes_cpu from_matrices", distance=4)
    assert d.distance == 4 and np.array_equal(d.Lx, c.Lx)


def test_register_refuses_builtin_names():
    c = codes.from_matrices(codes.STEANE_H, codes.STEANE_H, "steane")
    for name in ("steane", "[[72, 12, 6]]", "144"):
        c.name = name
        with pytest.raises(ValueError, match="built-in"):
            codes.register(c)
    c.name = "x.npz"
    with pytest.raises(ValueError):
        codes.register(c)
    with pytest.raises(TypeError):
        codes.register("steane")


def test_builtin_names_load_as_before():
    """Bit for bit what the parent commit's load_code returned: the closed-form matrices (Hx Fortran-ordered), the
    fixture logicals of qldpc_amd/data/logicals.npz, the distance literals; Steane without logicals."""
    with np.load(codes._DATA) as d:
        for name in codes.code_names():
            c = codes.load_code(name)
            Hx, Hz = codes.bb_matrices(name)
            assert c.name == name and c.distance == codes.DISTANCES[name]
            assert np.array_equal(c.Hx, Hx) and np.array_equal(c.Hz, Hz) and c.Hx.dtype == c.Hz.dtype == np.int64
            assert c.Hx.flags.f_contiguous and not c.Hx.flags.c_contiguous
            assert c.Hz.flags.c_contiguous == Hz.flags.c_contiguous        # (Hz: as bb_matrices leaves it)
            k, n = int(d[f"{name}/k"]), Hx.shape[1]
            for got, key in ((c.Lx, "Lx"), (c.Lz, "Lz")):
                assert got.dtype == np.uint8
                assert np.array_equal(got, np.unpackbits(d[f"{name}/{key}"], axis=1)[:k, :n])
    for alias, name in codes.ALIASES.items():
        assert codes.load_code(alias).name == name
    s = codes.load_code("steane")
    assert s.Lx is None and s.Lz is None and s.distance is None
    assert np.array_equal(s.Hx, codes.STEANE_H) and np.array_equal(s.Hz, codes.STEANE_H)
