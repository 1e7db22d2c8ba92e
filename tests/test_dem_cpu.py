"""Detector error models without a GPU: the DEM parser, the phenomenological model, the numpy statement of the
per-column sampler (against the oracle's uniform sampler) and the sharding / prior of mc.run_dem."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dem_sampler import errors_probs, thresholds
from oracle import oracle
from qldpc_amd import codes, dem, mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense(H):
    return np.asarray(H.toarray(), np.uint8)


def test_parse_basic_and_hyperedge():
    H, L, p = dem.parse_dem("""
        # comment line
        error(0.125) D0 D2 L0   # trailing comment
        error(0.25) D1 ^ D2 D3 ^ L1
        detector(0, 1, 2) D4
        logical_observable L2
    """)
    assert H.dtype == np.uint8 and L.dtype == np.uint8 and p.dtype == np.float64
    assert H.shape == (5, 2) and L.shape == (3, 2)
    assert dense(H)[:, 0].tolist() == [1, 0, 1, 0, 0]
    assert dense(H)[:, 1].tolist() == [0, 1, 1, 1, 0]
    assert L[:, 0].tolist() == [1, 0, 0] and L[:, 1].tolist() == [0, 1, 0]
    assert p.tolist() == [0.125, 0.25]


def test_caret_is_symmetric_difference():
    H, L, p = dem.parse_dem("error(0.1) D0 D1 ^ D1 D2 ^ L0 ^ L0 D3")
    assert dense(H)[:, 0].tolist() == [1, 0, 1, 1] and L.shape == (1, 1) and L[0, 0] == 0


def test_merge_rule_and_first_appearance_order():
    H, L, p = dem.parse_dem("""
        error(0.1) D1
        error(0.2) D0 L0
        error(0.3) D1
        error(0.4) L0 D0
        error(0.05) D1 ^ D0 ^ D0
    """)
    assert H.shape == (2, 2)
    assert dense(H).tolist() == [[0, 1], [1, 0]]
    q = 0.1 + 0.3 - 2 * 0.1 * 0.3
    q = q + 0.05 - 2 * q * 0.05
    assert p[0] == pytest.approx(q, abs=0, rel=1e-15)
    assert p[1] == pytest.approx(0.2 + 0.4 - 2 * 0.2 * 0.4, abs=0, rel=1e-15)
    assert L.tolist() == [[0, 1]]


def test_observable_only_kept_and_empty_dropped():
    H, L, p = dem.parse_dem("""
        error(0.1) D0
        error(0.01) L0
        error(0.2) D1 ^ D1
        error(0.3) L1 ^ L1
        error(0.02) L0
    """)
    assert H.shape == (2, 2)       # D1 declared by use, its only mechanism cancels
    assert dense(H)[:, 1].tolist() == [0, 0]
    assert L.tolist() == [[0, 1], [0, 0]]
    assert p[1] == pytest.approx(0.01 + 0.02 - 2 * 0.01 * 0.02)


def test_repeat_and_shift_nesting():
    text = """
        error(0.1) D0
        repeat 2 {
            error(0.2) D0 D1
            repeat 3 {
                error(0.3) D1 L0
                shift_detectors 1
            }
            shift_detectors(0, 0, 1) 2
        }
        detector D0
    """
    H, L, p = dem.parse_dem(text)
    # offsets: outer pass 0 starts at 0, inner shifts 0,1,2 -> 3, then +2 -> 5; pass 1 starts at 5 -> 8 -> 10
    cols = [(tuple(np.flatnonzero(c)), tuple(np.flatnonzero(l))) for c, l in zip(dense(H).T, L.T)]
    assert cols == [((0,), ()), ((0, 1), ()), ((1,), (0,)), ((2,), (0,)), ((3,), (0,)),
                    ((5, 6), ()), ((6,), (0,)), ((7,), (0,)), ((8,), (0,))]
    assert H.shape[0] == 11      # detector D0 after the shifts is D10
    assert np.allclose(p, [0.1, 0.2, 0.3, 0.3, 0.3, 0.2, 0.3, 0.3, 0.3])


def test_declared_unused_detectors_count():
    H, L, p = dem.parse_dem("detector(1, 2) D7\nerror(0.5) D0\nlogical_observable L3")
    assert H.shape == (8, 1) and L.shape == (4, 1) and dense(H)[1:].sum() == 0


@pytest.mark.parametrize("text", [
    "error(0.1) D0 X3",
    "error(0.1) D-1",
    "error(1.5) D0",
    "error(-0.1) D0",
    "error(abc) D0",
    "error D0",
    "error(0.1) ^ D0",
    "error(0.1) D0 ^",
    "error(0.1) D0 ^ ^ D1",
    "detector(0) X0",
    "shift_detectors",
    "shift_detectors -1",
    "repeat 3 {\nerror(0.1) D0",
    "error(0.1) D0\n}",
    "repeat {\n}",
    "repeat 2\nerror(0.1) D0",
    "detector_separator 1",
    "mystery(0.1) D0",
    "!!",
])
def test_malformed_raises_naming_the_line(text):
    with pytest.raises(ValueError, match="DEM"):
        dem.parse_dem("error(0.01) D5\n" + text)


def test_error_names_line_number():
    with pytest.raises(ValueError, match="line 3"):
        dem.parse_dem("error(0.1) D0\n# fine\nbogus D1\n")


def test_load_dem_path_string_and_object(tmp_path):
    text = "error(0.1) D0 L0\nrepeat 2 {\n error(0.2) D0 D1\n shift_detectors 1\n}\n"
    f = tmp_path / "m.dem"
    f.write_text(text)

    class Model:                 # e.g. stim.DetectorErrorModel: str() is the text
        def __str__(self):
            return text

    ref = dem.parse_dem(text)
    for x in (str(f), f, text, Model()):
        H, L, p = dem.load_dem(x)
        assert (H != ref[0]).nnz == 0 and np.array_equal(L, ref[1]) and np.array_equal(p, ref[2])


def spacetime_kron(H, T):
    """spaceTime.py:4-18 as written there (dense np.kron / np.eye)."""
    m, n = H.shape
    spatial = np.kron(np.eye(T), H)
    temporal = (np.eye(m * T) + np.eye(m * T, k=-m)) % 2
    return np.hstack([spatial, temporal]).astype(np.uint8)


@pytest.mark.parametrize("name,T", [("[[72, 12, 6]]", 1), ("[[72, 12, 6]]", 5), ("[[144, 12, 12]]", 12)])
def test_phenomenological_matches_kron(name, T):
    code = codes.load_code(name)
    H, L, p = dem.phenomenological(code, T, 0.01, 0.03)
    assert H.dtype == np.uint8
    assert np.array_equal(dense(H), spacetime_kron(code.Hx, T))
    n, mx = code.n, code.Hx.shape[0]
    assert np.array_equal(L, np.hstack([np.tile(code.Lx, (1, T)), np.zeros((code.Lx.shape[0], mx * T), np.uint8)]))
    assert np.array_equal(p, np.r_[np.full(n * T, 0.01), np.full(mx * T, 0.03)])
    H2, L2, p2 = dem.phenomenological(name, T, 0.02)
    assert (H2 != H).nnz == 0 and np.array_equal(L2, L) and np.all(p2 == 0.02)


@pytest.mark.parametrize("n,p,draws,seed,begin", [(7, 0.3, 1, 0, 0), (144, 0.05, 2, 99, 1 << 33),
                                                  (13, 0.5, 1, 12345678901, 17), (10, 2.0 ** -30, 2, 1, 5)])
def test_numpy_sampler_equals_oracle_uniform(n, p, draws, seed, begin):
    T = 64
    ours = errors_probs(np.full(n, p), draws, seed, begin, T)
    assert np.array_equal(ours, oracle.mc_errors(n, p, draws, seed, begin, T))


def test_thresholds_rule():
    assert thresholds([0.0, 1.0, 0.5, 2.0 ** -32, 2.0 ** -33]).tolist() == [0, 2 ** 32 - 1, 2 ** 31, 1, 0]


def test_numpy_sampler_per_column():
    probs = np.array([0.0, 1.0, 0.0, 1.0, 0.5])
    e = errors_probs(probs, 1, 3, 0, 200)
    assert not e[:, 0].any() and not e[:, 2].any() and e[:, 1].all() and e[:, 3].all()
    assert 50 < e[:, 4].sum() < 150
    assert not errors_probs(probs, 2, 3, 0, 20)[:, 1].any()     # two draws of p = 1 cancel


def test_run_dem_shards_tile_and_prior_clipped():
    H, L, probs = dem.parse_dem("error(0) D0 L0\nerror(1) D0 D1\nerror(0.25) D1\nerror(0.5) L1")
    seen = []

    def runner(H_, L_, probs_, prior, begin, end):
        seen.append((begin, end))
        assert np.array_equal(probs_, probs) and np.array_equal(L_, L)
        assert np.all(np.isfinite(prior))
        lo, hi = 1e-15, 1 - 1e-15                       # studyComplete.py:85-86
        assert prior[0] == np.log((1 - lo) / lo) and prior[1] == np.log((1 - hi) / hi)
        assert prior[2] == pytest.approx(np.log(3.0)) and prior[3] == 0.0
        out = np.zeros(12, np.int64)
        out[0] = end - begin
        out[7] = begin
        return out

    totals = [mc.run_dem(H, L, probs, 1001, rank=r, world=7, runner=runner) for r in range(7)]
    assert sorted(seen) == [mc.shard_range(1001, r, 7) for r in range(7)]
    assert seen[0][0] == 0 and seen[-1][1] == 1001
    assert sum(t[0] for t in totals) == 1001
    got = mc.run_dem(H, L, probs, 10, runner=runner, all_reduce=lambda c: c * 3)
    assert got[0] == 30
    custom = np.arange(4.0)
    mc.run_dem(H, L, probs, 4, prior=custom,
               runner=lambda *a: (np.testing.assert_array_equal(a[3], custom), np.zeros(12, np.int64))[1])


def test_run_dem_rejects_bad_shapes():
    H, L, probs = dem.parse_dem("error(0.1) D0 L0")
    run = lambda *a, **k: np.zeros(12, np.int64)   # noqa: E731
    with pytest.raises(ValueError, match="64"):
        mc.run_dem(H, np.zeros((65, 1), np.uint8), probs, 10, runner=run)
    with pytest.raises(ValueError):
        mc.run_dem(H, L, np.zeros(2), 10, runner=run)
    with pytest.raises(ValueError):
        mc.run_dem(H, L, probs, 10, prior=np.zeros(3), runner=run)
    with pytest.raises(ValueError):
        mc.run_dem(H, L, probs, 10, osd=False, osd_order=3, runner=run)


def test_cli_rejects_bad_dem_file(tmp_path):
    bad = tmp_path / "bad.dem"
    bad.write_text("error(0.1) D0\nnot_an_instruction D1\n")
    for arg in (str(bad), str(tmp_path / "missing.dem")):
        r = subprocess.run([sys.executable, "-m", "qldpc_amd.mc", "--dem", arg, "--trials", "10"], cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--dem" in r.stderr
