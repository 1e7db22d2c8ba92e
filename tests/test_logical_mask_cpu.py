"""CPU: the inputs of tests/test_gpu_logical_mask.py -- the placements are what tests/logical_mask_util.py says, the
oracle's classification has the property the GPU tests ask of the kernels, and a fold that lost bits 32 .. 63 of the
logical mask would not have it on these inputs."""
import numpy as np
import pytest

import logical_mask_util as lm
from oracle import oracle
from qldpc_amd import shots

MATRICES = {"72": lm.code72, "irregular": lm.irregular}


_RUNS = {}


def run(name, L):
    """oracle.mc_counters at the inputs of the GPU tests, BP only; computed once per (matrix, L)."""
    L = np.ascontiguousarray(L, np.uint8)
    key = (name, L.shape, L.tobytes())
    if key not in _RUNS:
        H, _, d = MATRICES[name]()
        _RUNS[key] = oracle.mc_counters(H, L, d, lm.P, lm.prior_of(H.shape[1]), 0, lm.TRIALS, seed=lm.SEED,
                                        max_iter=lm.MAX_ITER)
    return _RUNS[key]


def test_placements_are_what_they_say():
    _, L, _ = lm.code72()
    got = {name: (Lp, m) for name, Lp, m in lm.placements(L)}
    assert list(got) == ["top", "straddle", "spread", "k33"] + [f"single({r},{b})" for b in (31, 32, 63) for r in (0, 1)]
    want_maps = {"top": np.arange(52, 64), "straddle": np.arange(26, 38), "spread": 5 * np.arange(12) + 4}
    for name, (Lp, m) in got.items():
        assert Lp.dtype == np.uint8 and Lp.shape == ((33 if name == "k33" else 64), 72) and m.shape == (12,)
        on = m >= 0
        assert np.array_equal(Lp[m[on]], L[on]), name                 # the rows of L' under map are those of L
        rest = np.setdiff1d(np.arange(Lp.shape[0]), m[on])
        assert not Lp[rest].any(), name                               # and every other row is zero
        assert np.array_equal(lm.kept(L, m), L[on])
        if name in want_maps:
            assert np.array_equal(m, want_maps[name])
    assert got["straddle"][1].min() < 32 <= got["straddle"][1].max()   # it crosses the 31 / 32 boundary
    assert got["spread"][1].max() == 59 and (got["spread"][1] >= 32).sum() == 6
    assert got["k33"][1].tolist() == [32] + [-1] * 11 and not got["k33"][0][:32].any()
    for b in lm.SINGLE_BITS:
        for r in lm.SINGLE_ROWS:
            Lp, m = got[f"single({r},{b})"]
            assert m[r] == b and (np.delete(m, r) == -1).all() and np.flatnonzero(Lp.any(axis=1)).tolist() == [b]
    x = lm.extra_row(L)
    assert x.shape == (13, 72) and x[:12].tobytes() == np.ascontiguousarray(L).tobytes() and x[12].any()


def test_masks_round_trip_through_bit_63():
    rng = np.random.default_rng(63)
    obs = (rng.random((257, 64)) < 0.5).astype(np.uint8)
    obs[0], obs[1], obs[2, :63], obs[2, 63] = 0, 1, 0, 1
    masks = shots.masks_of(obs)
    assert masks.dtype == np.uint64 and masks[0] == 0 and masks[1] == np.uint64(2 ** 64 - 1) and masks[2] == np.uint64(1 << 63)
    assert np.array_equal(shots.obs_of(masks, 64), obs)
    assert np.array_equal(shots.obs_of(masks, 33)[:, 32], obs[:, 32])
    # move_bits is masks_of on the moved columns
    _, L, _ = lm.code72()
    base = (rng.random((257, 12)) < 0.5).astype(np.uint8)
    for name, Lp, m in lm.placements(L):
        moved = np.zeros((257, Lp.shape[0]), np.uint8)
        moved[:, m[m >= 0]] = base[:, m >= 0]
        assert np.array_equal(lm.move_bits(shots.masks_of(base), m), shots.masks_of(moved)), name
        errors = (rng.random((64, 72)) < 0.1).astype(np.int64)
        assert np.array_equal(shots.masks_of(errors @ Lp.T.astype(np.int64) % 2),
                              lm.move_bits(shots.masks_of(errors @ L.T.astype(np.int64) % 2), m)), name


def test_issue_table_on_72():
    """The figures the GPU tests' floors rest on: BP(8) at p = 0.06, 1500 trials, seed 3."""
    _, L, _ = lm.code72()
    base = run("72", L)
    assert [int(base[i]) for i in (0, 1, 5, 6, 8)] == [1500, 475, 10, 380, 368]
    assert [int(run("72", lm.single(L, r, 63)[1])[1]) for r in (0, 1, 2)] == [206, 190, 248]
    none = run("72", np.zeros((0, 72), np.uint8))
    assert none[1] == 0 and none[5] == 117


@pytest.mark.parametrize("name", list(MATRICES))
def test_oracle_has_the_property_and_the_inputs_discriminate(name):
    H, L, d = MATRICES[name]()
    n = H.shape[1]
    base = run(name, L)
    print(name, "base", base.tolist())
    assert base[0] == lm.TRIALS and base[1] >= 8 and base[6] >= 8 and base[8] >= 8
    ones = {r: run(name, L[r:r + 1]) for r in lm.SINGLE_ROWS}
    for name_p, Lp, m in lm.placements(L):
        got = run(name, Lp)
        want = run(name, lm.kept(L, m))
        assert np.array_equal(got, want), (name, name_p, got, want)
        if (m >= 0).sum() == 1:
            r = int(np.flatnonzero(m >= 0)[0])
            assert np.array_equal(got, ones[r]) and not np.array_equal(got, base), (name, name_p)
        else:
            assert np.array_equal(got, base), (name, name_p)
        # a fold that dropped bits 32 .. 63 classifies with rows 32 .. 63 zeroed
        low = run(name, lm.low_half(Lp))
        print(name, name_p, "[1]", int(got[1]), "with bits 32..63 lost", int(low[1]))
        if name_p.startswith("single") and m.max() == 31:
            assert np.array_equal(low, got)                          # (nothing above bit 31 to lose)
        elif name_p == "spread":
            assert low[1] != got[1], (name, name_p)
        else:
            assert got[1] - low[1] >= 8, (name, name_p, got[1], low[1])
    assert not np.array_equal(ones[0], ones[1])
    # without logical operators: no logical error, the counters that do not look at them unchanged
    none = run(name, np.zeros((0, n), np.uint8))
    assert not none[list(lm.L_ONLY)].any() and np.array_equal(none[list(lm.L_FREE)], base[list(lm.L_FREE)])
    # k = 13, the first 12 rows the same bytes: another answer than k = 12, whatever the order of the rows.  (On
    # [[72,12,6]] only: the 12 rows of the irregular matrix leave 5 non-zero residuals for a 13th row to find.)
    if name == "72":
        more = run(name, lm.extra_row(L))
        print(name, "k = 13 [1]", int(more[1]))
        assert more[1] - base[1] >= 8 and np.array_equal(more, run(name, lm.extra_row(L)[::-1]))
