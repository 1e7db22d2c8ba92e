"""The numpy statement of the distance search (tests/distance_oracle.py) alone.  No GPU."""
import numpy as np
import pytest

import distance_cases as dc
import distance_oracle as do


@pytest.mark.parametrize("name", ["steane", "72x", "72z", "rand37", "144"])
def test_codewords_are_detected_kernel_vectors(name):
    c = dc.case(name)
    out = dc.statement(name)
    res, cw = out["result"], out["codeword"]
    assert res[0] == c.trials and res[1] > 0 and c.begin <= res[2] < c.begin + c.trials and 0 <= res[3] < c.G.shape[0]
    assert not (c.H.astype(np.int64) @ cw % 2).any()                      # H c = 0
    lm = (c.L.astype(np.int64) @ cw % 2)
    assert lm.any() and out["logical_mask"] == sum(1 << int(l) for l in np.flatnonzero(lm))      # L c != 0
    assert int(cw.sum()) == res[1]
    hist = out["hist"]
    assert hist.shape == (c.n + 1,) and hist.sum() <= c.trials and hist[:res[1]].sum() == 0 and hist[res[1]] >= 1
    # the reported trial reaches that weight with that row, and no earlier trial does
    first = do.trial(c.G, c.L, c.seed, int(res[2]))
    assert first[0] == res[1] and first[1] == res[3] and np.array_equal(first[2], cw)
    for t in range(c.begin, int(res[2])):
        earlier = do.trial(c.G, c.L, c.seed, t)
        assert earlier is None or earlier[0] > res[1]


def test_hist_counts_the_trials_with_a_result():
    c = dc.case("72x")
    results = [do.trial(c.G, c.L, c.seed, t) for t in range(c.begin, c.begin + c.trials)]
    hist = np.zeros(c.n + 1, np.int64)
    for r in results:
        if r is not None:
            hist[r[0]] += 1
    out = dc.statement("72x")
    assert np.array_equal(out["hist"], hist) and hist.sum() == sum(r is not None for r in results)
    # ADDED to
    again = do.search(c.G, c.L, c.seed, c.begin, c.begin + 8, hist=np.full(c.n + 1, 5, np.int64))
    assert np.array_equal(again["hist"] - 5, do.search(c.G, c.L, c.seed, c.begin, c.begin + 8)["hist"])


@pytest.mark.parametrize("name,cut", [("72x", 1), ("72x", 32), ("steane", 63), ("rand37", 20)])
def test_halves_merge_to_the_whole(name, cut):
    c = dc.case(name)
    whole = dc.statement(name)
    a = do.search(c.G, c.L, c.seed, c.begin, c.begin + cut)
    b = do.search(c.G, c.L, c.seed, c.begin + cut, c.begin + c.trials)
    for merged in (do.merge(a, b),):
        assert np.array_equal(merged["result"], whole["result"]) and np.array_equal(merged["hist"], whole["hist"])
        assert np.array_equal(merged["codeword"], whole["codeword"]) and merged["logical_mask"] == whole["logical_mask"]


def test_an_empty_range_and_an_L_that_detects_nothing():
    c = dc.case("72x")
    out = do.search(c.G, c.L, c.seed, 5, 5)
    assert out["result"].tolist() == [0, -1, -1, -1] and out["codeword"] is None and not out["hist"].any()
    # rows of H are orthogonal to all of ker H
    out = do.search(c.G, c.H[:3], c.seed, 0, 4)
    assert out["result"].tolist() == [4, -1, -1, -1] and out["codeword"] is None and not out["hist"].any()


def test_column_order_is_a_permutation_keyed_by_trial_and_seed():
    a = do.column_order(0, 0, 72)
    assert sorted(a.tolist()) == list(range(72))
    assert not np.array_equal(a, do.column_order(0, 1, 72)) and not np.array_equal(a, do.column_order(1, 0, 72))
    assert not np.array_equal(do.column_order(0, 1 << 32, 72), a)        # hi32(t) is in the counter
    assert not np.array_equal(do.column_order(1 << 32, 0, 72), a)        # hi32(seed) is in the key
    keys = do.column_keys(0, 0, 72)
    assert np.all(keys[a][:-1] <= keys[a][1:]) and keys.max() < 1 << 32


@pytest.mark.parametrize("name,trials,d", [("steane", 64, 3), ("72x", 64, 6), ("144", 128, 12)])
def test_seed_0_reaches_the_distance(name, trials, d):
    """Confirmed on this statement before it was fixed here: the Philox order reaches 3, 6 and 12 within these trial
    counts at seed 0 (on [[144,12,12]] at trial 1)."""
    c = dc.case(name)
    assert (c.seed, c.begin, c.trials) == (0, 0, trials)
    assert dc.statement(name)["result"][1] == d
