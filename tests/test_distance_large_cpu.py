"""The cases of tests/distance_large_cases.py are what that module says, and they discriminate: for each defect a
kernel could have at a limit, the numpy statement with that defect built in (the keyword arguments of
tests/distance_oracle.py) gives another output than the statement on the case named for it -- so the bit-for-bit GPU
comparison of tests/test_gpu_distance_large.py on that case means something about the defect.  No GPU.

Every case of dlc.PARITY is in one of the "differs" assertions below, except:
  n1, n2, n3   NP = 4 > n: the only rule at stake is that the padding sorts behind the columns; no defect listed here.
  dem72        a detector error model through distance.bound: the matrix class, not a limit of the kernel.
r129_passes and wide8192_queue (GPU file only) are r129 and wide8192 over longer trial ranges: grid passes, not rules.
"""
import numpy as np
import pytest

import distance_large_cases as dlc
import distance_oracle as do
from qldpc_amd import gf2


def outputs(out):
    return (out["result"].tolist(), out["hist"].tolist(), None if out["codeword"] is None else out["codeword"].tolist(),
            out["logical_mask"])


def wrong(name, **defect):
    c = dlc.case(name)
    return do.search(c.G, c.L, c.seed, c.begin, c.begin + c.trials, **defect)


def differs(name, **defect):
    return outputs(wrong(name, **defect)) != outputs(dlc.statement(name))


def tied(tie):
    """The positions of equal neighbours in the sorted keys of a pinned trial, and the columns there."""
    keys = do.column_keys(tie["seed"], tie["trial"], tie["n"])
    order = do.column_order(tie["seed"], tie["trial"], tie["n"])
    at = np.flatnonzero(keys[order][:-1] == keys[order][1:])
    return at.tolist(), order


SHAPES = {   # name: (r, n, k, trials, W, NP, LDS bytes)
    "r2048_low": (2048, 576, 3, 4, 18, 1024, 157696), "r2048_high": (2048, 576, 3, 4, 18, 1024, 157696),
    "r1985": (1985, 200, 3, 4, 7, 256, 1985 * 8 * 4 + 512), "r1984": (1984, 200, 3, 4, 7, 256, 1984 * 8 * 4 + 512),
    "r129": (129, 200, 3, 16, 7, 256, 129 * 8 * 4 + 512), "r128": (128, 200, 3, 16, 7, 256, 128 * 8 * 4 + 512),
    "tall": (300, 96, 3, 16, 3, 128, 300 * 4 * 4 + 256),
    "288x": (150, 288, 12, 16, 9, 512, 150 * 10 * 4 + 1024), "288z": (150, 288, 12, 16, 9, 512, 150 * 10 * 4 + 1024),
    "wide8192": (120, 8192, 3, 4, 256, 8192, 120 * 257 * 4 + 16384),
    "at_limit": (63, 16384, 3, 4, 512, 16384, 163840),
    "tie": (40, 512, 2, 4, 16, 512, 8 * 512 + 1024),
    "n1": (1, 1, 1, 4, 1, 4, 48), "n2": (1, 2, 1, 4, 1, 4, 48), "n3": (2, 3, 1, 4, 1, 4, 48),
    "dem72": (216, 324, 12, 8, 11, 512, 216 * 12 * 4 + 1024),
}


@pytest.mark.parametrize("name", dlc.PARITY)
def test_shape_lds_bytes_and_a_weight_found(name):
    c, out = dlc.case(name), dlc.statement(name)
    r, n, k, trials, W, NP, lds = SHAPES[name]
    assert c.G.shape == (r, n) and c.L.shape == (k, n) and c.trials == trials
    assert dlc.lds_bytes(r, n) == (lds, W, NP) and lds <= dlc.LDS_LIMIT
    assert not (c.H.astype(np.int64) @ c.G.T % 2).any()
    res = out["result"]
    assert res[0] == trials and res[1] > 0 and c.begin <= res[2] < c.begin + trials and 0 <= res[3] < r
    assert out["codeword"].sum() == res[1] and out["hist"].sum() == trials           # every trial has a result


def test_the_limits_are_where_the_cases_say():
    assert set(SHAPES) == set(dlc.PARITY)
    # r = 2048 at n = 576 fits; one more word per row (n = 577) does not: the most rows at their widest n
    assert dlc.lds_bytes(2048, 576)[0] <= dlc.LDS_LIMIT < dlc.lds_bytes(2048, 577)[0]
    # n = 16384: 63 rows are exactly 160 KiB, 64 rows are 164 096 B
    assert dlc.lds_bytes(63, 16384)[0] == dlc.LDS_LIMIT == 163840 and dlc.lds_bytes(64, 16384)[0] == 164096
    # n = 16385: NP = 32768, 10 bytes per sorted column alone are 320 KiB -- the bytes refuse every n > 16384, so
    # the check against 65535 columns never is the one that fires
    assert dlc.lds_bytes(1, 16385)[1:] == (513, 32768) and dlc.lds_bytes(1, 16385)[0] == 10 * 32768 > dlc.LDS_LIMIT
    # a lane gains its 3rd row at r = 129 and its 32nd at r = 1985
    for r, rows in ((128, 2), (129, 3), (1984, 31), (1985, 32), (2048, 32)):
        assert len(range(0, r, 64)) == rows


def test_stacked_cases_low_rows_high_rows_and_rank():
    low, high = dlc.case("r2048_low"), dlc.case("r2048_high")
    nb = 540
    assert gf2.rank(low.G[:nb]) == nb == gf2.rank(low.G) < 2048            # a basis, then 1508 dependent rows
    assert np.array_equal(high.G[:2048 - nb], low.G[nb:]) and np.array_equal(high.G[2048 - nb:], low.G[:nb])
    assert np.array_equal(low.H, high.H) and np.array_equal(low.L, high.L)
    # the rows from 1984 on (bit 31 of every lane's masks) are independent of all rows before them: pivots in every trial
    assert gf2.rank(high.G[:1984]) == nb - 64
    # low: every pivot is one of the first 540 rows and every row behind them reduces to zero; the sweep walks all
    # 576 columns with rows left
    A = do.reduce_rows(low.G, do.column_order(low.seed, low.begin, low.n))
    assert not A[nb:].any() and (A[:nb].any(axis=1)).all()
    # high: the result row of the call is in bit 31
    assert dlc.statement("r2048_high")["result"][3] >= 1984
    assert dlc.statement("r2048_low")["result"][3] < nb
    for name, r in (("r1985", 1985), ("r1984", 1984), ("r129", 129), ("r128", 128)):
        c = dlc.case(name)
        nb = gf2.rank(c.G)
        assert nb < r and gf2.rank(c.G[r - nb:]) == nb and gf2.rank(c.G[:r - 1]) == nb - 1      # the last row is needed
    assert dlc.statement("r1985")["result"][3] == 1984                      # the one row in a lane's bit 31
    # r129: trial 50 of the range has its result in row 128, the one row in a lane's bit 2
    c = dlc.case("r129")
    assert c.begin <= 50 < c.begin + c.trials and do.trial(c.G, c.L, c.seed, 50)[1] == 128


def test_tall_ends_on_the_columns():
    c = dlc.case("tall")
    rank = gf2.rank(c.G)
    assert c.G.shape[0] > c.n > rank == 60
    # (left > 0 after the last column: 240 rows never get a pivot, and they are zero)
    A = do.reduce_rows(c.G, do.column_order(c.seed, c.begin, c.n))
    assert (A.any(axis=1)).sum() == rank


def test_wide_and_code_cases():
    w = dlc.case("wide8192")
    assert not w.G[:, :2].any() and gf2.rank(w.G) == 120 and w.L[0].all()
    assert 0.005 < w.G.mean() < 0.015
    assert dlc.statement("wide8192")["result"][1] > 256 // 32                 # (nowhere near a unit vector)
    x = dlc.statement("288x")["result"]
    assert (dlc.case("288x").seed, dlc.case("288x").begin) == (0, 0) and x.tolist()[:3] == [16, 24, 4]
    assert dlc.statement("288z")["result"][1] >= 18
    d = dlc.case("dem72")
    assert d.H.shape == (108, 324) and gf2.rank(d.G) == 216 == d.n - gf2.rank(d.H)


def test_the_pinned_ties_are_ties():
    for tie, name in ((dlc.TIE_512, "tie"), (dlc.TIE_16384, "at_limit")):
        at, order = tied(tie)
        q, a, b = tie["q"], tie["a"], tie["b"]
        assert at == [q] and (order[q], order[q + 1]) == (a, b) and a < b
        c = dlc.case(name)
        assert c.seed == tie["seed"] and c.begin <= tie["trial"] < c.begin + c.trials
        r = c.G.shape[0]
        assert gf2.rank(c.G) == r and gf2.rank(c.G[:, order[:q]]) == r - 1
        for col in (a, b):                                 # each of a, b alone completes the rank
            assert gf2.rank(c.G[:, list(order[:q]) + [col]]) == r
        assert c.G[0, a] == 1 and c.G[0, b] == 0            # ... and the two pivots leave row 0 differently
    assert dlc.case("tie").begin == dlc.TIE_512["trial"] - 2 and dlc.case("tie").trials == 4


# ---- the cases discriminate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tie", "at_limit"])
def test_ties_by_descending_column_differ(name):
    assert differs(name, ties="descending")


@pytest.mark.parametrize("name", ["r2048_high", "r1985"])
def test_rows_from_1984_on_never_chosen_as_pivots_differ(name):
    assert differs(name, pivot_rows=1984)


@pytest.mark.parametrize("name", ["r129", "r2048_high", "r2048_low"])
def test_rows_from_128_on_never_considered_differ(name):
    assert differs(name, candidate_rows=128)


@pytest.mark.parametrize("name", ["r1984", "r128"])
def test_the_last_row_left_out_differs(name):
    """r - 1 in place of r, in the sweep and in the row walk, at the row counts where every lane's last bit is full."""
    r = dlc.case(name).G.shape[0]
    assert differs(name, pivot_rows=r - 1) and differs(name, candidate_rows=r - 1)


@pytest.mark.parametrize("name", ["288x", "288z", "wide8192"])
def test_weights_over_the_first_8_words_differ(name):
    assert differs(name, weight_columns=8 * 32)


def test_a_sweep_that_stops_before_the_columns_are_exhausted_differs():
    """On ``tall`` r > n, so a sweep cut after min(r, n) columns is the whole sweep (asserted: no difference, by
    arithmetic).  What the case does tell apart is a sweep that allows itself one column per pivot there is to find --
    rank(G) = 60 columns -- instead of going on to the last column while rows are left."""
    c = dlc.case("tall")
    assert min(c.G.shape) == c.n and not differs("tall", column_budget=min(c.G.shape))
    assert differs("tall", column_budget=gf2.rank(c.G))
