"""CPU: the posterior-LLR histograms per iteration budget (qbp_mc_run_llr_hist) -- the numpy statement against a
fixture made by the reference's own loops, its identities, the argument checks, sharding with ONE reduce, and that the
inputs of the GPU tests reach every kind of column."""
import os

import numpy as np
import pytest

import llr_hist_cases as cases
from budget_oracle import ladder_counters
from llr_hist_oracle import columns, llr_hist, llr_hist_of_errors
from qldpc_amd import _lib, codes, dem, mc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "llr_hist.npz"))
    code = codes.load_code(str(g["code"]))
    errors = np.unpackbits(g["errors"], axis=1)[:, :code.n]
    p = float(g["p"])
    lo, hi = (float(x) for x in g["range"])
    hist = llr_hist_of_errors(code.Hx, errors, mc.prior_of(p, code.n), g["limits"], int(g["bins"]), lo, hi)
    return g, code, errors, hist


def test_statement_equals_the_reference_lists(golden):
    """llrs_per_iter = rows 0 + 1 + 2 + 3, llrs_per_iter_after_OSD = rows 2 + 3 (BP_per_Iteration.py), true_0 = rows
    0 + 2, true_1 = rows 1 + 3 (rework/Alvarado.py): np.histogram counts and the values outside the range."""
    g, code, errors, hist = golden
    bins = int(g["bins"])
    assert list(g["lists"]) == ["iter_llrs", "iter_llrs_after_OSD", "true_0", "true_1"]
    assert hist.shape == (len(g["limits"]), 4, bins + 3) and not hist[:, :, bins + 2].any()
    sums = np.stack([hist.sum(axis=1), hist[:, 2] + hist[:, 3], hist[:, 0] + hist[:, 2], hist[:, 1] + hist[:, 3]], axis=1)
    assert np.array_equal(sums[:, :, 1:bins + 1], g["counts"])
    assert np.array_equal(sums[:, :, 0], g["outside"][:, :, 0]) and np.array_equal(sums[:, :, bins + 1], g["outside"][:, :, 1])
    # the fixture is not trivial: unconverged trials at every limit, fewer with more iterations, values outside the range
    assert (g["counts"][:, 1].sum(axis=1) > 0).all() and g["counts"][0, 1].sum() > g["counts"][-1, 1].sum()
    assert g["outside"].sum() > 0


def test_identities(golden):
    g, code, errors, hist = golden
    T, n = errors.shape
    p = float(g["p"])
    cnt = np.stack([ladder_counters(code.Hx, code.Lx, code.distance, p, mc.prior_of(p, n), 0, 500, g["limits"], seed=3)])[0]
    lo, hi = (float(x) for x in g["range"])
    sampled = llr_hist(code.Hx, p, mc.prior_of(p, n), 0, 500, g["limits"], int(g["bins"]), lo, hi, seed=3)
    from oracle import oracle
    weight = int(oracle.mc_errors(n, p, 1, 3, 0, 500).sum())
    for j in range(len(g["limits"])):
        assert sampled[j].sum() == n * cnt[j, 0]
        assert sampled[j, 2:].sum() == n * cnt[j, 6]
        assert sampled[j, 1].sum() + sampled[j, 3].sum() == weight
        assert hist[j].sum() == n * T and hist[j, 1].sum() + hist[j, 3].sum() == int(errors.sum())
    assert cnt[0, 6] > cnt[-1, 6] > 0


def test_columns_rule():
    """Left-closed bins, the last one closed on both sides; -inf / +inf / NaN in their own columns."""
    x = np.array([-np.inf, -1.0000001, -1.0, -0.5, 0.0, 0.5, 1.0, 1.0000001, np.inf, np.nan, np.nan])
    assert columns(x, 4, -1.0, 1.0).tolist() == [2, 1, 1, 1, 2, 2, 2]
    assert columns([], 3, 0.0, 1.0).tolist() == [0] * 6
    assert np.array_equal(_lib.llr_hist_edges(4, -1.0, 1.0), np.linspace(-1.0, 1.0, 5))


def _never(*a):
    raise AssertionError("the runner must not be reached")


@pytest.mark.parametrize("bins,lo,hi,K", [
    (0, -1.0, 1.0, 1), (-3, -1.0, 1.0, 1), (2.5, -1.0, 1.0, 1), (True, -1.0, 1.0, 1), (8, 1.0, 1.0, 1), (8, 2.0, 1.0, 1),
    (8, -np.inf, 1.0, 1), (8, 0.0, np.inf, 1), (8, np.nan, 1.0, 1), (8, "a", 1.0, 1),
    (2046, -1.0, 1.0, 1), (1022, -1.0, 1.0, 2), (129, -1.0, 1.0, 16),
], ids=lambda v: str(v))
def test_check_llr_hist_refusals(bins, lo, hi, K):
    with pytest.raises(ValueError):
        _lib.check_llr_hist(bins, lo, hi, K)
    budgets = list(range(1, K + 1))
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.01)
    for runner in (_never, None):       # (no runner: the default path would need a GPU, and must not get that far)
        with pytest.raises(ValueError):
            mc.run_llr_hist("[[72, 12, 6]]", 0.05, 100, budgets, bins, (lo, hi), runner=runner)
        with pytest.raises(ValueError):
            mc.run_dem_llr_hist(H, L, probs, 100, budgets, bins, (lo, hi), runner=runner)


def test_check_llr_hist_accepts_the_cap():
    assert _lib.LLR_HIST_ROWS == 4
    assert _lib.check_llr_hist(128, -30, 30.0, 9) == (128, -30.0, 30.0)
    assert _lib.check_llr_hist(1024, -1.0, 1.0, 1)[0] == 1024
    assert _lib.check_llr_hist(2045, -1.0, 1.0, 1)[0] == 2045          # 4 * 2048 words: exactly the cap
    assert _lib.check_llr_hist(np.int32(125), 0, 1, 16)[0] == 125
    with pytest.raises(ValueError):
        mc.run_llr_hist("[[72, 12, 6]]", 0.05, 100, [5, 4], 8, (-1, 1), runner=_never)
    with pytest.raises(ValueError):
        mc.bp_per_iteration(["[[72, 12, 6]]"], 0.05, [5], 100, llr_bins=8, runner=_never)


def test_constants_equal_the_header():
    text = open(os.path.join(os.path.dirname(HERE), "include", "qbp.h")).read()
    assert f"#define QBP_LLR_HIST_ROWS {_lib.LLR_HIST_ROWS}\n" in text
    assert f"#define QBP_LLR_HIST_MAX_WORDS {_lib.LLR_HIST_MAX_WORDS}\n" in text
    assert f"QBP_OPT_LLR_HIST_CHUNK = {_lib.OPT_LLR_HIST_CHUNK}," in text
    for name, nargs in (("qbp_mc_run_llr_hist", 22), ("qbp_mc_run_llr_hist_device", 23), ("qbp_mc_run_errors_llr_hist", 19)):
        assert len(_lib.SIGNATURES[name][1]) == nargs


PS, TRIALS, BUDGETS, BINS, RANGE = 0.06, 301, (2, 5, 30), 24, (-9.0, 11.0)


def _oracle_runner(code, p, budgets, bins, llr_range, begin, end):
    prior = mc.prior_of(p, code.n)
    return (ladder_counters(code.Hx, code.Lx, code.distance, p, prior, begin, end, budgets, seed=11),
            llr_hist(code.Hx, p, prior, begin, end, budgets, bins, *llr_range, seed=11))


def test_shards_and_the_single_reduce():
    """Three ranks, each through run_llr_hist with its own slice; counters and table travel in ONE all-reduce."""
    one_cnt, one_hist, edges = mc.run_llr_hist("[[72, 12, 6]]", PS, TRIALS, BUDGETS, BINS, RANGE, runner=_oracle_runner)
    assert one_cnt.shape == (3, 12) and one_hist.shape == (3, 4, BINS + 3)
    assert np.array_equal(edges, np.linspace(*RANGE, BINS + 1))
    sent = []

    def all_reduce(flat):
        sent.append(np.array(flat))
        return flat

    world = 3
    for rank in range(world):
        mc.run_llr_hist("[[72, 12, 6]]", PS, TRIALS, BUDGETS, BINS, RANGE, rank=rank, world=world, runner=_oracle_runner,
                        all_reduce=all_reduce)
    assert len(sent) == world                                   # one reduce per rank
    assert all(s.size == 3 * 12 + 3 * 4 * (BINS + 3) for s in sent)
    cnt, hist = mc._split_llr_hist(np.sum(sent, axis=0), 3, BINS)
    assert np.array_equal(cnt, one_cnt) and np.array_equal(hist, one_hist)
    assert (cnt[:, 0] == TRIALS).all() and hist[0, 2:].sum() > hist[-1, 2:].sum() > 0
    # the matrix form, with a probability per column
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.02)

    def dem_runner(H, L, probs, prior, budgets, bins, llr_range, begin, end):
        return (np.zeros((len(budgets), 12), np.int64),
                llr_hist(H, probs, prior, begin, end, budgets, bins, *llr_range, seed=0))

    whole = mc.run_dem_llr_hist(H, L, probs, 60, (1, 6), 8, (-5, 5), runner=dem_runner)[1]
    parts = sum(mc.run_dem_llr_hist(H, L, probs, 60, (1, 6), 8, (-5, 5), rank=r, world=2, runner=dem_runner)[1] for r in (0, 1))
    assert np.array_equal(whole, parts) and whole.sum() == 2 * 60 * H.shape[1]


def test_bp_per_iteration_and_llr_distributions():
    def budgets_runner(code, p, budgets, begin, end):
        return ladder_counters(code.Hx, code.Lx, code.distance, p, mc.prior_of(p, code.n), begin, end, budgets, seed=11)

    name = "[[72, 12, 6]]"
    plain = mc.bp_per_iteration([name], PS, BUDGETS, TRIALS, osd=False, runner=budgets_runner)
    assert set(plain[name]) == {"logicalErrors", "degeneracies", "OSD_invocations", "iterations"}      # as ever
    table = mc.run_budgets(name, PS, TRIALS, BUDGETS, runner=budgets_runner)
    assert plain[name]["OSD_invocations"] == (table[:, 6] / TRIALS).tolist()
    assert plain[name]["logicalErrors"] == (table[:, 1] / TRIALS).tolist()
    rich = mc.bp_per_iteration([name], PS, BUDGETS, TRIALS, osd=False, llr_bins=BINS, llr_range=RANGE, runner=_oracle_runner)
    for k in plain[name]:
        assert rich[name][k] == plain[name][k]
    assert set(rich[name]) - set(plain[name]) == {"llrs_per_iter_hist", "llrs_per_iter_after_OSD_hist", "llr_edges"}
    _, hist, edges = mc.run_llr_hist(name, PS, TRIALS, BUDGETS, BINS, RANGE, runner=_oracle_runner)
    assert np.array_equal(rich[name]["llrs_per_iter_hist"], hist.sum(axis=1))
    assert np.array_equal(rich[name]["llrs_per_iter_after_OSD_hist"], hist[:, 2] + hist[:, 3])
    assert np.array_equal(rich[name]["llr_edges"], edges)
    assert (rich[name]["llrs_per_iter_hist"].sum(axis=1) == 72 * TRIALS).all()
    d = mc.llr_distributions(name, PS, TRIALS, 30, BINS, RANGE, runner=_oracle_runner)
    assert set(d) == {"true_0", "true_1", "edges"}
    assert np.array_equal(d["true_0"], hist[2, 0] + hist[2, 2]) and np.array_equal(d["true_1"], hist[2, 1] + hist[2, 3])


def test_gpu_inputs_reach_every_kind_of_column():
    """The cases of tests/test_gpu_llr_hist.py, by the statement: interior bins in all four rows, both outer columns,
    the NaN column, and priors exactly on lo, on hi and on an interior edge."""
    c, h = cases.case("steane"), cases.statement("steane")       # (seven bits: every trial is settled by iteration 3)
    assert (h.sum(axis=(1, 2)) == 7 * c.T).all() and ((h[:, :2, 1:c.bins + 1] > 0).sum(axis=2) >= 3).all()
    assert h[0, 2:].sum() > 0 and h[:, :, c.bins + 1].sum() > 0 and not np.array_equal(h[0], h[1])
    # (damped min-sum on the irregular matrix runs into NaN messages behind its rows of weight 1: the general-H kernel's
    # NaN column; what it leaves unconverged is all NaN)
    c, h = cases.case("rand37_minsum"), cases.statement("rand37_minsum")
    assert h[:, :, c.bins + 2].sum() > 0 and ((h[:, :2, 1:c.bins + 1] > 0).sum(axis=2) >= 3).all()
    assert (h.sum(axis=(1, 2)) == 37 * c.T).all() and h[0, 2:].sum() > h[-1, 2:].sum() > 0
    for name in ("72", "72_minsum", "dem72", "rand37"):
        c, h = cases.case(name), cases.statement(name)
        n = c.H.shape[1]
        assert h.shape == (len(c.budgets), 4, c.bins + 3) and (h.sum(axis=(1, 2)) == n * c.T).all(), name
        inside = h[:, :, 1:c.bins + 1]
        assert ((inside > 0).sum(axis=2) >= 3).all(), (name, (inside > 0).sum(axis=2))      # every row of every budget
        assert h[:, :, 0].sum() > 0 and h[:, :, c.bins + 1].sum() > 0, name                 # both outer columns
        assert h[0, 2:].sum() > h[-1, 2:].sum() > 0, name          # unconverged at every budget, fewer at the last
        assert h[-1, :2].sum() > h[0, :2].sum(), name
        assert not np.array_equal(h[0], h[1]) and not np.array_equal(h[1], h[2]), name
    c, h = cases.case("inf_nan"), cases.statement("inf_nan")
    # NaN from the second iteration on; after the first one the +inf posterior of every trial, above the range
    assert h[1:, :, c.bins + 2].sum() > 0 and not h[0, :, c.bins + 2].any() and h[0, :, c.bins + 1].sum() >= c.T
    # priors exactly on edges: the two columns without a check add T to the bin of their prior, whatever the budget
    bins, (lo, hi) = cases.ZERO_BINS, cases.ZERO_RANGE
    plain = cases.statement("72", bins, (lo, hi))
    for name, where in (("zero_lo_hi", (1, bins)), ("zero_edge_lo", (cases.ZERO_EDGE + 1, 1))):
        c, h = cases.case(name), cases.statement(name)
        assert not c.H[:, list(cases.ZERO_COLUMNS)].any() and c.H.any(axis=0).sum() == 70
        edges = np.linspace(lo, hi, bins + 1)
        for v, col in zip(cases.ZERO_COLUMNS, where):
            assert c.prior[v] == edges[col - 1] if col < bins else c.prior[v] == edges[bins]
            assert columns([c.prior[v]], bins, lo, hi)[col] == 1
        for j in range(len(c.budgets)):
            per_col = h[j].sum(axis=0)
            for col in set(where):
                assert per_col[col] >= c.T * where.count(col)
    assert plain.shape == h.shape
