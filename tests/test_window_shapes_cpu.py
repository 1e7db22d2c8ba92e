"""CPU: what tests/test_gpu_window_shapes.py takes for granted -- the vectorised classification equals
oracle.classify_trials with the two window rules, the batches it decodes pass one grid pass of every glue kernel by the
arithmetic of wo.plan alone, both ends of its 60000 records hold every kind of record, and the matrices it sends to the
general-H kernel have the rows, columns and window classes it says."""
import numpy as np
import pytest

import window_oracle as wo
import window_shapes_util as ws
from oracle import oracle
from qldpc_amd import _lib, bp
from test_window_plan import matrix


def cpu_statement(H, cr, W, F, syn, prior, osd):
    def decode(Hk, s, pr):
        return oracle.decode_batch(Hk, s, pr, ws.MAX_ITER, _lib.MIN_SUM, ws.ALPHA, ws.DAMPING, ws.CLIP)

    def osd0(Hk, s, llr, hard):
        return np.array([oracle.osd0(Hk, s[i], llr[i], hard[i]) for i in range(s.shape[0])], np.uint8)
    return wo.decode(H, cr, W, F, syn, prior, decode, osd0 if osd else None)


@pytest.fixture(scope="module")
def ends():
    """The first 2000 and the last 2000 records of A1's input, and the CPU statement on them."""
    H, cr, errors, syn, prior = ws.inputs("steane", ws.STRIDE_B, ws.STRIDE_SEED)
    rows = np.r_[0:2000, ws.STRIDE_B - 2000:ws.STRIDE_B]
    out = {(W, F, osd): cpu_statement(H, cr, W, F, syn[rows], prior, osd) for W, F in ws.SIZES for osd in (False, True)}
    return H, errors[rows], syn[rows], out


def test_vectorised_classification_equals_classify_trials(ends):
    H, errors, syn, out = ends
    L, _ = ws.mc_inputs()
    seen = 0
    for (W, F, osd), (x, conv, iters, _, fails) in out.items():
        half = slice(0, 2000)
        want = oracle.classify_trials(H, L, ws.MC_DISTANCE, errors[half], syn[half], x[half], fails[half] == 0, iters[half])
        want[10] = int((~conv[half]).sum())                 # the corrections that miss the syndrome
        got, valid = ws.classify(H, L, ws.MC_DISTANCE, errors[half], x[half], iters[half], fails[half])
        assert np.array_equal(got, want), (W, F, osd, got, want)
        assert np.array_equal(valid, conv[half])
        # [5] is asked of H x == s, not of BP: some of its trials have a window BP did not converge on (the window
        # rule that mc_count_trial alone, with conv = window_fails == 0, would miss)
        res = (x[half] ^ errors[half]).astype(np.int64)
        made_valid = (fails[half] > 0) & valid & res.any(axis=1) & ~(res @ L.T % 2).any(axis=1)
        print(f"({W}, {F}) osd {osd}: {got.tolist()}, degenerate with a window BP left {int(made_valid.sum())}")
        assert got[0] == 2000 and got[1] >= 8 and got[6] >= 8 and got[9] >= 8 and got[3] >= 8 and got[4] >= 8
        assert got[5] >= made_valid.sum() and (osd or got[10] >= 8)
        seen += int(made_valid.sum())
    assert seen >= 1


def test_both_ends_of_the_long_batch_hold_every_kind(ends):
    _, _, _, out = ends
    for (W, F, osd), want in out.items():
        for name, part in (("first 2000", slice(0, 2000)), ("last 2000", slice(2000, 4000))):
            ws.assert_kinds([a[part] for a in want], osd, f"({W}, {F}) osd {osd}, {name}")


def test_threshold_arithmetic():
    """From wo.plan alone.  steane, six rounds: m0 = 3 checks and 7 + 3 columns a round.
    (3, 1): four windows of 9 checks; windows 0 .. 2 commit one round (10 columns, 6 checks hold an entry of them: the
    round's own and, through the measurement columns, the next round's), the last all 30 of its columns (9 checks).
    (4, 2): two windows of 12 checks; window 0 commits 20 columns seen by 9 checks, the last 40 seen by 12.
    So B = 60000 gives at least 540000 gather lanes and 1020000 commit items per window against 524288."""
    H, cr = matrix("steane")
    assert ws.GRID_LANES == 524288 and ws.GRID_WAVES == 8192
    assert ws.window_work(H, cr, 3, 1) == [(9, 10, 6)] * 3 + [(9, 30, 9)]
    assert ws.window_work(H, cr, 4, 2) == [(12, 20, 9), (12, 40, 12)]
    assert ws.assert_every_loop_strides(ws.STRIDE_B, H, cr, 3, 1) == 58254
    assert ws.assert_every_loop_strides(ws.STRIDE_B, H, cr, 4, 2) == 43690
    assert ws.STRIDE_B - 2000 < 58254 < ws.STRIDE_B - 8             # (the last 2000 records reach into every later pass)
    # ... and not with the batches of the other window tests
    with pytest.raises(AssertionError):
        ws.assert_every_loop_strides(257, H, cr, 3, 1)
    # Monte-Carlo: one chunk, window_classify_kernel's eighth trip, window_syndrome_kernel's third
    n, m = H.shape[1], H.shape[0]
    assert ws.MC_T <= (1 << 28) // n and ws.MC_T <= 1 << 20
    assert 7 * ws.GRID_WAVES < ws.MC_T <= 8 * ws.GRID_WAVES and 2 * ws.GRID_LANES < ws.MC_T * m
    assert 14 * 4099 < ws.MC_T <= 15 * 4099 and 4099 < ws.GRID_WAVES and 4099 * 17 < ws.GRID_LANES
    # the failure list: one record per lane
    assert ws.LIST_B > ws.GRID_LANES and ws.LIST_B - ws.GRID_LANES == 4099
    rows = ws.list_rows()
    assert np.all(np.diff(rows) > 0) and rows[-1] == ws.LIST_B - 1 and (rows >= ws.GRID_LANES).sum() == 4099
    assert rows.size == 8128 + 2 * 4099


def test_the_failure_list_rows_hold_second_stages():
    """A4's records: BP on window 0 alone tells which of the rows beyond one pass reach the second stage."""
    H, cr, _, syn, prior = ws.inputs("steane", ws.LIST_B, ws.LIST_SEED)
    beyond = syn[ws.GRID_LANES:]
    want = cpu_statement(H, cr, 3, 1, beyond, prior, True)
    plain = cpu_statement(H, cr, 3, 1, beyond, prior, False)
    second = want[4] > 0
    changed = second & (want[0] != plain[0]).any(axis=1)
    print(f"rows beyond {ws.GRID_LANES}: {int(second.sum())} with a second stage, {int(changed.sum())} of them changed by it")
    assert second.sum() >= 8 and changed.sum() >= 1


@pytest.mark.parametrize("make", [ws.heavy_everywhere, ws.heavy_last_round])
def test_heavy_matrices_are_what_the_module_says(make):
    H, cr = make()
    rp, ci, m, n = bp.csr_from_H(H)
    assert ws.fits_on_chip(wo.spacetime(ws.ring(), 6)[0]) and ws.ring().sum(axis=1).tolist() == [4] * 6
    assert ws.ring(True).sum(axis=1).tolist() == [9, 4, 4, 4, 4, 4] and ws.ring(True).sum(axis=0).max() == 3
    for W, F in ws.SIZES:
        plan = _lib.window_plan(rp, ci, m, n, cr, W, F)
        want = wo.plan(H, cr, W, F)
        assert np.array_equal(plan["cls"], want["cls"])
        fits = [ws.fits_on_chip(Hk) for _, _, _, Hk in wo.windows(H, want)]
        rows = [int(Hk.sum(axis=1).max()) for _, _, _, Hk in wo.windows(H, want)]
        print(make.__name__, (W, F), "classes", plan["cls"].tolist(), "heaviest row per window", rows)
        if make is ws.heavy_everywhere:
            assert H.shape == (36, 108) and plan["cls"].tolist() == [0] * plan["K"]
            assert not any(fits) and rows == [11] * plan["K"] and H.sum(axis=0).max() == 3
        else:
            assert H.shape == (37, 108) and H[36].sum() == 9 and cr[36] == 5
            assert plan["cls"].tolist() == [0] * (plan["K"] - 1) + [1]
            assert fits == [True] * (plan["K"] - 1) + [False] and rows == [6] * (plan["K"] - 1) + [9]
