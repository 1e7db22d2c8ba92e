"""No GPU: every case of tests/quant_large_cases.py reaches the path of bp_quant_kernel it is named for.  Asserted on
shapes, on the restated launch arithmetic and on the statement's output alone -- the conditions on the inputs that
tests/test_gpu_quant_large.py relies on."""
import numpy as np
import pytest

import quant_cases as qc
import quant_large_cases as lc
import quant_oracle as qo
from qldpc_amd import quant

PIDS = {lc.Q4: "q4", lc.Q6: "q6", lc.Q8: "q8", lc.Q16: "q16"}


# ---- shapes ---------------------------------------------------------------------------------------------------------------
def test_ph72x9_walks_the_syndrome_ballot_twice_with_a_ragged_second_trip():
    c = lc.case("ph72x9")
    assert c.shape == (324, 972, 2556)
    # the ballot: a wavefront takes rows c0 .. c0 + 63 with c0 = 64 w + 256 trip; its lane 0 writes words c0 / 32 and,
    # if it is below mw, c0 / 32 + 1.  Trip 1: wavefront 0 at c0 = 256 writes words 8 and 9, wavefront 1 at c0 = 320
    # writes word 10 and must not write word 11 = mw; wavefronts 2 and 3 have no second trip
    mw = (c.m + 31) // 32
    assert mw == 11 and 256 + 64 < c.m <= 256 + 128
    assert (320 >> 5) + 1 == mw
    assert lc.THREADS < c.m and lc.THREADS < c.n and lc.THREADS < c.E


def test_tall_has_a_column_of_300_entries_two_empty_columns_and_more_rows_than_columns():
    c = lc.case("tall")
    H = c.H
    assert c.m == 300 and c.n == 96 and c.m > c.n and c.m > lc.THREADS
    assert c.E == int(H.sum()) == 1105
    col_w, row_w = H.sum(axis=0), H.sum(axis=1)
    assert set(row_w.tolist()) == {3, 4}
    assert col_w[lc.TALL_HEAVY] == 300 > lc.THREADS and col_w[lc.TALL_HEAVY] > qo.M_of(8)
    assert np.flatnonzero(col_w == 0).tolist() == list(lc.TALL_EMPTY)
    rest = np.delete(col_w, (lc.TALL_HEAVY,) + lc.TALL_EMPTY)
    assert 3 <= rest.min() and rest.max() <= 17 and 8 <= rest.mean() <= 9.5
    assert (c.m + 31) // 32 == 10                       # the second trip of the ballot: wavefront 0 alone, two words


def test_refill_case_is_the_small_matrix():
    c = lc.case("refill")
    assert c.shape == (36, 72, 216) and c.errors.shape == (lc.REFILL_POOL, 72) and c.L.shape == (12, 72) and c.d == 6


# ---- launch arithmetic ------------------------------------------------------------------------------------------------------
def test_restated_lds_bytes_by_hand():
    # ph72x9, int8: P 972 words; per slot V 972 + messages 2556 / 4 = 639 + bookkeeping 10 + 11 + 1 = 22; 32 words;
    # 972 + 1611 = 2583 words of state are rounded up to even
    assert quant.lds_bytes(324, 972, 2556, 1, False) == 4 * (2584 + 32 + 22) == 10552
    assert quant.lds_bytes(324, 972, 2556, 24, False) == 4 * (972 + 24 * 1611 + 32 + 24 * 22) == 160784
    assert quant.lds_bytes(324, 972, 2556, 17, True) == 4 * (972 + 17 * (972 + 1278) + 32 + 17 * 22) == 158512
    # tall, int8: 1105 bytes of messages are 277 words; 96 + 373 = 469 words are rounded up to even
    assert quant.lds_bytes(300, 96, 1105, 1, False) == 4 * (470 + 32 + 20) == 2088


# (tag, wide) -> {QBP_OPT_QUANT_SLOTS: (slots, lds_bytes)} on a batch of 48
GEOMETRY = {
    ("ph72x9", False): {0: (1, 10552), 1: (1, 10552), 3: (3, 23616), 32: (24, 160784)},
    ("ph72x9", True): {0: (1, 13104), 1: (1, 13104), 3: (3, 31280), 32: (17, 158512)},
    ("tall", False): {0: (10, 16232), 1: (1, 2088), 3: (3, 5232), 32: (32, 50816)},
    ("tall", True): {0: (10, 27272), 1: (1, 3192), 3: (3, 8544), 32: (32, 86144)},
}


@pytest.mark.parametrize("tag,is_wide", list(GEOMETRY))
def test_slots_and_lds_of_every_geometry_the_gpu_tests_launch(tag, is_wide):
    c = lc.case(tag)
    for opt, (S, lds) in GEOMETRY[tag, is_wide].items():
        got = lc.geometry(c.shape, is_wide, lc.BATCH, 256, opt)
        print(tag, "int16" if is_wide else "int8", "option", opt, "-> (slots, grid, lds_bytes)", got)
        assert (got[0], got[2]) == (S, lds) and lds <= lc.LDS_LIMIT
        assert got[1] == -(-lc.BATCH // S)                  # (48 records never fill 256 CUs)
    # the tiled batch: one slot, one workgroup per CU, more records than workgroups
    assert lc.geometry(c.shape, is_wide, 2 * 256 + 5, 256, 1, 1)[:2] == (1, 256)


def test_option_32_is_lowered_by_the_160_kib_loop_on_ph72x9_only():
    ph, tall = lc.case("ph72x9"), lc.case("tall")
    for is_wide, S in ((False, 24), (True, 17)):
        assert lc.slots(ph.shape, is_wide, lc.BATCH, 32) == S < 32
        assert lc.lds_bytes(ph.shape, S, is_wide) <= lc.LDS_LIMIT < lc.lds_bytes(ph.shape, S + 1, is_wide)
        assert lc.LDS_DEFAULT < lc.lds_bytes(ph.shape, S, is_wide)
        assert lc.slots(ph.shape, is_wide, lc.BATCH, 0) == 1 == 4 * lc.THREADS // ph.n
        assert lc.slots(tall.shape, is_wide, lc.BATCH, 32) == 32
    # the records bound the slots last
    assert lc.slots(ph.shape, False, 5, 32) == 5 and lc.slots(tall.shape, True, 1, 0) == 1


def test_which_geometries_lie_above_the_default_dynamic_lds():
    """Above 64 KiB a launch needs hipFuncSetAttribute: ph72x9 under option 32 at both widths (the batch and the
    Monte-Carlo build, so all four instantiations), tall under option 32 at int16 only."""
    above = {(tag, w, opt) for (tag, w), g in GEOMETRY.items() for opt, (_, lds) in g.items() if lds > lc.LDS_DEFAULT}
    assert above == {("ph72x9", False, 32), ("ph72x9", True, 32), ("tall", True, 32)}


def test_refill_geometry_gives_every_slot_a_second_trial():
    c = lc.case("refill")
    for cus in (8, 256, 304):
        for is_wide in (False, True):
            for S in (1, 3):
                T = 2 * cus * S + 5
                assert lc.geometry(c.shape, is_wide, T, cus, S, 1)[:2] == (S, cus)
                assert T >= 2 * cus * S                     # first come grid * S trials, the rest through the counter
                # the halves and the thirds of the range still pass the grid once
                assert lc.geometry(c.shape, is_wide, T // 2, cus, S, 1)[1] == cus
                assert T // 3 > cus * S // 2


# ---- the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("tag,params", [(t, p) for t in lc.TAGS for p in lc.BATCH_PARAMS[t]], ids=lambda x: PIDS.get(x, x))
def test_batches_hold_every_record_class(tag, kind, params):
    hard, conv, iters, V, llr = lc.statement(tag, kind, params)
    counts = qc.classes(conv, iters)
    print(tag, kind, params, "(at 0, later, never)", counts)
    assert len(conv) == lc.BATCH and min(counts) >= 4
    assert iters.max() == lc.MAX_ITER - 1 and 1 <= iters[conv].max() < lc.MAX_ITER
    # with max_iter = 1 the records of the first class alone converge
    hard1, conv1, iters1, V1, _ = lc.statement(tag, kind, params, 1)
    assert np.array_equal(conv1, conv & (iters == 0)) and not iters1.any()
    assert np.array_equal(V1[conv1], V[conv1]) and (V1[~conv] != V[~conv]).any()


@pytest.mark.parametrize("params", lc.MC_PARAMS, ids=lambda p: PIDS[p])
@pytest.mark.parametrize("tag", lc.TAGS)
def test_monte_carlo_batches_hold_every_record_class(tag, params):
    out, counters = lc.mc_statement(tag, params)
    counts = qc.classes(out[1], out[2])
    print(tag, params, "(at 0, later, never)", counts, counters.tolist())
    assert min(counts) >= 4 and counters[0] == lc.BATCH and counters[6] == counts[2]
    assert counters[1] >= 4                             # logical failures, so the counters are no row of zeros


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("params", [lc.Q4, lc.Q8], ids=lambda p: PIDS[p])
def test_tall_posterior_of_the_heavy_column_leaves_the_message_range(params, kind):
    """V = P + sum R is an int32 without saturation: on the column of 300 entries it passes M, and passes 127, the
    range of an int8 message, at both bit widths -- a sum kept in the message type would wrap."""
    M = qo.M_of(params[0])
    V = lc.statement("tall", kind, params)[3][:, lc.TALL_HEAVY].astype(np.int64)
    print(params, kind, "|V| > M:", int((np.abs(V) > M).sum()), "|V| > 127:", int((np.abs(V) > 127).sum()), "max", int(np.abs(V).max()))
    assert (np.abs(V) > M).sum() >= 8 and (np.abs(V) > 127).sum() >= 8
    assert (V > 127).sum() >= 4 and (V < -127).sum() >= 4
    # the empty columns keep V = P
    Vall = lc.statement("tall", kind, params)[3]
    P = qo.quantize(lc.batch_inputs("tall", kind)[1], params[0], params[1])
    assert np.array_equal(Vall[:, list(lc.TALL_EMPTY)], np.tile(P[list(lc.TALL_EMPTY)], (lc.BATCH, 1)))


@pytest.mark.parametrize("params", lc.MC_PARAMS, ids=lambda p: PIDS[p])
def test_refill_pool_gives_the_resets_something_to_clear(params):
    """Part 2 of the turnover clears the logical mask, the error weight and the difference flag of a classified trial;
    a slot that does not would carry them into its next trial.  So among the trials the statement converges there are
    converged-but-wrong ones (a difference, a weight) and ones with a nonzero logical mask; and trials it never
    converges, which the failure-list path hands on."""
    c = lc.case("refill")
    out, counters = lc.mc_statement("refill", params)
    wrong, logical, never = lc.residual_classes(c, out)
    print(params, "converged but wrong", wrong, "of them logical", logical, "never", never, counters.tolist())
    assert wrong >= 8 and logical >= 4 and never >= 8
    assert (out[1] & ~(out[0] ^ c.errors).any(axis=1)).sum() >= 8       # and trials decoded exactly, which a stale flag spoils
    assert (c.errors.sum(axis=1) >= c.d // 2).sum() >= 8 and (c.errors.sum(axis=1) > 0).all()
