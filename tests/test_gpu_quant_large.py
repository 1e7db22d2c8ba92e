"""GPU: bp_quant_kernel where the small matrices of tests/test_gpu_quant.py do not take it -- m > 256 and m > 320 (the
second trip of the syndrome ballot, two words from wavefront 0 and the guarded word of a ragged wavefront 1), a column
of 300 entries, m > n, dynamic LDS between 64 and 160 KiB in all four instantiations, QBP_OPT_QUANT_SLOTS lowered by the
160 KiB loop, and slots of the Monte-Carlo build that take a second trial from the work counter -- against the numpy
statement (tests/quant_oracle.py, its edge-indexed twin) bit for bit, into poisoned buffers.

tests/test_quant_large_cpu.py asserts, without a GPU, that the cases of tests/quant_large_cases.py reach these paths; the
tests here assert the launch geometry the library reports against the restatement there and print it."""
import numpy as np
import pytest

import geometry_util as gu
import quant_cases as qc
import quant_large_cases as lc
import quant_oracle as qo
import test_gpu_quant as tq
from oracle import oracle
from qldpc_amd import _lib

pytestmark = pytest.mark.gpu

QUANT = _lib.FLAG_QUANT
PIDS = {lc.Q4: "q4", lc.Q6: "q6", lc.Q8: "q8", lc.Q16: "q16"}
SLOT_OPTIONS = (0, 1, 3, 32)
MC_KW = dict(max_iter=lc.MAX_ITER, variant=_lib.MIN_SUM)


def check_geometry(dec, c, params, B, opt_slots=0, blocks_per_cu=0, what=""):
    """QBP_INFO_LDS_BYTES and QBP_INFO_GRID of the last launch against the restatement; prints (slots, grid, lds_bytes)."""
    S, grid, lds = lc.geometry(c.shape, lc.wide(params), B, dec.info("num_cu"), opt_slots, blocks_per_cu)
    print(f"{what}{c.tag} q{params[0]} B {B} option {opt_slots} per_cu {blocks_per_cu}: (slots, grid, lds_bytes) = "
          f"({S}, {dec.info('grid')}, {dec.info('lds_bytes')})")
    assert dec.info("last_kernel") == 5 and dec.info("threads") == lc.THREADS
    assert (dec.info("grid"), dec.info("lds_bytes")) == (grid, lds)
    return S, grid, lds


# ---- a. the batch build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("tag", lc.TAGS)
def test_batch_kernel_equals_statement_on_large_matrices(tag, kind):
    """int8 (two sets) and int16 messages, max_iter 1 and 12, automatic slots and QBP_OPT_QUANT_SLOTS 1, 3 and 32 -- on
    ph72x9 the last is lowered to 24 (int8) and 17 (int16) slots, above the 64 KiB a kernel gets without the attribute."""
    c = lc.case(tag)
    syn, prior = lc.batch_inputs(tag, kind)
    B = len(syn)
    dec = tq.fresh(c.H)
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = tq.Outputs(B, c.n)
    above = 0
    for params in lc.BATCH_PARAMS[tag]:
        dec.quant_configure(tq.cfg_of(params))
        for max_iter in (1, lc.MAX_ITER):
            want = lc.statement(tag, kind, params, max_iter)
            for opt in SLOT_OPTIONS:
                dec.set_option(_lib.OPT_QUANT_SLOTS, opt)
                got = out.run(dec, syn_t, prior_t, B, max_iter)
                tq.assert_same(got, want, f"{tag} {kind} {params} max_iter {max_iter} slots option {opt}")
                above += check_geometry(dec, c, params, B, opt)[2] > lc.LDS_DEFAULT
    assert above >= (4 if tag == "ph72x9" else 2)


@pytest.mark.parametrize("tag", lc.TAGS)
def test_batch_kernel_hands_out_records_beyond_the_grid_and_forced(tag):
    """One slot, one workgroup per CU, 2 num_cu + 5 records (the batch, tiled): every workgroup takes records from the
    work counter.  And QBP_FLAG_FORCE_FULL (rule 7: the outputs of the first converged iteration) on the batch."""
    c = lc.case(tag)
    syn, prior = lc.batch_inputs(tag, "mixed")
    dec = tq.fresh(c.H)
    cus = dec.info("num_cu")
    B = 2 * cus + 5
    rows = np.arange(B) % len(syn)
    syn_t, prior_t = gu.to_device(syn[rows]), gu.to_device(prior)
    out = tq.Outputs(B, c.n)
    for params in (lc.BATCH_PARAMS[tag][0], lc.Q16):
        dec.quant_configure(tq.cfg_of(params))
        want = lc.statement(tag, "mixed", params)
        dec.set_option(_lib.OPT_QUANT_SLOTS, 1)
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
        got = out.run(dec, syn_t, prior_t, B, lc.MAX_ITER)
        tq.assert_same(got, tuple(x[rows] for x in want), f"{tag} {params} tiled to {B}")
        S, grid, _ = check_geometry(dec, c, params, B, 1, 1, "tiled ")
        assert (S, grid) == (1, cus) and B > 2 * grid * S
        dec.set_option(_lib.OPT_QUANT_SLOTS, 0)
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)
        got = out.run(dec, syn_t, prior_t, lc.BATCH, lc.MAX_ITER, flags=_lib.FLAG_FORCE_FULL)
        tq.assert_same(got, want, f"{tag} {params} forced")
        check_geometry(dec, c, params, lc.BATCH, what="forced ")


# ---- b. Monte-Carlo counters and failure records --------------------------------------------------------------------------
def osd0_expectation(dec, c, errors, syn, out, rows=None):
    """Counters of statement -> qbp_osd_batch (OSD-0) on its failures with llr = (double)V -> numpy classification, summed
    over `rows` of the records (default: each once); and the number of failures among them."""
    hard, conv, iters, _, llr = out
    f = np.flatnonzero(~conv)
    det = hard.copy()
    det[f] = dec.osd0(syn[f], llr[f], hard[f])
    per_trial = lc.trial_counters(c, errors, syn, det, conv, iters)
    per_trial[f, 10] = (qc.syndromes_of(c.H, det[f]) != syn[f]).any(axis=1)
    rows = np.arange(len(errors)) if rows is None else rows
    return per_trial[rows].sum(axis=0), int((~conv[rows]).sum())


@pytest.mark.parametrize("params", lc.MC_PARAMS, ids=lambda p: PIDS[p])
@pytest.mark.parametrize("tag", lc.TAGS)
def test_mc_counters_and_failure_records_on_large_matrices(tag, params):
    """Both Monte-Carlo instantiations: the syndromes formed from the stored errors for rows beyond 256, the counters,
    and under QBP_FLAG_OSD0 the failure records (fail_syn of rows >= 256, fail_llr = (double)V) -- with automatic slots
    and with QBP_OPT_QUANT_SLOTS = 32."""
    c = lc.case(tag)
    prior = c.prior("noisy")
    out, want = lc.mc_statement(tag, params)
    dec = tq.fresh(c.H)
    dec.quant_configure(tq.cfg_of(params))
    want_osd, failures = osd0_expectation(dec, c, c.errors, c.syn, out)
    assert failures >= 4
    for opt in (0, 32):
        dec.set_option(_lib.OPT_QUANT_SLOTS, opt)
        got = dec.mc_run_errors(c.L, c.d, c.errors, prior, flags=QUANT, **MC_KW)
        print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
        assert np.array_equal(got, want), f"slots option {opt}"
        lds = check_geometry(dec, c, params, lc.BATCH, opt, what="mc ")[2]
        assert (lds > lc.LDS_DEFAULT) == (opt == 32 and (tag == "ph72x9" or lc.wide(params)))
        got = dec.mc_run_errors(c.L, c.d, c.errors, prior, flags=QUANT | _lib.FLAG_OSD0, **MC_KW)
        print("osd0", dict(zip(_lib.COUNTER_NAMES, got.tolist())))
        assert got[6] == failures
        assert np.array_equal(got, want_osd), f"OSD-0, slots option {opt}"
    # a split of the stored errors
    dec.set_option(_lib.OPT_QUANT_SLOTS, 0)
    parts = [dec.mc_run_errors(c.L, c.d, c.errors[a:b], prior, flags=QUANT, **MC_KW) for a, b in ((0, 17), (17, 48))]
    assert np.array_equal(parts[0] + parts[1], want)


# ---- c. Monte-Carlo slot refill ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("params", lc.MC_PARAMS, ids=lambda p: PIDS[p])
def test_mc_slots_take_further_trials_from_the_work_counter(params, S):
    """One workgroup per CU with S slots and 2 num_cu S + 5 stored errors (the pool of 192, tiled): every slot classifies
    a trial, clears its logical mask, error weight and difference flag, and decodes another; under QBP_FLAG_OSD0 a slot
    that wrote a failure record goes on with the next trial."""
    c = lc.case("refill")
    prior = c.prior("noisy")
    out, _ = lc.mc_statement("refill", params)
    dec = tq.fresh(c.H)
    dec.quant_configure(tq.cfg_of(params))
    cus = dec.info("num_cu")
    T = 2 * cus * S + 5
    rows = (np.arange(T) + 7 * S) % lc.REFILL_POOL
    errors = np.ascontiguousarray(c.errors[rows])
    want = lc.trial_counters(c, c.errors, c.syn, out[0], out[1], out[2])[rows].sum(axis=0)
    want_osd, failures = osd0_expectation(dec, c, c.errors, c.syn, out, rows)
    assert want[0] == T and failures >= 8
    dec.set_option(_lib.OPT_QUANT_SLOTS, S)
    dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
    got = dec.mc_run_errors(c.L, c.d, errors, prior, flags=QUANT, **MC_KW)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    grid = check_geometry(dec, c, params, T, S, 1, "refill ")[1]
    assert dec.info("grid") == cus == grid and T >= 2 * grid * S
    assert np.array_equal(got, want)
    half = T // 2
    parts = [dec.mc_run_errors(c.L, c.d, errors[a:b], prior, flags=QUANT, **MC_KW) for a, b in ((0, half), (half, T))]
    assert dec.info("grid") == cus
    assert np.array_equal(parts[0] + parts[1], want)
    got = dec.mc_run_errors(c.L, c.d, errors, prior, flags=QUANT | _lib.FLAG_OSD0, **MC_KW)
    print("osd0", dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[6] == failures
    assert np.array_equal(got, want_osd)


@pytest.mark.parametrize("params", lc.MC_PARAMS, ids=lambda p: PIDS[p])
def test_mc_sampled_entry_refills_its_slots(params):
    """qbp_mc_run_probs on its sampler's errors, three slots, one workgroup per CU: the whole range is one chunk longer
    than the grid; the range split in three gives the same counters."""
    c = lc.case("refill")
    prior = c.prior("noisy")
    probs = c.probs * 1.3
    S, begin, seed = 3, 5, 9
    dec = tq.fresh(c.H)
    dec.quant_configure(tq.cfg_of(params))
    cus = dec.info("num_cu")
    T = 2 * cus * S + 5
    errors = dec.mc_sample_errors_probs(probs, begin, T, seed=seed)
    syn = qc.syndromes_of(c.H, errors)
    hard, conv, iters, _, _ = qo.decode_batch_edges(c.H, syn, prior, lc.MAX_ITER, *params)
    want = oracle.classify_trials(c.H, c.L, c.d, errors, syn, hard, conv, iters)
    res = hard ^ errors
    assert (conv & res.any(axis=1)).sum() >= 8 and (~conv).sum() >= 8       # something for the resets to clear
    dec.set_option(_lib.OPT_QUANT_SLOTS, S)
    dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)

    def run(a, b):
        return dec.mc_run_probs(c.L, c.d, probs, prior, a, b, seed=seed, flags=QUANT, **MC_KW)

    got = run(begin, begin + T)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    grid = check_geometry(dec, c, params, T, S, 1, "sampled ")[1]
    assert grid == cus
    assert np.array_equal(got, want)
    third = T // 3
    assert np.array_equal(run(begin, begin + third) + run(begin + third, begin + 2 * third) + run(begin + 2 * third, begin + T),
                          want)
