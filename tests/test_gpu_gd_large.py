"""GPU: BP guided decimation's large build (QBP_OPT_GD_MEM: the messages of a record in a per-workgroup global
workspace, the working prior as two bit maps, V and the bookkeeping in LDS) against the numpy statement
(tests/gd_oracle.py) and against the LDS build, bit for bit, NaN equal to NaN, into poisoned buffers -- forced on the
small matrices of tests/test_gpu_gd.py and on the detector error model of record_kernel_util, chosen one round past the
LDS build's limit (41 rounds of the [[72,12,6]] phenomenological matrix for min-sum, 40 for sum-product); a workgroup
that reuses its slice of the workspace; the arg-max's tie rule; the records build behind QBP_FLAG_GD against the
composition of first-stage decode, statement and classification; the refusals; the Python layers."""
import functools

import numpy as np
import pytest

import large_util as lu
import gd_oracle as go
import geometry_util as gu
import record_kernel_util as ru
import test_gpu_gd as tg
import test_gpu_record_kernel_sizes as ts
from qldpc_amd import _lib, bp, gd, mc

pytestmark = pytest.mark.gpu

EXTRA = ("rounds",)
ITER_LIMIT = ts.GD_ITER_LIMIT
VIDS = tg.VIDS
SMALL = [c for c in tg.GD_CASES if c[0] != "144"]       # Steane, [[72,12,6]], the irregular 20 x 37 matrix, 36 x 74
BATCH_CASES = SMALL + ["dem_synth"]
ROUNDS = [6, "n"]


def fresh(H, mem=None):
    dec = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    if mem is not None:
        dec.set_option(_lib.OPT_GD_MEM, mem)
    return dec


def configure_raw(dec, cfg):
    """qbp_gd_configure without Decoder.gd_configure's option write: the handle's QBP_OPT_GD_MEM stays."""
    return _lib.load().qbp_gd_configure(dec._h, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant, cfg.alpha,
                                        cfg.clip_llr)


def with_large(cfg, large):
    return gd.GDConfig(cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant, cfg.alpha, cfg.clip_llr, large=large)


def statement(H, syn, prior, cfg):
    return go.gd_decode_batch(H, syn, prior, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant, cfg.alpha,
                              cfg.clip_llr)


@functools.lru_cache(maxsize=None)
def batch_inputs(case, variant, rounds):
    """(H, syndromes, prior, config, statement) of a case of test 1."""
    if case == "dem_synth":
        c, cfg, want = ts.gd_ref("dem_synth", variant, rounds)
        return c.H, c.syn, c.prior, cfg, want
    H, syn, prior = tg.inputs(*case)
    cfg = tg.config(variant, H.shape[1] if rounds == "n" else rounds)
    return H, syn, prior, cfg, statement(H, syn, prior, cfg)


def launch(dec, syn_t, prior_t, B, n, what, stream):
    out = ru.RecordOutputs(B, n, EXTRA)
    ru.gd_launch(dec, syn_t, prior_t, B, out, stream)
    return out.fetch_all(B, ITER_LIMIT, what)


def expected_info(sh, B, num_cu, variant, mem, blocks=0):
    sp = variant == _lib.SUM_PRODUCT
    if mem == lu.MEM_LARGE:
        return dict(threads=ru.gd_threads(sh), grid=lu.gd_large_grid(sh, B, num_cu, sp, blocks),
                    lds_bytes=lu.gd_large_lds_bytes(sh.m, sh.n, sp))
    return dict(threads=ru.gd_threads(sh), grid=ru.gd_grid(sh, B, num_cu, sp, blocks),
                lds_bytes=ru.gd_lds_bytes(sh.m, sh.n, sh.E, sp))


# ---- 1. the forced large build against the statement and against the LDS build ------------------------------------------
def test_statement_classes_are_present_in_the_batch_cases():
    pooled = {k: sum(go.classes(batch_inputs(c, v, r)[4])[k] for c in BATCH_CASES for v in tg.VARIANTS for r in ROUNDS)
              for k in ("round0", "later", "never")}
    print(pooled)
    assert all(v >= 8 for v in pooled.values()), pooled


@pytest.mark.parametrize("rounds", ROUNDS, ids=["six_rounds", "to_exhaustion"])
@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: c if isinstance(c, str) else f"{c[0]}-{c[1]}")
def test_forced_large_build_equals_statement_and_lds_build(case, variant, rounds):
    H, syn, prior, cfg, want = batch_inputs(case, variant, rounds)
    B, n, sh = len(syn), H.shape[1], ru.Shape(H)
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    got = {}
    for mem in (lu.MEM_LARGE, lu.MEM_LDS):
        dec = fresh(H, mem)
        assert configure_raw(dec, cfg) == 0
        what = f"gd {case} variant {variant} max_rounds {rounds} mem {mem}"
        ts.on_own_stream(lambda s: got.__setitem__(mem, launch(dec, syn_t, prior_t, B, n, what, s)))
        ru.assert_same(got[mem], ru.gd_want(want), what)
        info = ru.info(dec)
        print(what, info, go.classes(want))
        assert info == expected_info(sh, B, dec.info("num_cu"), variant, mem)
    ru.assert_same(got[lu.MEM_LARGE], got[lu.MEM_LDS], f"gd {case}: large build against LDS build")


# ---- 2. one round past the LDS build's limit -----------------------------------------------------------------------------
NEAR_B, NEAR_P = 8, 0.01


@functools.lru_cache(maxsize=None)
def past_limit(variant):
    """The first round count past gd_lds_bytes for the variant: 8 records, rounds of 4 iterations, 12 decimations."""
    T = lu.gd_first_rounds_beyond_the_lds_build(variant == _lib.SUM_PRODUCT)
    c = ru.phenomenological(T, NEAR_P, 200 + T, NEAR_B)
    cfg = gd.GDConfig(4, 12, tg.LLR, variant, tg.ALPHA, 20.0)
    return c, cfg, statement(c.H, c.syn, c.prior, cfg)


@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
def test_one_round_past_the_limit(variant):
    c, cfg, want = past_limit(variant)
    sh, sp = c.shape, variant == _lib.SUM_PRODUCT
    large_lds = lu.gd_large_lds_bytes(sh.m, sh.n, sp)
    assert ru.gd_lds_bytes(sh.m, sh.n, sh.E, sp) > ru.LDS_LIMIT > large_lds
    syn_t, prior_t = gu.to_device(c.syn), gu.to_device(c.prior)
    lib = _lib.load()
    # large=False: today's refusal, and no output is touched
    dec = fresh(c.H)
    with pytest.raises(_lib.QbpError) as e:
        dec.gd_configure(with_large(cfg, False))
    msg = lib.qbp_last_error()
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in msg and b"two rows of n doubles in LDS" in msg
    out = ru.RecordOutputs(NEAR_B, c.n, EXTRA)
    with pytest.raises(_lib.QbpError) as e:
        ru.gd_launch(dec, syn_t, prior_t, NEAR_B, out, gu.stream_ptr())
    assert e.value.code == _lib.E_INVALID and out.untouched()          # (nothing is configured on this handle)
    # large=True: the statement
    dec.gd_configure(with_large(cfg, True))
    what = f"gd variant {variant} T = {sh.m // 36}"
    got = launch(dec, syn_t, prior_t, NEAR_B, c.n, what, gu.stream_ptr())
    ru.assert_same(got, ru.gd_want(want), what)
    info = ru.info(dec)
    print(c.H.shape, info, go.classes(want), "rounds", want["rounds"].tolist())
    assert info == dict(threads=ru.gd_threads(sh), grid=NEAR_B, lds_bytes=large_lds)
    # a second, smaller launch on the same handle
    small = launch(dec, syn_t, prior_t, 3, c.n, what + ", B = 3", gu.stream_ptr())
    ru.assert_same(small, ru.gd_want(want, slice(0, 3)), what + ", B = 3")
    # the option set back after the configuration: the launch checks again, with today's message
    dec.set_option(_lib.OPT_GD_MEM, lu.MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        ru.gd_launch(dec, syn_t, prior_t, NEAR_B, out, gu.stream_ptr())
    msg = lib.qbp_last_error()
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in msg and b"two rows of n doubles in LDS" in msg
    assert out.untouched()
    # "auto", on a fresh handle: the large build, the statement
    auto = fresh(c.H)
    auto.gd_configure(with_large(cfg, "auto"))
    again = launch(auto, syn_t, prior_t, NEAR_B, c.n, what + " auto", gu.stream_ptr())
    ru.assert_same(again, ru.gd_want(want), what + " auto")
    assert ru.info(auto) == info


@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
def test_automatic_choice_keeps_the_lds_build_where_it_fits(variant):
    H, syn, prior, cfg, want = batch_inputs(("72", 0.1, 1), variant, 6)
    sh = ru.Shape(H)
    dec = fresh(H)
    dec.gd_configure(with_large(cfg, "auto"))
    got = launch(dec, gu.to_device(syn[:40]), gu.to_device(prior), 40, 72, "gd 72 auto", gu.stream_ptr())
    ru.assert_same(got, ru.gd_want(want, slice(0, 40)), "gd 72 auto")
    assert ru.info(dec) == expected_info(sh, 40, dec.info("num_cu"), variant, lu.MEM_LDS)


# ---- 3. more records than workgroups: a workgroup reuses its slice of the workspace ---------------------------------------
@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
def test_work_counter_with_the_messages_in_the_workspace(variant):
    other = _lib.MIN_SUM if variant == _lib.SUM_PRODUCT else _lib.SUM_PRODUCT
    H, syn, prior, cfg, ref = batch_inputs(("72", 0.1, 1), variant, 6)
    _, _, _, cfg_other, ref_other = batch_inputs(("72", 0.1, 1), other, 6)
    sh, n = ru.Shape(H), H.shape[1]
    dec = fresh(H, lu.MEM_LARGE)
    assert configure_raw(dec, cfg) == 0
    num_cu = dec.info("num_cu")
    B = 3 * 2 * num_cu + 37                   # three records and more per workgroup at one and at two workgroups per CU
    idx = ts.spread(B, 256, 5)
    syn_t, prior_t = gu.to_device(syn[idx]), gu.to_device(prior)
    got = {}
    for blocks in (1, 2):
        what = f"gd large variant {variant} blocks {blocks} B {B}"
        with gu.options(dec, blocks=blocks):
            ts.on_own_stream(lambda s: got.__setitem__(blocks, launch(dec, syn_t, prior_t, B, n, what, s)))
        info = ru.info(dec)
        print(what, info, go.classes(ref))
        assert info == expected_info(sh, B, num_cu, variant, lu.MEM_LARGE, blocks) and B >= 3 * info["grid"]
        assert info["grid"] == blocks * num_cu
        ru.assert_same(got[blocks], ru.gd_want(ref, idx), what)
    ru.assert_same(got[1], got[2], "gd large: one against two workgroups per CU")
    # the other variant on the same handle, at the automatic grid: the workspace is the handle's
    assert configure_raw(dec, cfg_other) == 0
    what = f"gd large variant {other} after {variant}"
    second = launch(dec, syn_t, prior_t, B, n, what, gu.stream_ptr())
    assert ru.info(dec) == expected_info(sh, B, num_cu, other, lu.MEM_LARGE)
    ru.assert_same(second, ru.gd_want(ref_other, idx), what)
    # and the first one again
    assert configure_raw(dec, cfg) == 0
    third = launch(dec, syn_t, prior_t, B, n, what + " and back", gu.stream_ptr())
    ru.assert_same(third, got[1], what + " and back")


# ---- 4. exact ties in |V|: the lowest original index --------------------------------------------------------------------
@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
def test_tied_posteriors_go_to_the_lowest_index(variant):
    H, syn, prior = tg.inputs("72", 0.1, 1)
    assert np.all(prior == prior[0])
    cfg = tg.config(variant, 6, T=2)
    want = statement(H, syn, prior, cfg)
    # the condition on the inputs: after the first round, records whose largest |V| is shared by several candidates
    first = statement(H, syn, prior, tg.config(variant, 0, T=2))
    a = np.abs(first["llr"][~first["converged"]])
    tied = int(((a == a.max(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())
    print("records with a tied maximum after round 0:", tied, "of", len(a), go.classes(want))
    assert tied >= 8
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    got = {}
    for mem in (lu.MEM_LARGE, lu.MEM_LDS):
        dec = fresh(H, mem)
        assert configure_raw(dec, cfg) == 0
        got[mem] = launch(dec, syn_t, prior_t, len(syn), 72, f"gd ties mem {mem}", gu.stream_ptr())
        assert np.array_equal(got[mem][4], want["rounds"]) and np.array_equal(got[mem][0], want["hard"])
        ru.assert_same(got[mem], ru.gd_want(want), f"gd ties mem {mem}")
    ru.assert_same(got[lu.MEM_LARGE], got[lu.MEM_LDS], "gd ties: large build against LDS build")


# ---- 5. the records build behind QBP_FLAG_GD ----------------------------------------------------------------------------
FIRST = ["sum_product", "min_sum", "layered", "layered_large"]


def first_stage(dec, first):
    """(variant, layered) of a first stage; configures the layered ones (layered_large: its messages in global memory)."""
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    layered = first.startswith("layered")
    if layered:
        dec.layered_configure(None)
        dec.set_option(_lib.OPT_LAYERED_MEM, 1 if first == "layered_large" else 0)
    return variant, layered


@pytest.mark.parametrize("first", FIRST)
def test_mc_run_errors_equals_the_composition_and_the_lds_build(first):
    H, L, d = tg.matrix("72")
    L = np.ascontiguousarray(L, np.uint8)
    errors = (np.random.default_rng(17).random((400, 72)) < 0.08).astype(np.uint8)
    prior = mc.prior_of(0.08, 72)
    # the second stage's variant is the configuration's own: the other one than the first stage's, both get covered
    cfg = tg.config(_lib.SUM_PRODUCT if first == "min_sum" else _lib.MIN_SUM, 6)
    got = {}
    for mem in (lu.MEM_LARGE, lu.MEM_LDS):
        dec = fresh(H, mem)
        assert configure_raw(dec, cfg) == 0
        variant, layered = first_stage(dec, first)
        kw = dict(max_iter=tg.MC_ITERS, variant=variant, alpha=tg.ALPHA,
                  flags=_lib.FLAG_GD | (_lib.FLAG_LAYERED if layered else 0))
        got[mem] = dec.mc_run_errors(L, d, errors, prior, **kw)
        assert dec.info("lds_bytes") == expected_info(ru.Shape(H), 1, 1, cfg.variant, mem)["lds_bytes"]
        parts = dec.mc_run_errors(L, d, errors[:150], prior, **kw) + dec.mc_run_errors(L, d, errors[150:], prior, **kw)
        assert np.array_equal(parts, got[mem])
    want, failures = tg.compose(dec, H, L, d, errors, prior, cfg, variant, layered)
    print(first, dict(zip(_lib.COUNTER_NAMES, got[lu.MEM_LARGE].tolist())), "failures", failures)
    assert failures >= 8 and want[6] == failures and want[0] == len(errors)
    assert np.array_equal(got[lu.MEM_LARGE], want)
    assert np.array_equal(got[lu.MEM_LARGE], got[lu.MEM_LDS])


DEM_TRIALS, DEM_SEED, DEM_RATE = 256, 9, 5.0


@pytest.mark.parametrize("first", ["sum_product", "layered"])
def test_mc_run_probs_on_the_detector_error_model(first):
    c = ru.case("dem_synth")
    L = np.ascontiguousarray(c.L, np.uint8)
    probs = np.minimum(0.5, c.probs * DEM_RATE)
    cfg = tg.config(_lib.MIN_SUM if first == "sum_product" else _lib.SUM_PRODUCT, 6)
    got = {}
    for mem in (lu.MEM_LARGE, lu.MEM_LDS):
        dec = fresh(c.H, mem)
        assert configure_raw(dec, cfg) == 0
        variant, layered = first_stage(dec, first)
        kw = dict(seed=DEM_SEED, max_iter=tg.MC_ITERS, variant=variant, alpha=tg.ALPHA,
                  flags=_lib.FLAG_GD | (_lib.FLAG_LAYERED if layered else 0))
        got[mem] = dec.mc_run_probs(L, 0, probs, c.prior, 0, DEM_TRIALS, **kw)
        assert dec.info("lds_bytes") == expected_info(c.shape, 1, 1, cfg.variant, mem)["lds_bytes"]
        parts = dec.mc_run_probs(L, 0, probs, c.prior, 0, 77, **kw) + dec.mc_run_probs(L, 0, probs, c.prior, 77, DEM_TRIALS, **kw)
        assert np.array_equal(parts, got[mem])
    errors = dec.mc_sample_errors_probs(probs, 0, DEM_TRIALS, seed=DEM_SEED)
    want, failures = tg.compose(dec, c.H, L, 0, errors, c.prior, cfg, variant, layered)
    print(first, dict(zip(_lib.COUNTER_NAMES, got[lu.MEM_LARGE].tolist())), "failures", failures)
    assert failures >= 8 and got[lu.MEM_LARGE][0] == DEM_TRIALS and got[lu.MEM_LARGE][6] == failures
    assert np.array_equal(got[lu.MEM_LARGE], want)
    assert np.array_equal(got[lu.MEM_LARGE], got[lu.MEM_LDS])


def test_run_dem_takes_large():
    c = ru.case("dem_synth")
    probs = np.minimum(0.5, c.probs * DEM_RATE)
    cfg = tg.config(_lib.MIN_SUM, 6)
    kw = dict(seed=DEM_SEED, max_iter=tg.MC_ITERS)
    settings = dict(iters_per_round=cfg.iters_per_round, max_rounds=cfg.max_rounds, decim_llr=cfg.decim_llr,
                    variant=cfg.variant, alpha=cfg.alpha, clip_llr=cfg.clip_llr)
    got = mc.run_dem(c.H, c.L, probs, DEM_TRIALS, prior=c.prior, gd=dict(settings, large=True), **kw)
    lds = mc.run_dem(c.H, c.L, probs, DEM_TRIALS, prior=c.prior, gd=settings, **kw)
    dec = fresh(c.H)
    dec.gd_configure(with_large(cfg, True))
    direct = dec.mc_run_probs(np.ascontiguousarray(c.L, np.uint8), 0, probs, c.prior, 0, DEM_TRIALS, flags=_lib.FLAG_GD, **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), ru.info(dec))
    assert dec.info("lds_bytes") == lu.gd_large_lds_bytes(c.shape.m, c.shape.n, False)
    assert got[0] == DEM_TRIALS and got[6] >= 8
    assert np.array_equal(got, direct) and np.array_equal(got, lds)


def test_mc_past_the_limit_is_refused_without_the_option_and_runs_with_it():
    c, cfg, _ = past_limit(_lib.MIN_SUM)
    L = np.ascontiguousarray(c.L, np.uint8)
    # (at p = 0.03 a trial has 130 errors among 4428 columns: 8 iterations of BP leave nearly all of them)
    errors = ru.draw([np.full(c.n, 0.03)], 24, np.random.default_rng(31))
    dec = fresh(c.H)
    dec.gd_configure(with_large(cfg, True))
    kw = dict(max_iter=tg.MC_ITERS, alpha=tg.ALPHA, flags=_lib.FLAG_GD)
    got = dec.mc_run_errors(L, 6, errors, c.prior, **kw)
    assert dec.info("lds_bytes") == lu.gd_large_lds_bytes(c.shape.m, c.shape.n, False)
    want, failures = tg.compose(dec, c.H, L, 6, errors, c.prior, cfg, _lib.SUM_PRODUCT, False)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), "failures", failures)
    assert failures >= 8 and got[6] == failures and np.array_equal(got, want)
    # without the option the Monte-Carlo call is refused before any GPU work
    dec.set_option(_lib.OPT_GD_MEM, lu.MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_errors(L, 6, errors, c.prior, **kw)
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in _lib.load().qbp_last_error()


# ---- 6. the upper refusal (host only) and the option's range ----------------------------------------------------------------
def one_check(n):
    H = np.zeros((1, n), np.uint8)
    H[0, :5] = 1
    return H


@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
def test_upper_refusal_and_option_range(variant):
    lib = _lib.load()
    sp = variant == _lib.SUM_PRODUCT
    n = lu.first_n_beyond_the_limit(lambda n: lu.gd_large_lds_bytes(1, n, sp))
    assert n == (19466 if sp else 19839)
    dec = fresh(one_check(n))
    out = ru.RecordOutputs(2, n, EXTRA)
    syn_t, prior_t = gu.to_device(np.zeros((2, 1), np.uint8)), gu.to_device(np.ones(n))
    for large in (True, "auto"):
        with pytest.raises(_lib.QbpError) as e:
            dec.gd_configure(gd.GDConfig(4, 2, tg.LLR, variant, large=large))
        msg = lib.qbp_last_error()
        assert e.value.code == _lib.E_UNSUPPORTED
        assert b"global memory" in msg and str(lu.gd_large_lds_bytes(1, n, sp)).encode() in msg and b"160 KiB" in msg
        with pytest.raises(_lib.QbpError) as e:             # nothing was configured: no launch
            ru.gd_launch(dec, syn_t, prior_t, 2, out, gu.stream_ptr())
        assert e.value.code == _lib.E_INVALID and out.untouched()
    # one column fewer fits
    fits = fresh(one_check(n - 1))
    fits.gd_configure(gd.GDConfig(4, 2, tg.LLR, variant, large="auto"))
    # the option's range
    for bad in (3, -1):
        with pytest.raises(_lib.QbpError) as e:
            dec.set_option(_lib.OPT_GD_MEM, bad)
        assert e.value.code == _lib.E_INVALID
    for ok in (0, 1, 2):
        dec.set_option(_lib.OPT_GD_MEM, ok)


# ---- 7. the Python layers --------------------------------------------------------------------------------------------------
def test_perform_bpgd_takes_large():
    c, cfg, want = past_limit(_lib.MIN_SUM)
    args = (cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant, cfg.alpha, cfg.clip_llr)
    r = gd.performBPGDBatch(c.H, c.syn, c.prior, *args, large=True)
    ru.assert_same(tuple(r), ru.gd_want(want), "performBPGDBatch past the limit")
    hard, conv, llr, iters = gd.performBPGD(c.H, c.syn[0], c.prior, *args, large="auto")
    assert np.array_equal(hard, want["hard"][0]) and conv == bool(want["converged"][0]) and iters == want["iters"][0]
    assert go.same(llr, want["llr"][0])
    with pytest.raises(_lib.QbpError) as e:
        gd.performBPGDBatch(c.H, c.syn, c.prior, *args)
    assert e.value.code == _lib.E_UNSUPPORTED
