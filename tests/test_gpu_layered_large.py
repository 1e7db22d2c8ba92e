"""GPU: layered BP's large build (QBP_OPT_LAYERED_MEM: the messages of every slot in the workgroup's slice of a global
workspace, V, the syndrome bits and the slot words in LDS) against the numpy statement (tests/layered_oracle.py) and
against the LDS build, bit for bit, NaN equal to NaN, into poisoned buffers -- forced on the small matrices of
tests/test_gpu_layered.py and on the detector error model of record_kernel_util, and chosen automatically one round past
the LDS build's limit (40 rounds of the [[72,12,6]] phenomenological matrix, 1440 x 4320); slot reuse with more records
than slots; QBP_FLAG_FORCE_FULL; the Monte-Carlo build alone and under OSD-0 and Relay-BP; the refusals; the Python
layers."""
import functools

import numpy as np
import pytest

import geometry_util as gu
import large_util as lu
import layered_oracle as lo
import record_kernel_util as ru
import test_gpu_layered as tl
import test_gpu_record_kernel_sizes as ts
from oracle import oracle
from qldpc_amd import _lib, bp, layered, mc

pytestmark = pytest.mark.gpu

LAYERED = _lib.FLAG_LAYERED
VARIANTS, VIDS = tl.VARIANTS, ["sum_product", "min_sum"]
KINDS = ("default", "random")
SMALL = ["steane", "72", "irr37", "disjoint70"]
ITERS = (1, 2, 50)


def fresh(H, mem=None):
    dec = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    if mem is not None:
        dec.set_option(_lib.OPT_LAYERED_MEM, mem)
    return dec


def configure_raw(dec, order):
    """qbp_layered_configure alone: the handle's QBP_OPT_LAYERED_MEM stays (as Decoder.layered_configure(order))."""
    oin = None if order is None else np.ascontiguousarray(order, np.int32)
    return _lib.load().qbp_layered_configure(dec._h, 0 if oin is None else oin.ctypes.data)


@functools.lru_cache(maxsize=None)
def batch_inputs(name):
    """(H, syndromes, prior) of a case of test 1."""
    if name == "dem_synth":
        c = ru.case("dem_synth")
        return c.H, c.syn, c.prior
    H, _, syn, prior = tl.case(name)
    return H, syn, prior


@functools.lru_cache(maxsize=None)
def batch_statement(name, kind, variant, alpha, max_iter):
    if name != "dem_synth":
        return tl.statement(name, kind, variant, alpha, max_iter)
    H, syn, prior = batch_inputs(name)
    return lo.layered_decode_batch(H, syn, prior, max_iter, variant, alpha, 20.0, lo.order_of(H, kind), "level")


def expected_info(sh, width, B, tables, slots, large, num_cu, blocks=0):
    S = lu.layered_slots(sh, width, B, tables, slots, large)
    return S, dict(threads=ru.LAYERED_THREADS, grid=lu.layered_grid(sh, S, B, num_cu, tables, large, blocks),
                   lds_bytes=lu.layered_build_lds(sh, S, tables, large))


# ---- 1. the forced large build against the statement and against the LDS build ------------------------------------------
def test_dem_synth_has_rows_beyond_eight():
    sh = ru.Shape(batch_inputs("dem_synth")[0])
    assert sh.long_rows >= 1                            # (the two-pass loop of the level step runs)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SMALL + ["dem_synth"])
def test_forced_large_build_equals_statement_and_lds_build(name, kind):
    H, syn, prior = batch_inputs(name)
    B, n, sh = len(syn), H.shape[1], ru.Shape(H)
    order = lo.order_of(H, kind)
    width = max(ru.level_widths(H, order))
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = gu.Outputs(B, n)
    decs = {mem: fresh(H, mem) for mem in (lu.MEM_LARGE, lu.MEM_LDS)}
    for dec in decs.values():
        assert configure_raw(dec, order) == 0
    num_cu = decs[lu.MEM_LDS].info("num_cu")
    for variant, alpha in VARIANTS:
        tables = variant == _lib.SUM_PRODUCT
        for max_iter in ITERS:
            want = batch_statement(name, kind, variant, alpha, max_iter)
            for slots in (1, 2, 0):
                got = {}
                for mem, dec in decs.items():
                    what = f"layered {name} {kind} variant {variant} max_iter {max_iter} slots {slots} mem {mem}"
                    with ts.layered_slots_option(dec, slots):
                        got[mem] = gu.decode(dec, syn_t, prior_t, B, out, what, max_iter=max_iter, variant=variant,
                                             alpha=alpha, flags=LAYERED)
                    gu.assert_same(got[mem], want, what)
                    assert dec.info("last_kernel") == 4
                    S, info = expected_info(sh, width, B, tables, slots, mem == lu.MEM_LARGE, num_cu)
                    assert ru.info(dec) == info, (what, S, ru.info(dec), info)
                gu.assert_same(got[lu.MEM_LARGE], got[lu.MEM_LDS], f"{name} {kind}: large build against LDS build")
    print(name, kind, "widest level", width, ru.info(decs[lu.MEM_LARGE]), ru.info(decs[lu.MEM_LDS]))


def test_automatic_choice_keeps_the_lds_build_where_it_fits():
    H, syn, prior = batch_inputs("72")
    sh = ru.Shape(H)
    assert not lu.layered_auto_is_large(sh)
    dec = fresh(H)
    dec.layered_configure(None, large=True)
    out = gu.Outputs(40, 72)
    got = gu.decode(dec, gu.to_device(syn[:40]), gu.to_device(prior), 40, out, "72 auto", variant=_lib.MIN_SUM, alpha=0.8,
                    flags=LAYERED)
    gu.assert_same(got, tuple(x[:40] for x in tl.statement("72", "default", _lib.MIN_SUM, 0.8, 50)), "72 auto")
    width = max(ru.level_widths(H, lo.order_of(H, "default")))
    assert ru.info(dec) == expected_info(sh, width, 40, False, 0, False, dec.info("num_cu"))[1]


# ---- 2. one round past the LDS build's limit -----------------------------------------------------------------------------
ROUNDS, PAST_B, PAST_ITERS = 40, 8, 12
PAST_FIRST = {"sum_product": [1, 4, 2, 1, 1, None, 4, 2], "min_sum": [1, 3, 2, 1, 2, None, None, 2]}


@functools.lru_cache(maxsize=None)
def past_limit():
    c = ru.phenomenological(ROUNDS, 0.01, 139, PAST_B)
    assert c.H.shape == (1440, 4320) and c.shape.E == 11484
    return c


@functools.lru_cache(maxsize=None)
def past_order(kind):
    """The default order by qbp_layered_plan (host only; the numpy colouring takes H H^T), or the seeded random one."""
    c = past_limit()
    return layered.layered_order(c.H)[0] if kind == "default" else lo.order_of(c.H, "random")


@functools.lru_cache(maxsize=None)
def past_statement(kind, variant, alpha):
    c = past_limit()
    return lo.layered_decode_batch(c.H, c.syn, c.prior, PAST_ITERS, variant, alpha, 20.0, past_order(kind), "level")


def past_launch(dec, syn_t, prior_t, B, out, variant, alpha, what):
    return gu.decode(dec, syn_t, prior_t, B, out, what, max_iter=PAST_ITERS, variant=variant, alpha=alpha, flags=LAYERED)


def test_one_round_past_the_limit():
    c = past_limit()
    sh = c.shape
    assert ru.layered_lds_bytes(sh.m, sh.n, sh.E, 1, True) > ru.LDS_LIMIT > lu.layered_large_lds_bytes(sh.m, sh.n, 1, True)
    widths = {k: ru.level_widths(c.H, past_order(k)) for k in KINDS}
    print({k: (len(w), max(w)) for k, w in widths.items()})
    assert widths["default"] == [360] * 4 and len(widths["random"]) == 28      # (360 > 256 threads: two passes a level)
    # the statement's own classes in the default order: satisfied at the earliest iteration any record is, later, never
    # (`iters` as the statement returns it, 0-based: no record of this batch is satisfied after the very first pass)
    for (variant, alpha), vid in zip(VARIANTS, VIDS):
        _, conv, iters, _ = past_statement("default", variant, alpha)
        first = [int(i) if ok else None for ok, i in zip(conv, iters)]
        print(vid, "first satisfied in iteration", first)
        assert first == PAST_FIRST[vid]
        assert (conv & (iters == 1)).any() and (conv & (iters > 1)).any() and (~conv).any()
    syn_t, prior_t = gu.to_device(c.syn), gu.to_device(c.prior)
    out = gu.Outputs(PAST_B, c.n)
    out.poison()
    # mode 0: today's refusal, and no output is touched
    dec = fresh(c.H)
    with pytest.raises(_lib.QbpError) as e:
        dec.layered_configure(None, large=False)
    msg = _lib.load().qbp_last_error()
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in msg and b"the prior of a record in LDS" in msg
    with pytest.raises(_lib.QbpError) as e:
        gu.launch(dec, syn_t, prior_t, PAST_B, out, max_iter=PAST_ITERS, flags=LAYERED)
    assert e.value.code == _lib.E_INVALID                       # (nothing is configured on this handle)
    gu.torch().cuda.synchronize()
    assert all(out.poisoned(k, 0) for k in gu.NAMES)
    num_cu = dec.info("num_cu")
    for kind in KINDS:
        dec.layered_configure(past_order(kind), large=True)
        for variant, alpha in VARIANTS:
            want = past_statement(kind, variant, alpha)
            what = f"layered T = 40 {kind} variant {variant}"
            gu.assert_same(past_launch(dec, syn_t, prior_t, PAST_B, out, variant, alpha, what), want, what)
            tables = variant == _lib.SUM_PRODUCT
            S, info = expected_info(sh, max(widths[kind]), PAST_B, tables, 0, True, num_cu)
            print(what, ru.info(dec), "S", S, "converged", int(want[1].sum()))
            assert ru.info(dec) == info
            # a second, smaller launch on the same handle
            small = past_launch(dec, syn_t, prior_t, 3, out, variant, alpha, what + ", B = 3")
            gu.assert_same(small, tuple(x[:3] for x in want), what + ", B = 3")
    # the option set back after the configuration: every launch checks again, with today's message
    variant, alpha = VARIANTS[1]
    dec.set_option(_lib.OPT_LAYERED_MEM, lu.MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        gu.launch(dec, syn_t, prior_t, PAST_B, out, max_iter=PAST_ITERS, variant=variant, alpha=alpha, flags=LAYERED)
    msg = _lib.load().qbp_last_error()
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in msg and b"the prior of a record in LDS" in msg
    gu.torch().cuda.synchronize()
    assert all(out.poisoned(k, 0) for k in gu.NAMES)
    dec.set_option(_lib.OPT_LAYERED_MEM, lu.MEM_AUTO)
    again = past_launch(dec, syn_t, prior_t, PAST_B, out, variant, alpha, "layered T = 40 again")
    gu.assert_same(again, past_statement("random", variant, alpha), "layered T = 40 again")


# ---- 3. more records than slots: a slot reuses its slice of the workspace -------------------------------------------------
@pytest.mark.parametrize("slots", [1, 3])
def test_more_records_than_slots(slots):
    H, syn, prior = batch_inputs("72")
    sh, n, base = ru.Shape(H), H.shape[1], len(syn)
    width = max(ru.level_widths(H, lo.order_of(H, "default")))
    dec = fresh(H, lu.MEM_LARGE)
    assert configure_raw(dec, None) == 0
    prior_t = gu.to_device(prior)
    num_cu = dec.info("num_cu")

    def run(variant, alpha, S_opt, B):
        tables = variant == _lib.SUM_PRODUCT
        want = tl.statement("72", "default", variant, alpha, 50)
        idx = ts.spread(B, base, 7)
        syn_t = gu.to_device(syn[idx])
        out = gu.Outputs(B, n)
        what = f"layered large 72 variant {variant} slots {S_opt} B {B}"
        with gu.options(dec, blocks=1), ts.layered_slots_option(dec, S_opt):
            ts.on_own_stream(lambda s: gu.launch(dec, syn_t, prior_t, B, out, variant=variant, alpha=alpha, flags=LAYERED))
        got = out.fetch(B, 50, what)
        S, info = expected_info(sh, width, B, tables, S_opt, True, num_cu, blocks=1)
        print(what, ru.info(dec), "S", S)
        assert S == S_opt and ru.info(dec) == info
        gu.assert_same(got, tuple(x[idx] for x in want), what)
        return info["grid"]

    for variant, alpha in VARIANTS:
        assert run(variant, alpha, slots, 37) == -(-37 // slots)
        B = 2 * num_cu * slots + 5
        assert run(variant, alpha, slots, B) == num_cu and B > num_cu * slots      # every slot takes a third record
        # another S on the same handle: the slices move, the workspace grows
        run(variant, alpha, slots + 2, B)
        run(variant, alpha, slots, 37)


# ---- 4. QBP_FLAG_FORCE_FULL ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72", "irr37"])
def test_force_full_returns_the_early_exit_bits(name):
    H, syn, prior = batch_inputs(name)
    B, n = len(syn), H.shape[1]
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = gu.Outputs(B, n)
    decs = {mem: fresh(H, mem) for mem in (lu.MEM_LARGE, lu.MEM_LDS)}
    for dec in decs.values():
        assert configure_raw(dec, None) == 0
    for variant, alpha in VARIANTS:
        for max_iter in (1, 50):
            want = tl.statement(name, "default", variant, alpha, max_iter)
            got = {}
            for mem, dec in decs.items():
                what = f"{name} forced variant {variant} max_iter {max_iter} mem {mem}"
                got[mem] = gu.decode(dec, syn_t, prior_t, B, out, what, max_iter=max_iter, variant=variant, alpha=alpha,
                                     flags=LAYERED | _lib.FLAG_FORCE_FULL)
                gu.assert_same(got[mem], want, what)
            gu.assert_same(got[lu.MEM_LARGE], got[lu.MEM_LDS], f"{name} forced: large build against LDS build")


# ---- 5. the Monte-Carlo build ------------------------------------------------------------------------------------------------
MC_ITERS = tl.MC_ITERS


@functools.lru_cache(maxsize=None)
def mc_inputs(name):
    """(H, L, distance, errors, prior)"""
    if name == "dem_synth":
        return ts.mc_case("dem_synth")
    H, errors, _, prior = tl.case(name)
    L, d = tl.logicals(name)
    return H, np.ascontiguousarray(L, np.uint8), d, errors, prior


@functools.lru_cache(maxsize=None)
def mc_statement(name, variant, alpha):
    H, L, d, errors, prior = mc_inputs(name)
    syn = gu.syndromes_of(H, errors)
    hard, conv, iters, llr = lo.layered_decode_batch(H, syn, prior, MC_ITERS, variant, alpha, 20.0, None, "level")
    return syn, hard, conv, iters, llr


def mc_decoders(H):
    decs = {mem: fresh(H, mem) for mem in (lu.MEM_LARGE, lu.MEM_LDS)}
    for dec in decs.values():
        assert configure_raw(dec, None) == 0
    return decs


@pytest.mark.parametrize("variant,alpha", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("name", ["72", "dem_synth"])
def test_mc_run_errors_equals_statement_and_the_lds_build(name, variant, alpha):
    H, L, d, errors, prior = mc_inputs(name)
    syn, hard, conv, iters, _ = mc_statement(name, variant, alpha)
    want = oracle.classify_trials(H, L, d, errors, syn, hard, conv, iters)
    failures = int((~conv).sum())
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=alpha, flags=LAYERED)
    got = {}
    sh = ru.Shape(H)
    width = max(ru.level_widths(H, lo.order_of(H, "default")))
    for mem, dec in mc_decoders(H).items():
        got[mem] = dec.mc_run_errors(L, d, errors, prior, **kw)
        assert dec.info("last_kernel") == 4
        info = expected_info(sh, width, len(errors), variant == _lib.SUM_PRODUCT, 0, mem == lu.MEM_LARGE, dec.info("num_cu"))[1]
        assert ru.info(dec) == info
        assert np.array_equal(dec.mc_run_errors(L, d, errors[:31], prior, **kw)
                              + dec.mc_run_errors(L, d, errors[31:], prior, **kw), got[mem])
        with ts.layered_slots_option(dec, 1):
            assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, **kw), got[mem])
    print(name, dict(zip(_lib.COUNTER_NAMES, got[lu.MEM_LARGE].tolist())), "failures", failures)
    assert 8 <= failures < len(errors)
    assert np.array_equal(got[lu.MEM_LARGE], want)
    assert np.array_equal(got[lu.MEM_LARGE], got[lu.MEM_LDS])


@pytest.mark.parametrize("stage", ["osd0", "relay"])
@pytest.mark.parametrize("name", ["72", "dem_synth"])
def test_second_stages_act_on_the_large_builds_failure_records(name, stage):
    """Counters = the statement's first stage -> qbp_osd_batch / qbp_relay_decode_batch on its failures -> numpy
    classification, for both builds."""
    H, L, d, errors, prior = mc_inputs(name)
    variant, alpha = VARIANTS[0]
    syn, hard, conv, iters, llr = mc_statement(name, variant, alpha)
    f = np.flatnonzero(~conv)
    assert len(f) >= 8
    decs = mc_decoders(H)
    det = hard.copy()
    helper = decs[lu.MEM_LDS]
    if stage == "relay":
        cfg = tl.relay_config(H.shape[1])
        for dec in decs.values():
            dec.relay_configure(cfg)
        r_hard, r_conv = helper.relay_decode(syn[f], prior, cfg)[:2]
        det[f] = r_hard
        invalid = int((~r_conv).sum())
        flags = LAYERED | _lib.FLAG_RELAY
    else:
        det[f] = helper.osd0(syn[f], llr[f], hard[f])
        invalid = int((gu.syndromes_of(H, det[f]) != syn[f]).any(1).sum())
        flags = LAYERED | _lib.FLAG_OSD0
    want = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    want[10] = invalid
    got = {mem: dec.mc_run_errors(L, d, errors, prior, max_iter=MC_ITERS, variant=variant, alpha=alpha, flags=flags)
           for mem, dec in decs.items()}
    print(name, stage, dict(zip(_lib.COUNTER_NAMES, got[lu.MEM_LARGE].tolist())))
    assert got[lu.MEM_LARGE][6] == len(f)
    assert np.array_equal(got[lu.MEM_LARGE], want)
    assert np.array_equal(got[lu.MEM_LARGE], got[lu.MEM_LDS])


@pytest.mark.parametrize("name", ["72", "dem_synth"])
def test_mc_run_weight_does_not_depend_on_the_build_the_split_or_the_chunk(name):
    H, L, d, _, prior = mc_inputs(name)
    n = H.shape[1]
    T, w = 96, max(2, n // 14)
    variant, alpha = VARIANTS[1]
    kw = dict(seed=9, max_iter=MC_ITERS, variant=variant, alpha=alpha, flags=LAYERED)
    decs = mc_decoders(H)
    errors = decs[lu.MEM_LDS].mc_sample_errors_weight(w, 5, T, seed=9)
    syn = gu.syndromes_of(H, errors)
    hard, conv, iters, _ = lo.layered_decode_batch(H, syn, prior, MC_ITERS, variant, alpha, 20.0, None, "level")
    want = oracle.classify_trials(H, L, d, errors, syn, hard, conv, iters)
    for mem, dec in decs.items():
        run = lambda a, b: dec.mc_run_weight(L, d, w, prior, a, b, **kw)
        assert np.array_equal(run(5, 5 + T), want), mem
        assert np.array_equal(run(5, 6) + run(6, 50) + run(50, 5 + T), want), mem
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 7)
        assert np.array_equal(run(5, 5 + T), want), mem
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)


# ---- 6. the upper refusal (host only) and the option's range ----------------------------------------------------------------
def one_check(n):
    H = np.zeros((1, n), np.uint8)
    H[0, :5] = 1
    return H


def test_upper_refusal_and_option_range():
    lib = _lib.load()
    limit = lu.layered_n_limit(1)
    n = limit + 1
    for mem in (lu.MEM_AUTO, lu.MEM_LARGE):
        dec = fresh(one_check(n), mem)
        rc = configure_raw(dec, None)
        msg = lib.qbp_last_error()
        assert rc == _lib.E_UNSUPPORTED
        assert b"global memory" in msg and str(lu.layered_large_lds_bytes(1, n, 1, True)).encode() in msg
        assert b"160 KiB" in msg and f"n <= {limit}".encode() in msg
    out = gu.Outputs(2, n)
    out.poison()
    with pytest.raises(_lib.QbpError) as e:             # nothing was configured: no launch
        gu.launch(dec, gu.to_device(np.zeros((2, 1), np.uint8)), gu.to_device(np.ones(n)), 2, out, flags=LAYERED)
    assert e.value.code == _lib.E_INVALID
    gu.torch().cuda.synchronize()
    assert all(out.poisoned(k, 0) for k in gu.NAMES)
    # the widest matrix the option accepts configures; without the option it is refused as ever
    dec = fresh(one_check(limit))
    dec.layered_configure(None, large=True)
    dec.set_option(_lib.OPT_LAYERED_MEM, lu.MEM_LDS)
    counters = np.full(12, 7, np.int64)
    Lx = np.zeros((1, limit), np.uint8)
    Lx[0, 0] = 1
    prior = np.ones(limit)
    rc = lib.qbp_mc_run(dec._h, Lx.ctypes.data, 1, 0, 0.001, 1, 0, 0, 50, prior.ctypes.data, 4, 0, 1.0, 1.0, 20.0,
                        LAYERED, counters.ctypes.data)
    msg = lib.qbp_last_error()
    assert rc == _lib.E_UNSUPPORTED and np.all(counters == 7) and b"160 KiB" in msg and b"global memory" not in msg
    for bad in (3, -1):
        with pytest.raises(_lib.QbpError) as e:
            dec.set_option(_lib.OPT_LAYERED_MEM, bad)
        assert e.value.code == _lib.E_INVALID
    for ok in (0, 1, 2):
        dec.set_option(_lib.OPT_LAYERED_MEM, ok)


# ---- 7. the Python layers --------------------------------------------------------------------------------------------------
def test_perform_layered_bp_takes_large():
    c = past_limit()
    variant, alpha = VARIANTS[1]
    want = past_statement("random", variant, alpha)
    order = past_order("random")
    got = layered.performLayeredBPBatch(c.H, c.syn, c.prior, PAST_ITERS, "min-sum", alpha, order=order, large=True)
    gu.assert_same(got, want, "performLayeredBPBatch T = 40")
    hard, conv, llr, it = layered.performLayeredBP(c.H, c.syn[1], c.prior, PAST_ITERS, "min-sum", alpha, order=order,
                                                   large=True)
    assert np.array_equal(hard, want[0][1]) and conv == bool(want[1][1]) and it == want[2][1] and lo.same(llr, want[3][1])
    with pytest.raises(_lib.QbpError) as e:
        layered.performLayeredBPBatch(c.H, c.syn, c.prior, PAST_ITERS, "min-sum", alpha, order=order)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_run_dem_takes_large():
    c = ru.case("dem_synth")
    probs = np.minimum(0.5, c.probs * 5.0)
    kw = dict(prior=c.prior, seed=9, max_iter=MC_ITERS, variant=_lib.MIN_SUM, alpha=0.8, osd=True)
    plain = mc.run_dem(c.H, c.L, probs, 2000, layered=True, **kw)
    dec = bp.decoder_for(c.H, device=bp.DEVICE)
    assert not lu.layered_auto_is_large(c.shape)
    large = mc.run_dem(c.H, c.L, probs, 2000, layered="large", **kw)
    print(dict(zip(_lib.COUNTER_NAMES, large.tolist())))
    assert large[0] == 2000 and large[6] >= 64
    assert np.array_equal(large, plain)
    # past the LDS build's limit only "large" runs
    p = past_limit()
    pk = dict(prior=p.prior, distance=6, seed=11, max_iter=MC_ITERS, variant=_lib.MIN_SUM, alpha=0.8)
    got = mc.run_dem(p.H, p.L, p.probs, 64, layered="large", **pk)
    dec = bp.decoder_for(p.H, device=bp.DEVICE)
    errors = dec.mc_sample_errors_probs(p.probs, 0, 64, seed=11)
    syn = gu.syndromes_of(p.H, errors)
    order = past_order("default")
    hard, conv, iters, _ = lo.layered_decode_batch(p.H, syn, p.prior, MC_ITERS, _lib.MIN_SUM, 0.8, 20.0, order, "level")
    want = oracle.classify_trials(p.H, np.ascontiguousarray(p.L, np.uint8), 6, errors, syn, hard, conv, iters)
    assert np.array_equal(got, want)
    with pytest.raises(_lib.QbpError) as e:
        mc.run_dem(p.H, p.L, p.probs, 64, layered=True, **pk)
    assert e.value.code == _lib.E_UNSUPPORTED
