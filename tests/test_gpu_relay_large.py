"""GPU: Relay-BP's large build (QBP_OPT_RELAY_MEM: the messages of a record in a per-workgroup global workspace, V and
the bookkeeping in LDS) against the numpy statement (tests/relay_oracle.py) and against the LDS build, bit for bit, NaN
equal to NaN, into poisoned buffers -- forced on the small matrices of tests/test_gpu_relay.py and on the detector
error model of record_kernel_util, and chosen automatically one round past the LDS build's limit (34 rounds of the
[[72,12,6]] phenomenological matrix, 1224 x 3672); the records build behind QBP_FLAG_RELAY against the composition of
first-stage decode, statement and classification; the refusals; the Python layers."""
import functools

import numpy as np
import pytest

import geometry_util as gu
import record_kernel_util as ru
import large_util as lu
import relay_oracle as ro
import test_gpu_record_kernel_sizes as ts
import test_gpu_relay as tr
from qldpc_amd import _lib, bp, mc, relay

pytestmark = pytest.mark.gpu

OUTPUTS = ("hard", "converged", "iters", "llr", "legs", "solutions")
EXTRA = ("legs", "solutions")
ITER_LIMIT = tr.LEGS * tr.ITERS + 1
SMALL = [c for c in tr.CASES if c[0] != "144"]          # Steane, [[72,12,6]], the irregular 20 x 37 matrix
ROUNDS, NEAR_B = 34, ts.NEAR_B


def fresh(H, mem=None):
    dec = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    if mem is not None:
        dec.set_option(_lib.OPT_RELAY_MEM, mem)
    return dec


def configure_raw(dec, cfg):
    """qbp_relay_configure without Decoder.relay_configure's option write: the handle's QBP_OPT_RELAY_MEM stays."""
    return _lib.load().qbp_relay_configure(dec._h, cfg.gammas.ctypes.data, cfg.gammas.shape[0], cfg.leg_iters.ctypes.data,
                                           cfg.stop_after, cfg.alpha, cfg.clip_llr)


def with_large(cfg, large):
    return relay.RelayConfig(cfg.gammas, cfg.leg_iters, cfg.stop_after, cfg.alpha, cfg.clip_llr, large=large)


def batch_inputs(case):
    """(H, syndromes, prior, config, statement) of a case of test 1."""
    if case == "dem_synth":
        c = ru.case("dem_synth")
        return c.H, c.syn, c.prior, ts.relay_config(c.n), ts.relay_ref("dem_synth")
    return ts.relay_small_ref(*case)


def launch(dec, syn_t, prior_t, B, n, what, stream):
    out = ru.RecordOutputs(B, n, EXTRA)
    ru.relay_launch(dec, syn_t, prior_t, B, out, stream)
    return out.fetch_all(B, ITER_LIMIT, what)


# ---- 1. the forced large build against the statement and against the LDS build ------------------------------------------
BATCH_CASES = SMALL + ["dem_synth"]


def test_statement_classes_are_present_in_the_batch_cases():
    pooled = {k: sum(ro.classes(batch_inputs(c)[4])[k] for c in BATCH_CASES) for k in ("leg0", "later", "replaced", "never")}
    print(pooled)
    assert all(v >= 8 for v in pooled.values()), pooled


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: c if isinstance(c, str) else f"{c[0]}-{c[1]}")
def test_forced_large_build_equals_statement_and_lds_build(case):
    H, syn, prior, cfg, want = batch_inputs(case)
    B, n, sh = len(syn), H.shape[1], ru.Shape(H)
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    got = {}
    for mem in (lu.MEM_LARGE, lu.MEM_LDS):
        dec = fresh(H, mem)
        assert configure_raw(dec, cfg) == 0
        what = f"relay {case} mem {mem}"
        ts.on_own_stream(lambda s: got.__setitem__(mem, launch(dec, syn_t, prior_t, B, n, what, s)))
        ru.assert_same(got[mem], ru.relay_want(want), what)
        info = ru.info(dec)
        print(what, info, ro.classes(want))
        num_cu = dec.info("num_cu")
        if mem == lu.MEM_LARGE:
            assert info == dict(threads=ru.relay_threads(sh), grid=lu.relay_large_grid(sh, B, num_cu),
                                lds_bytes=lu.relay_large_lds_bytes(sh.m, sh.n))
        else:
            assert info == dict(threads=ru.relay_threads(sh), grid=ru.relay_grid(sh, B, num_cu),
                                lds_bytes=ru.relay_lds_bytes(sh.m, sh.n, sh.E))
    ru.assert_same(got[lu.MEM_LARGE], got[lu.MEM_LDS], f"relay {case}: large build against LDS build")


# ---- 2. one round past the LDS build's limit -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def past_limit():
    """The 34-round case of test_near_limit_decodes_and_one_round_more_is_unsupported, its configuration and statement."""
    c = ru.phenomenological(ROUNDS, ts.NEAR_P, 100 + ROUNDS - 1, NEAR_B)
    assert c.H.shape == (1224, 3672)
    cfg = ts.relay_config(c.n)
    want = ro.relay_decode_batch(c.H, c.syn, c.prior, cfg.gammas, cfg.leg_iters, tr.STOP, tr.ALPHA)
    return c, cfg, want


def test_one_round_past_the_limit():
    c, cfg, want = past_limit()
    sh = c.shape
    assert ru.relay_lds_bytes(sh.m, sh.n, sh.E) > ru.LDS_LIMIT > lu.relay_large_lds_bytes(sh.m, sh.n)
    syn_t, prior_t = gu.to_device(c.syn), gu.to_device(c.prior)
    # large=False: today's refusal, and no output is touched
    dec = fresh(c.H)
    with pytest.raises(_lib.QbpError) as e:
        dec.relay_configure(with_large(cfg, False))
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in _lib.load().qbp_last_error()
    out = ru.RecordOutputs(NEAR_B, c.n, EXTRA)
    with pytest.raises(_lib.QbpError) as e:
        ru.relay_launch(dec, syn_t, prior_t, NEAR_B, out, gu.stream_ptr())
    assert e.value.code == _lib.E_INVALID and out.untouched()          # (nothing is configured on this handle)
    # large=True: the statement
    dec.relay_configure(with_large(cfg, True))
    got = launch(dec, syn_t, prior_t, NEAR_B, c.n, "relay T = 34", gu.stream_ptr())
    ru.assert_same(got, ru.relay_want(want), "relay T = 34")
    info = ru.info(dec)
    print(c.H.shape, info, ro.classes(want))
    assert info["lds_bytes"] == lu.relay_large_lds_bytes(sh.m, sh.n) and info["grid"] == NEAR_B == 8
    assert info["threads"] == ru.relay_threads(sh)
    # a second, smaller launch on the same handle
    small = launch(dec, syn_t, prior_t, 3, c.n, "relay T = 34, B = 3", gu.stream_ptr())
    ru.assert_same(small, ru.relay_want(want, slice(0, 3)), "relay T = 34, B = 3")
    # the option set back after the configuration: the launch checks again, with today's message
    dec.set_option(_lib.OPT_RELAY_MEM, lu.MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        ru.relay_launch(dec, syn_t, prior_t, NEAR_B, out, gu.stream_ptr())
    msg = _lib.load().qbp_last_error()
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in msg and b"three rows of n doubles in LDS" in msg
    assert out.untouched()
    dec.set_option(_lib.OPT_RELAY_MEM, lu.MEM_AUTO)
    again = launch(dec, syn_t, prior_t, NEAR_B, c.n, "relay T = 34 again", gu.stream_ptr())
    ru.assert_same(again, ru.relay_want(want), "relay T = 34 again")


def test_automatic_choice_keeps_the_lds_build_where_it_fits():
    H, syn, prior, cfg, want = ts.relay_small_ref("72", 0.1, 1)
    sh = ru.Shape(H)
    dec = fresh(H)
    dec.relay_configure(with_large(cfg, True))
    got = launch(dec, gu.to_device(syn[:40]), gu.to_device(prior), 40, 72, "relay 72 auto", gu.stream_ptr())
    ru.assert_same(got, ru.relay_want(want, slice(0, 40)), "relay 72 auto")
    assert dec.info("lds_bytes") == ru.relay_lds_bytes(sh.m, sh.n, sh.E)


# ---- 3. more records than workgroups: a workgroup reuses its slice of the workspace ---------------------------------------
def test_work_counter_with_the_messages_in_the_workspace():
    H, syn, prior, cfg, ref = ts.relay_small_ref("72", 0.1, 1)
    sh, n = ru.Shape(H), H.shape[1]
    dec = fresh(H, lu.MEM_LARGE)
    assert configure_raw(dec, cfg) == 0
    B = 2 * lu.relay_large_grid(sh, 1 << 30, dec.info("num_cu")) + 37
    idx = ts.spread(B, 256, 5)
    syn_t, prior_t = gu.to_device(syn[idx]), gu.to_device(prior)
    got = []
    ts.on_own_stream(lambda s: got.append(launch(dec, syn_t, prior_t, B, n, f"relay large B {B}", s)))
    info = ru.info(dec)
    print(info, "B", B, ro.classes(ref))
    assert B == 2 * info["grid"] + 37 and info["lds_bytes"] == lu.relay_large_lds_bytes(sh.m, sh.n)
    ru.assert_same(got[0], ru.relay_want(ref, idx), f"relay large B {B}")


# ---- 4. the records build at the size of ph72x6 --------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["sum_product", "min_sum"])
@pytest.mark.parametrize("tag", ["ph72x6", "dem_synth"])
def test_mc_run_errors_equals_the_composition_and_the_lds_build(tag, first):
    H, L, d, errors, prior = ts.mc_case(tag)
    n = H.shape[1]
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    cfg = tr.config(n, 4)
    kw = dict(max_iter=ts.MC_ITERS, variant=variant, alpha=tr.ALPHA, flags=_lib.FLAG_RELAY)
    got = {}
    for mem in (lu.MEM_LARGE, lu.MEM_LDS):
        dec = fresh(H, mem)
        assert configure_raw(dec, cfg) == 0
        got[mem] = dec.mc_run_errors(L, d, errors, prior, **kw)
        sh = ru.Shape(H)
        assert dec.info("lds_bytes") == (lu.relay_large_lds_bytes(sh.m, sh.n, True) if mem == lu.MEM_LARGE
                                         else ru.relay_lds_bytes(sh.m, sh.n, sh.E, True))
    want, failures = tr.compose(dec, H, L, d, errors, prior, cfg, variant)
    print(tag, first, dict(zip(_lib.COUNTER_NAMES, got[lu.MEM_LARGE].tolist())), "failures", failures)
    assert failures >= 64 and want[6] == failures and want[0] == len(errors)
    assert np.array_equal(got[lu.MEM_LARGE], want)
    assert np.array_equal(got[lu.MEM_LARGE], got[lu.MEM_LDS])


# ---- 5. the records build past the limit ---------------------------------------------------------------------------------
MC_TRIALS, MC_P, MC_SEED = 192, 0.02, 11
# At p = 0.02 a trial of the 34-round matrix has 73 errors on average among 3672 columns; 8 iterations of BP converge on
# next to none of them (the first-stage count is asserted below), so nearly every trial reaches the second stage.


def test_mc_run_probs_past_the_limit():
    c, _, _ = past_limit()
    L = np.ascontiguousarray(c.L, np.uint8)
    probs = np.full(c.n, MC_P)
    prior = c.prior
    cfg = with_large(tr.config(c.n, 4), True)
    dec = fresh(c.H)
    dec.relay_configure(cfg)
    kw = dict(seed=MC_SEED, max_iter=ts.MC_ITERS, alpha=tr.ALPHA, flags=_lib.FLAG_RELAY)
    got = dec.mc_run_probs(L, 6, probs, prior, 0, MC_TRIALS, **kw)
    sh = c.shape
    assert dec.info("lds_bytes") == lu.relay_large_lds_bytes(sh.m, sh.n, True)
    errors = dec.mc_sample_errors_probs(probs, 0, MC_TRIALS, seed=MC_SEED)
    want, failures = tr.compose(dec, c.H, L, 6, errors, prior, cfg, _lib.SUM_PRODUCT)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), "failures", failures)
    assert failures >= 64 and got[0] == MC_TRIALS and got[6] == failures
    assert np.array_equal(got, want)
    parts = dec.mc_run_probs(L, 6, probs, prior, 0, 77, **kw) + dec.mc_run_probs(L, 6, probs, prior, 77, MC_TRIALS, **kw)
    assert np.array_equal(parts, got)
    # without the option the Monte-Carlo call is refused before any GPU work
    dec.set_option(_lib.OPT_RELAY_MEM, lu.MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_probs(L, 6, probs, prior, 0, MC_TRIALS, **kw)
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in _lib.load().qbp_last_error()


# ---- 6. the upper refusal (host only) and the option's range ----------------------------------------------------------------
def one_check(n):
    H = np.zeros((1, n), np.uint8)
    H[0, :5] = 1
    return H


def test_upper_refusal_and_option_range():
    lib = _lib.load()
    # 1 x 20 475: the first width whose large build passes 160 KiB (8 n + 48 bytes)
    n = lu.first_n_beyond_the_limit(lambda n: lu.relay_large_lds_bytes(1, n))
    dec = fresh(one_check(n))
    cfg = relay.RelayConfig(np.zeros((1, n)), [3], large=True)
    with pytest.raises(_lib.QbpError) as e:
        dec.relay_configure(cfg)
    msg = lib.qbp_last_error()
    assert e.value.code == _lib.E_UNSUPPORTED
    assert b"global memory" in msg and str(lu.relay_large_lds_bytes(1, n)).encode() in msg and b"160 KiB" in msg
    out = ru.RecordOutputs(2, n, EXTRA)
    with pytest.raises(_lib.QbpError) as e:             # nothing was configured: no launch
        ru.relay_launch(dec, gu.to_device(np.zeros((2, 1), np.uint8)), gu.to_device(np.ones(n)), 2, out, gu.stream_ptr())
    assert e.value.code == _lib.E_INVALID and out.untouched()
    # 1 x 20 000 with option 2: 160 048 bytes fit the batch build, the records build (+ n bytes) does not -- the
    # Monte-Carlo call is refused before any GPU work, with the large build's need in the message
    n = 20000
    dec = fresh(one_check(n))
    dec.relay_configure(relay.RelayConfig(np.zeros((1, n)), [3], large=True))
    counters = np.full(12, 7, np.int64)
    Lx = np.zeros((1, n), np.uint8)
    Lx[0, 0] = 1
    prior = np.ones(n)
    rc = lib.qbp_mc_run(dec._h, Lx.ctypes.data, 1, 0, 0.001, 1, 0, 0, 50, prior.ctypes.data, 4, 0, 1.0, 1.0, 20.0,
                        _lib.FLAG_RELAY, counters.ctypes.data)
    msg = lib.qbp_last_error()
    assert rc == _lib.E_UNSUPPORTED and np.all(counters == 7)
    assert b"global memory" in msg and str(lu.relay_large_lds_bytes(1, n, True)).encode() in msg
    # the option's range
    for bad in (3, -1):
        with pytest.raises(_lib.QbpError) as e:
            dec.set_option(_lib.OPT_RELAY_MEM, bad)
        assert e.value.code == _lib.E_INVALID
    for ok in (0, 1, 2):
        dec.set_option(_lib.OPT_RELAY_MEM, ok)


# ---- 7. the Python layers --------------------------------------------------------------------------------------------------
def test_perform_relay_bp_takes_large():
    c, cfg, want = past_limit()
    r = relay.performRelayBPBatch(c.H, c.syn, c.prior, cfg.gammas, cfg.leg_iters, tr.STOP, tr.ALPHA, large=True)
    ru.assert_same(tuple(r), ru.relay_want(want), "performRelayBPBatch T = 34")
    hard, conv, llr, iters = relay.performRelayBP(c.H, c.syn[0], c.prior, cfg.gammas, cfg.leg_iters, tr.STOP, tr.ALPHA,
                                                  large=True)
    assert np.array_equal(hard, want["hard"][0]) and conv == bool(want["converged"][0]) and iters == want["iters"][0]
    assert ro.same(llr, want["llr"][0])
    with pytest.raises(_lib.QbpError) as e:
        relay.performRelayBPBatch(c.H, c.syn, c.prior, cfg.gammas, cfg.leg_iters, tr.STOP, tr.ALPHA)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_run_dem_takes_large():
    c, _, _ = past_limit()
    probs = np.full(c.n, MC_P)
    cfg = with_large(tr.config(c.n, 4), True)
    kw = dict(seed=MC_SEED, max_iter=ts.MC_ITERS, alpha=tr.ALPHA)
    got = mc.run_dem(c.H, c.L, probs, MC_TRIALS, prior=c.prior, distance=6, relay=cfg.as_dict(), **kw)
    dec = fresh(c.H)
    dec.relay_configure(cfg)
    direct = dec.mc_run_probs(np.ascontiguousarray(c.L, np.uint8), 6, probs, c.prior, 0, MC_TRIALS, flags=_lib.FLAG_RELAY,
                              **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[0] == MC_TRIALS and got[6] >= 64
    assert np.array_equal(got, direct)
    with pytest.raises(_lib.QbpError) as e:
        mc.run_dem(c.H, c.L, probs, MC_TRIALS, prior=c.prior, distance=6, relay=with_large(cfg, False), **kw)
    assert e.value.code == _lib.E_UNSUPPORTED
