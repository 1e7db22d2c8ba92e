"""GPU: bp_layered_kernel against the numpy statement of layered BP (tests/layered_oracle.py), bit for bit -- the batch
build on five matrices, three orders, both variants and three iteration limits; launch geometries into poisoned buffers;
and the Monte-Carlo build behind QBP_FLAG_LAYERED against statement + classification, alone and under OSD and Relay-BP.

"Bit for bit" for float64 outputs: equal values, NaN equal to NaN (none is expected: the irregular matrix has no check
of weight 1)."""
import functools

import numpy as np
import pytest

import geometry_util as gu
import layered_oracle as lo
from oracle import oracle
from qldpc_amd import _lib, bp, codes, dem, mc, relay

pytestmark = pytest.mark.gpu

MATRICES = ["steane", "72", "irr37", "disjoint70", "144"]
ORDERS = ["default", "ascending", "random"]
VARIANTS = [(_lib.SUM_PRODUCT, 1.0), (_lib.MIN_SUM, 0.8)]
PS = (0.01, 0.03, 0.06, 0.1, 0.15)
PER_P = {"steane": 16, "72": 24, "irr37": 20, "disjoint70": 13, "144": 13}       # B = 5 * PER_P: 64 .. 120
LAYERED = _lib.FLAG_LAYERED


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


@functools.lru_cache(maxsize=None)
def case(name):
    """(H, errors, syndromes, prior) of one matrix: error rates from 0.01 to 0.15, a non-uniform prior."""
    H = lo.matrix(name)
    n = H.shape[1]
    rng = np.random.default_rng(100 + len(name) + n)
    errors = np.concatenate([(rng.random((PER_P[name], n)) < p).astype(np.uint8) for p in PS])
    syn = (errors.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    prior = np.log(0.95 / 0.05) * rng.uniform(0.5, 1.5, n)
    return H, errors, syn, prior


@functools.lru_cache(maxsize=None)
def statement(name, kind, variant, alpha, max_iter):
    H, _, syn, prior = case(name)
    return lo.layered_decode_batch(H, syn, prior, max_iter, variant, alpha, 20.0, lo.order_of(H, kind), "level")


def logicals(name):
    """(Lx, distance) of the Monte-Carlo matrices."""
    if name == "irr37":
        return (np.random.default_rng(3).random((3, 37)) < 0.3).astype(np.uint8), 4
    c = codes.load_code({"72": "[[72, 12, 6]]", "144": "[[144, 12, 12]]"}[name])
    return np.asarray(c.Lx).astype(np.uint8), c.distance


# ---- 1. the batch build against the statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("name", MATRICES)
def test_batch_kernel_equals_statement(name, kind):
    H, _, syn, prior = case(name)
    B, n = len(syn), H.shape[1]
    # both outcomes, and late convergers, are present in the records of this matrix (pooled over variants and orders)
    pool = [statement(name, k, v, a, 50) for k in ORDERS for v, a in VARIANTS]
    conv = np.concatenate([r[1] for r in pool])
    iters = np.concatenate([r[2] for r in pool])
    print(name, "converged", int(conv.sum()), "of", len(conv), "late (> 2)", int((conv & (iters > 2)).sum()))
    assert conv.sum() >= 8 and (~conv).sum() >= 8
    dec = fresh(H)
    dec.layered_configure(lo.order_of(H, kind))
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = gu.Outputs(B, n)
    for variant, alpha in VARIANTS:
        for max_iter in (1, 2, 50):
            want = statement(name, kind, variant, alpha, max_iter)
            what = f"{name} {kind} variant {variant} max_iter {max_iter}"
            got = gu.decode(dec, syn_t, prior_t, B, out, what, max_iter=max_iter, variant=variant, alpha=alpha,
                            flags=LAYERED)
            gu.assert_same(got, want, what)
            assert dec.info("last_kernel") == 4


def test_late_convergers_are_present():
    late = 0
    for name in ("72", "irr37", "144"):
        for v, a in VARIANTS:
            _, conv, iters, _ = statement(name, "default", v, a, 50)
            late += int((conv & (iters > 2)).sum())
    assert late >= 8


# ---- 2. launch geometry: slots, B = 1, B no multiple of S ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72", "irr37", "disjoint70"])
def test_outputs_do_not_depend_on_slots_or_batch(name):
    H, _, syn, prior = case(name)
    n = H.shape[1]
    dec = fresh(H)
    dec.layered_configure(None)
    prior_t = gu.to_device(prior)
    for variant, alpha in VARIANTS:
        want = statement(name, "default", variant, alpha, 50)
        for slots in (1, 2, 0):
            dec.set_option(_lib.OPT_LAYERED_SLOTS, slots)
            for B in (1, 37, len(syn)):
                # (37 is no multiple of 2, nor of the automatic S of these matrices: 28, 32 and 3)
                rows = np.arange(len(syn) - B, len(syn))          # the tail: the high-rate records
                out = gu.Outputs(B, n)
                what = f"{name} variant {variant} slots {slots} B {B}"
                got = gu.decode(dec, gu.to_device(syn[rows]), prior_t, B, out, what, variant=variant, alpha=alpha,
                                flags=LAYERED)
                gu.assert_same(got, tuple(x[rows] for x in want), what)
                # null outputs stay untouched
                got = gu.decode(dec, gu.to_device(syn[rows]), prior_t, B, out, what, variant=variant, alpha=alpha,
                                flags=LAYERED, nulls=("llr", "iters"))
                assert np.array_equal(got[0], want[0][rows]) and np.array_equal(got[1], want[1][rows])
        dec.set_option(_lib.OPT_LAYERED_SLOTS, 0)


@pytest.mark.parametrize("name", ["72", "irr37"])
def test_force_full_returns_the_early_exit_bits(name):
    H, _, syn, prior = case(name)
    B, n = len(syn), H.shape[1]
    dec = fresh(H)
    dec.layered_configure(None)
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = gu.Outputs(B, n)
    for variant, alpha in VARIANTS:
        for max_iter in (1, 50):
            want = statement(name, "default", variant, alpha, max_iter)
            what = f"{name} forced variant {variant} max_iter {max_iter}"
            got = gu.decode(dec, syn_t, prior_t, B, out, what, max_iter=max_iter, variant=variant, alpha=alpha,
                            flags=LAYERED | _lib.FLAG_FORCE_FULL | _lib.FLAG_FAST_MATH)
            gu.assert_same(got, want, what)


@pytest.mark.parametrize("name", ["steane", "72", "irr37"])
def test_host_and_device_entries_agree(name):
    H, _, syn, prior = case(name)
    dec = fresh(H)
    for kind in ("default", "random"):
        for variant, alpha in VARIANTS:
            want = statement(name, kind, variant, alpha, 50)
            got = dec.decode(syn, prior, 50, variant, alpha, layered=lo.order_of(H, kind))
            gu.assert_same(got, want, f"{name} host entry {kind} {variant}")
            one = dec.decode(syn[-1:], prior, 50, variant, alpha, layered=True)       # (the small-call path)
            gu.assert_same(one, tuple(x[-1:] for x in want), f"{name} host entry, one syndrome")
    from qldpc_amd import layered
    hard, conv, llr, it = layered.performLayeredBP(H, syn[3], prior, 50, "min-sum", 0.8, order=lo.order_of(H, "random"))
    want = statement(name, "random", _lib.MIN_SUM, 0.8, 50)
    assert np.array_equal(hard, want[0][3]) and conv == want[1][3] and it == want[2][3] and lo.same(llr, want[3][3])


def test_flag_clear_is_untouched_by_the_configuration():
    H, _, syn, prior = case("72")
    dec = fresh(H)
    before = [dec.decode(syn, prior, 50, v, a) for v, a in VARIANTS + [(_lib.DAMPED_SP, 0.9)]]
    dec.layered_configure(lo.order_of(H, "random"))
    dec.decode(syn, prior, 50, layered=True)
    after = [dec.decode(syn, prior, 50, v, a) for v, a in VARIANTS + [(_lib.DAMPED_SP, 0.9)]]
    for x, y in zip(before, after):
        gu.assert_same(x, y, "flooding after qbp_layered_configure")
    assert dec.info("last_kernel") != 4


# ---- 3. Monte-Carlo -----------------------------------------------------------------------------------------------------------
MC_ITERS = 12


def expected_counters(H, L, d, errors, prior, variant, alpha, order=None):
    syn = (errors.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    hard, conv, iters, _ = lo.layered_decode_batch(H, syn, prior, MC_ITERS, variant, alpha, 20.0, order)
    return oracle.classify_trials(H, L, d, errors, syn, hard, conv, iters), int((~conv).sum())


@pytest.mark.parametrize("variant,alpha", VARIANTS, ids=["sum_product", "min_sum"])
@pytest.mark.parametrize("name", ["72", "irr37", "144"])
def test_mc_run_errors_equals_statement_and_classification(name, variant, alpha):
    H, errors, _, prior = case(name)
    L, d = logicals(name)
    want, failures = expected_counters(H, L, d, errors, prior, variant, alpha)
    dec = fresh(H)
    dec.layered_configure(None)
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=alpha, flags=LAYERED)
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), failures)
    assert failures >= 8 and failures < len(errors)
    assert np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, d, errors[:31], prior, **kw)
                          + dec.mc_run_errors(L, d, errors[31:], prior, **kw), want)
    dec.set_option(_lib.OPT_LAYERED_SLOTS, 1)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, **kw), want)


@pytest.mark.parametrize("name", ["72", "irr37", "144"])
def test_sampled_entries_equal_the_statement_on_their_samplers_errors(name):
    H, _, _, prior = case(name)
    n = H.shape[1]
    L, d = logicals(name)
    T, p, w = 96, 0.07, max(2, n // 14)
    probs = np.random.default_rng(5).uniform(0.02, 0.12, n)
    dec = fresh(H)
    dec.layered_configure(None)
    variant, alpha = _lib.MIN_SUM, 0.8
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=alpha, flags=LAYERED)
    runs = [
        (dec.mc_sample_errors(p, 5, T, seed=9), lambda a, b: dec.mc_run(L, d, p, prior, a, b, seed=9, **kw)),
        (dec.mc_sample_errors_probs(probs, 5, T, seed=9), lambda a, b: dec.mc_run_probs(L, d, probs, prior, a, b, seed=9, **kw)),
        (dec.mc_sample_errors_weight(w, 5, T, seed=9), lambda a, b: dec.mc_run_weight(L, d, w, prior, a, b, seed=9, **kw)),
    ]
    for errors, run in runs:
        want, failures = expected_counters(H, L, d, errors, prior, variant, alpha)
        whole = run(5, 5 + T)
        assert np.array_equal(whole, want), (whole, want)
        assert np.array_equal(run(5, 6) + run(6, 50) + run(50, 5 + T), want)          # the split of the range
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 7)                                   # several chunks per call
        assert np.array_equal(run(5, 5 + T), want)
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)


def relay_config(n):
    return relay.RelayConfig(relay.relay_gammas(n, 3, 0.125, (-0.24, 0.66), 4), [10] * 3, 1, 0.9)


@pytest.mark.parametrize("stage", ["osd0", "cs7", "relay"])
@pytest.mark.parametrize("name", ["72", "irr37", "144"])
def test_second_stages_act_on_the_layered_failure_records(name, stage):
    """Counters = layered decode (batch entry) -> qbp_osd_batch / qbp_relay_decode_batch on the failures -> numpy
    classification."""
    H, errors, syn, prior = case(name)
    n = H.shape[1]
    L, d = logicals(name)
    variant, alpha = _lib.SUM_PRODUCT, 1.0
    dec = fresh(H)
    dec.layered_configure(None)
    hard, conv, iters, llr = dec.decode(syn, prior, MC_ITERS, variant, alpha, layered=True)
    f = np.flatnonzero(~conv)
    assert len(f) >= 8
    det = hard.copy()
    if stage == "relay":
        cfg = relay_config(n)
        r_hard, r_conv = dec.relay_decode(syn[f], prior, cfg)[:2]
        det[f] = r_hard
        invalid = int((~r_conv).sum())
        flags = LAYERED | _lib.FLAG_RELAY
    else:
        if stage == "osd0":
            det[f] = dec.osd0(syn[f], llr[f], hard[f])
            flags = LAYERED | _lib.FLAG_OSD0
        else:
            det[f] = dec.osd(syn[f], llr[f], hard[f], method="cs", order=7)
            flags = LAYERED | _lib.FLAG_OSD0 | _lib.osd_flags("cs", 7)
        invalid = int(((det[f].astype(np.int64) @ H.T.astype(np.int64) % 2) != syn[f]).any(1).sum())
    want = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    want[10] = invalid
    got = dec.mc_run_errors(L, d, errors, prior, max_iter=MC_ITERS, variant=variant, alpha=alpha, flags=flags)
    print(stage, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[6] == len(f)
    assert np.array_equal(got, want)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refused_combinations_return_their_codes():
    H, _, syn, prior = case("72")
    n = 72
    L, d = logicals("72")
    Lx = np.ascontiguousarray(L, np.uint8)
    lib = _lib.load()
    dec = fresh(H)
    fill = np.full(12, 7, np.int64)
    probs = np.full(n, 0.05)

    def code_of(fn):
        with pytest.raises(_lib.QbpError) as e:
            fn()
        return e.value.code

    def mc_rc(flags, variant=0, pr=prior):
        counters = fill.copy()
        rc = lib.qbp_mc_run(dec._h, Lx.ctypes.data, Lx.shape[0], d, 0.05, 1, 0, 0, 50, pr.ctypes.data, 8, variant, 1.0, 1.0,
                            20.0, flags, counters.ctypes.data)
        assert rc == 0 or np.array_equal(counters, fill)
        return rc

    # the flag without a configuration
    assert code_of(lambda: dec.decode(syn, prior, 8, flags=LAYERED)) == _lib.E_INVALID
    assert b"qbp_layered_configure" in lib.qbp_last_error()
    assert mc_rc(LAYERED) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_errors(L, d, np.zeros((4, n), np.uint8), prior, flags=LAYERED)) == _lib.E_INVALID
    # a refused order configures nothing
    bad = np.arange(36, dtype=np.int32); bad[3] = 2
    assert lib.qbp_layered_configure(dec._h, bad.ctypes.data) == _lib.E_INVALID
    assert mc_rc(LAYERED) == _lib.E_INVALID
    dec.layered_configure(None)
    assert mc_rc(LAYERED) == 0
    # the damped variant, column-sum orders
    assert code_of(lambda: dec.decode(syn, prior, 8, _lib.DAMPED_SP, flags=LAYERED)) == _lib.E_INVALID
    assert mc_rc(LAYERED, variant=_lib.DAMPED_SP) == _lib.E_INVALID
    for colsum in (_lib.FLAG_PAIRWISE_COLSUM, _lib.FLAG_DENSE_F_COLSUM, _lib.FLAG_DENSE_F_COLSUM_ITER0):
        assert code_of(lambda: dec.decode(syn, prior, 8, flags=LAYERED | colsum)) == _lib.E_INVALID
        assert mc_rc(LAYERED | colsum) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_weight(L, d, 3, prior, 0, 10, variant=_lib.DAMPED_SP, flags=LAYERED)) == _lib.E_INVALID
    # a prior that is not finite, at the host entries
    inf = prior.copy(); inf[5] = np.inf
    assert code_of(lambda: dec.decode(syn, inf, 8, flags=LAYERED)) == _lib.E_INVALID
    assert mc_rc(LAYERED, pr=inf) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_errors(L, d, np.zeros((4, n), np.uint8), inf, flags=LAYERED)) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_probs(L, d, probs, inf, 0, 10, flags=LAYERED)) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_weight(L, d, 3, inf, 0, 10, flags=LAYERED)) == _lib.E_INVALID
    dec.decode(syn, inf, 8)                                     # (legal without the flag)
    # entries without a layered build
    for fn in (lambda: dec.mc_run_budgets(L, d, probs, prior, (4, 8), 0, 100, flags=LAYERED),
               lambda: dec.mc_run_spectrum(L, d, probs, prior, 0, 100, max_iter=8, flags=LAYERED),
               lambda: dec.mc_run_errors_spectrum(L, d, np.zeros((10, n), np.uint8), prior, max_iter=8, flags=LAYERED),
               lambda: dec.decode_shots(L, np.zeros((10, 5), np.uint8), prior, max_iter=8, flags=LAYERED),
               lambda: dec.check_messages(syn[:2], prior, _lib.MIN_SUM, flags=LAYERED)):
        assert code_of(fn) == _lib.E_UNSUPPORTED
    # the option's range
    assert code_of(lambda: dec.set_option(_lib.OPT_LAYERED_SLOTS, 33)) == _lib.E_INVALID
    assert code_of(lambda: dec.set_option(_lib.OPT_LAYERED_SLOTS, -1)) == _lib.E_INVALID
    # a matrix whose single-slot state exceeds the LDS, and the largest one that must work
    Hst = np.asarray(dem.phenomenological("[[144, 12, 12]]", 12, 0.004)[0].todense()).astype(np.uint8)
    assert Hst.shape == (864, 2592)
    big = fresh(Hst)
    big.layered_configure(None)
    s = np.zeros((3, 864), np.uint8); s[1, 5] = 1; s[2, [7, 300]] = 1
    pr = np.full(2592, 5.0)
    gu.assert_same(big.decode(s, pr, 6, _lib.MIN_SUM, 0.9, layered=True),
                   lo.layered_decode_batch(Hst, s, pr, 6, lo.MIN_SUM, 0.9), "864 x 2592")
    wide = np.zeros((4, 8000), np.uint8)                        # (prior, posterior and messages: 3 n doubles, 188 KiB)
    wide[np.arange(8000) % 4, np.arange(8000)] = 1
    assert code_of(lambda: fresh(wide).layered_configure(None)) == _lib.E_UNSUPPORTED
