"""GPU: bp_relay_kernel against the numpy statement of Relay-BP (tests/relay_oracle.py), bit for bit -- the batch
build on four matrices, the gamma = 0 identity with the min-sum decoder, and the records build behind QBP_FLAG_RELAY
against the composition of first-stage decode, statement and classification.

"Bit for bit" for float64 outputs: equal values, NaN equal to NaN (the irregular matrix has checks of weight 1, whose
message is infinite and turns its variable's posterior into NaN from the second iteration on, as in the reference's
min-sum)."""
import numpy as np
import pytest

import relay_oracle as ro
from oracle import oracle
from qldpc_amd import _lib, bp, codes, dem, mc, relay

pytestmark = pytest.mark.gpu

LEGS, ITERS, STOP, GAMMA0, INTERVAL, ALPHA = 5, 12, 2, 0.125, (-0.24, 0.66), 0.9
# (matrix, error rate, seed of errors and gammas)
CASES = [("steane", 0.1, 1), ("steane", 0.15, 2), ("72", 0.1, 1), ("72", 0.15, 2), ("rand37", 0.05, 1),
         ("rand37", 0.1, 2), ("144", 0.05, 1), ("144", 0.1, 2)]


def irregular37():
    """An irregular 20 x 37 matrix (row weights 1 .. 13, column weights 1 .. 7: long rows and long columns) and three
    logical rows."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.3, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1          # (no empty row)
    L = (rng.random((3, 37)) < 0.3).astype(np.uint8)
    return H, L


def matrix(name):
    if name == "rand37":
        H, L = irregular37()
        return H, L, 4
    c = codes.load_code({"steane": "steane", "72": "[[72, 12, 6]]", "144": "[[144, 12, 12]]"}[name])
    return np.asarray(c.Hx), np.asarray(c.Lx), c.distance


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def config(n, seed):
    return relay.RelayConfig(relay.relay_gammas(n, LEGS, GAMMA0, INTERVAL, seed), [ITERS] * LEGS, STOP, ALPHA)


@pytest.fixture(scope="module")
def references():
    """The statement on every case, computed once: (H, syndromes, prior, config, result)."""
    out = {}
    for name, p, seed in CASES:
        H, _, _ = matrix(name)
        n = H.shape[1]
        errors = (np.random.default_rng(seed).random((256, n)) < p).astype(np.uint8)
        syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
        prior = np.full(n, np.log((1 - p) / p))
        cfg = config(n, seed)
        out[name, p] = (H, syn, prior, cfg, ro.relay_decode_batch(H, syn, prior, cfg.gammas, cfg.leg_iters, STOP, ALPHA))
    return out


# ---- 1. the batch kernel against the statement -------------------------------------------------------------------------
@pytest.mark.parametrize("name,p,seed", CASES)
def test_batch_kernel_equals_statement(references, name, p, seed):
    """The four classes are counted over the whole set of cases: every syndrome of the Steane code is solved in leg 0,
    and the irregular matrix's records are solved in leg 0 or never (a NaN posterior does not recover), so no single
    matrix shows all four; every matrix contributes to at least two."""
    pooled = {k: sum(ro.classes(r[4])[k] for r in references.values()) for k in ("leg0", "later", "replaced", "never")}
    print(pooled, ro.classes(references[name, p][4]))
    assert all(v >= 8 for v in pooled.values()), pooled
    per_matrix = {k: sum(ro.classes(references[nm, q][4])[k] for nm, q, _ in CASES if nm == name) for k in pooled}
    assert sum(v >= 8 for v in per_matrix.values()) >= 2, per_matrix
    H, syn, prior, cfg, want = references[name, p]
    dec = fresh(H)
    hard, conv, iters, llr, legs, sols = dec.relay_decode(syn, prior, cfg)
    assert np.array_equal(conv, want["converged"])
    assert np.array_equal(iters, want["iters"]) and np.array_equal(legs, want["legs"])
    assert np.array_equal(sols, want["solutions"])
    assert np.array_equal(hard, want["hard"])
    assert ro.same(llr, want["llr"])
    # null outputs, and a second call on the configured handle
    h2, c2, i2, none, l2, s2 = dec.relay_decode(syn[:100], prior, want_llr=False)
    assert none is None and np.array_equal(h2, hard[:100]) and np.array_equal(i2, iters[:100])


# ---- 2. gammas = 0, one leg, stop_after = 1: the device's min-sum decoder -------------------------------------------------
@pytest.mark.parametrize("name", ["72", "rand37"])
def test_gamma_zero_is_min_sum_on_the_device(name):
    H, _, _ = matrix(name)
    n = H.shape[1]
    errors = (np.random.default_rng(5).random((300, n)) < 0.05).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log(0.95 / 0.05))
    dec = fresh(H)
    hard, conv, iters, llr = dec.decode(syn, prior, 30, variant=_lib.MIN_SUM, alpha=0.8, damping=1.0)
    r_hard, r_conv, r_iters, r_llr, legs, sols = dec.relay_decode(syn, prior, relay.RelayConfig(np.zeros((1, n)), [30], 1, 0.8))
    assert 20 < conv.sum() < 300
    assert np.array_equal(r_hard, hard) and np.array_equal(r_conv, conv) and np.array_equal(r_iters - 1, iters)
    assert ro.same(r_llr, llr)
    assert np.all(legs == 1) and np.array_equal(sols, conv.astype(np.int32))


# ---- 3. QBP_FLAG_RELAY: the records build ------------------------------------------------------------------------------------
MC_ITERS = 8


def compose(dec, H, L, d, errors, prior, cfg, variant):
    """qbp_decode_batch (first stage), the statement on its failures, oracle.classify_trials' rules."""
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, _ = dec.decode(syn, prior, MC_ITERS, variant=variant, alpha=ALPHA)
    det = hard.copy()
    f = np.flatnonzero(~conv)
    r = ro.relay_decode_batch(H, syn[f], prior, cfg.gammas, cfg.leg_iters, cfg.stop_after, cfg.alpha, cfg.clip_llr)
    det[f] = r["hard"]
    cnt = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    cnt[10] = int((~r["converged"]).sum())
    assert cnt[10] == int(((det[f].astype(np.int64) @ H.T % 2) != syn[f]).any(1).sum())
    return cnt, len(f)


@pytest.mark.parametrize("variant", [_lib.SUM_PRODUCT, _lib.MIN_SUM], ids=["sum_product", "min_sum"])
@pytest.mark.parametrize("name,p", [("72", 0.08), ("rand37", 0.06)])
def test_mc_run_errors_equals_the_composition(name, p, variant):
    H, L, d = matrix(name)
    n = H.shape[1]
    errors = (np.random.default_rng(17).random((700, n)) < p).astype(np.uint8)
    prior = mc.prior_of(p, n)
    cfg = config(n, 4)
    dec = fresh(H)
    dec.relay_configure(cfg)
    want, failures = compose(dec, H, L, d, errors, prior, cfg, variant)
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=ALPHA, flags=_lib.FLAG_RELAY)
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), failures)
    assert failures >= 8 and got[6] == failures and got[0] == 700
    assert np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, **kw), want)       # the record buffers reused
    assert np.array_equal(dec.mc_run_errors(L, d, errors[:300], prior, **kw)
                          + dec.mc_run_errors(L, d, errors[300:], prior, **kw), want)


def test_counters_do_not_depend_on_the_split_of_the_range():
    H, L, d = matrix("72")
    prior = mc.prior_of(0.08, 72)
    dec = fresh(H)
    dec.relay_configure(config(72, 4))
    kw = dict(seed=21, max_iter=MC_ITERS, flags=_lib.FLAG_RELAY)
    whole = dec.mc_run(L, d, 0.08, prior, 0, 1000, **kw)
    assert whole[0] == 1000 and whole[6] >= 8
    parts = dec.mc_run(L, d, 0.08, prior, 0, 1, **kw) + dec.mc_run(L, d, 0.08, prior, 1, 377, **kw) \
        + dec.mc_run(L, d, 0.08, prior, 377, 1000, **kw)
    assert np.array_equal(parts, whole)
    assert np.array_equal(fresh_configured(H).mc_run_probs(L, d, np.full(72, 0.08), prior, 0, 1000, **kw), whole)
    bp_only = dec.mc_run(L, d, 0.08, prior, 0, 1000, seed=21, max_iter=MC_ITERS)
    assert np.array_equal(bp_only[[0, 6, 7]], whole[[0, 6, 7]])      # the first stage's bookkeeping is untouched
    assert whole[1] <= bp_only[1]


def fresh_configured(H):
    dec = fresh(H)
    dec.relay_configure(config(H.shape[1], 4))
    return dec


def test_fixed_weight_run_takes_the_flag():
    H, L, d = matrix("72")
    prior = mc.prior_of(0.05, 72)
    dec = fresh_configured(H)
    kw = dict(max_iter=MC_ITERS, flags=_lib.FLAG_RELAY)
    got = dec.mc_run_weight(L, d, 9, prior, 0, 500, seed=4, **kw)
    errors = dec.mc_sample_errors_weight(9, 0, 500, seed=4)
    assert got[6] >= 8 and np.array_equal(got, dec.mc_run_errors(L, d, errors, prior, **kw))


# ---- 4. QBP_E_INVALID and QBP_E_UNSUPPORTED -----------------------------------------------------------------------------------
def test_invalid_and_unsupported_cases():
    H, L, d = matrix("72")
    Lx = np.ascontiguousarray(L, np.uint8)
    n = 72
    prior = mc.prior_of(0.05, n)
    lib = _lib.load()
    dec = fresh(H)
    syn = np.zeros((4, 36), np.uint8)
    fill = np.full(12, 7, np.int64)

    def run(flags, h=dec):
        counters = fill.copy()
        rc = lib.qbp_mc_run(h._h, Lx.ctypes.data, Lx.shape[0], d, 0.05, 1, 0, 0, 200, prior.ctypes.data, MC_ITERS, 0, 1.0,
                            1.0, 20.0, flags, counters.ctypes.data)
        assert rc == 0 or np.array_equal(counters, fill)
        return rc

    # nothing configured yet
    with pytest.raises(_lib.QbpError) as e:
        dec.relay_decode(syn, prior)
    assert e.value.code == -1
    assert run(_lib.FLAG_RELAY) == -1 and b"qbp_relay_configure" in lib.qbp_last_error()

    def configure(g, iters, stop=1, alpha=1.0, clip=20.0, L_=None):
        g = np.ascontiguousarray(g, np.float64)
        it = np.ascontiguousarray(iters, np.int32)
        return lib.qbp_relay_configure(dec._h, g.ctypes.data, len(it) if L_ is None else L_, it.ctypes.data, stop, alpha, clip)

    g = relay.relay_gammas(n, 2, 0.1, (-0.2, 0.6), 0)
    bad = g.copy()
    bad[1, 70] = np.nan
    assert configure(bad, [3, 3]) == -1 and b"gammas[1][70]" in lib.qbp_last_error()
    bad[1, 70] = np.inf
    assert configure(bad, [3, 3]) == -1
    assert configure(g, [3, 0]) == -1 and configure(g, [3, 3], L_=0) == -1 and configure(g, [3, 3], stop=0) == -1
    assert configure(g, [3, 3], alpha=np.nan) == -1 and configure(g, [3, 3], clip=np.inf) == -1
    assert lib.qbp_relay_configure(dec._h, None, 2, np.ones(2, np.int32).ctypes.data, 1, 1.0, 20.0) == -1
    assert run(_lib.FLAG_RELAY) == -1                       # (a refused configuration configures nothing)
    assert configure(g, [3, 3]) == 0
    assert run(_lib.FLAG_RELAY) == 0
    # one second stage per call
    for flags in (_lib.FLAG_RELAY | _lib.FLAG_OSD0, _lib.FLAG_RELAY | _lib.osd_flags("cs", 3),
                  _lib.FLAG_RELAY | _lib.FLAG_OSD_E | (2 << 16), _lib.FLAG_RELAY | _lib.FLAG_OSD_LARGE):
        assert run(flags) == -1
        with pytest.raises(_lib.QbpError) as e:
            dec.mc_run_weight(L, d, 3, prior, 0, 100, flags=flags)
        assert e.value.code == -1
    counters = fill.copy()                                  # the record limit of QBP_FLAG_OSD0
    assert lib.qbp_mc_run(dec._h, Lx.ctypes.data, Lx.shape[0], d, 0.05, 1, 0, 0, _lib.MC_OSD_MAX_TRIALS + 1,
                          prior.ctypes.data, MC_ITERS, 0, 1.0, 1.0, 20.0, _lib.FLAG_RELAY, counters.ctypes.data) == -1
    assert b"at most" in lib.qbp_last_error() and np.array_equal(counters, fill)
    # entries without a Relay stage
    probs = np.full(n, 0.05)
    for fn in (lambda: dec.mc_run_budgets(L, d, probs, prior, (4, 8), 0, 100, flags=_lib.FLAG_RELAY),
               lambda: dec.mc_run_spectrum(L, d, probs, prior, 0, 100, max_iter=8, flags=_lib.FLAG_RELAY),
               lambda: dec.mc_run_errors_spectrum(L, d, np.zeros((10, n), np.uint8), prior, max_iter=8,
                                                  flags=_lib.FLAG_RELAY),
               lambda: dec.decode_shots(L, np.zeros((10, 5), np.uint8), prior, max_iter=8, flags=_lib.FLAG_RELAY)):
        with pytest.raises(_lib.QbpError) as e:
            fn()
        assert e.value.code == _lib.E_UNSUPPORTED
    # a matrix whose state does not fit the LDS: 3 n doubles alone are 164 KiB
    wide = np.zeros((4, 7000), np.uint8)
    wide[np.arange(7000) % 4, np.arange(7000)] = 1
    big = fresh(wide)
    with pytest.raises(_lib.QbpError) as e:
        big.relay_configure(relay.RelayConfig(np.zeros((1, 7000)), [3]))
    assert e.value.code == _lib.E_UNSUPPORTED
    # the largest matrix the issue names as supported configures: the 864 x 2592 phenomenological one
    Hp, Lp, pr = dem.phenomenological("[[144, 12, 12]]", 12, 0.004)
    assert Hp.shape == (864, 2592)
    fresh(Hp).relay_configure(relay.RelayConfig(np.zeros((1, 2592)), [3]))
