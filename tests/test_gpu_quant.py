"""GPU: bp_quant_kernel against the numpy statement of fixed-point min-sum (tests/quant_oracle.py), bit for bit -- the
batch build on seven matrices, four parameter sets, three iteration limits and two kinds of prior; the float
cross-check through qbp_decode_batch on integer priors; launch geometries into poisoned buffers; and the Monte-Carlo
build behind QBP_FLAG_QUANT, at 6 bits (int8 messages) and at 16 (int16), against statement + classification, alone and
under OSD, LSD and Relay-BP.  tests/test_gpu_quant_large.py goes on where these matrices end."""
import numpy as np
import pytest

import geometry_util as gu
import quant_cases as qc
import quant_oracle as qo
from oracle import oracle
from qldpc_amd import _lib, bp, codes, dem, quant, relay

pytestmark = pytest.mark.gpu

QUANT = _lib.FLAG_QUANT
NAMES = ("hard", "converged", "iters", "posterior_q", "llr")
LLR_POISON = -1.2345e300


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def cfg_of(params):
    bits, scale, num, shift, beta = params
    return quant.QuantConfig(bits, scale, (num, shift), beta)


class Outputs:
    """The five output tensors of a launch, rows + 3 rows each, poisoned before every launch."""

    def __init__(self, rows, n):
        t = gu.torch()
        R = rows + 3
        self.t = dict(hard=t.empty((R, n), dtype=t.uint8, device="cuda"), converged=t.empty(R, dtype=t.uint8, device="cuda"),
                      iters=t.empty(R, dtype=t.int32, device="cuda"),
                      posterior_q=t.empty((R, n), dtype=t.int32, device="cuda"),
                      llr=t.empty((R, n), dtype=t.float64, device="cuda"))
        self.poison = dict(hard=0xFF, converged=0xFF, iters=-1, posterior_q=-(2 ** 31), llr=LLR_POISON)

    def run(self, dec, syn_t, prior_t, B, max_iter, flags=0, nulls=(), stream=None):
        """Poison, launch on `stream` (default: torch's current one), sync; rows [0, B) written, the rest and the null
        outputs untouched.  Returns the numpy arrays (None for a null output)."""
        t = gu.torch()
        for k, x in self.t.items():
            x.fill_(self.poison[k])
        t.cuda.synchronize()
        p = {k: (0 if k in nulls else x.data_ptr()) for k, x in self.t.items()}
        dec.quant_decode_device(syn_t.data_ptr(), prior_t.data_ptr(), B, max_iter, flags, p["hard"], p["converged"],
                                p["iters"], p["posterior_q"], p["llr"], gu.stream_ptr() if stream is None else stream)
        t.cuda.synchronize()
        out = []
        for k in NAMES:
            x = self.t[k]
            lo = 0 if k in nulls else B
            assert bool((x[lo:] == self.poison[k]).all().item()), f"{k} written beyond row {lo}"
            if k in nulls:
                out.append(None)
                continue
            a = x[:B].cpu().numpy()
            assert not (a == self.poison[k]).any(), f"{k}: a record never got its output"
            out.append(a.astype(bool) if k == "converged" else a)
        return tuple(out)


def assert_same(got, want, what):
    for k, x, y in zip(NAMES, got, want):
        if x is None:
            continue
        assert x.dtype == np.asarray(y).dtype and x.shape == y.shape, (what, k, x.dtype, x.shape)
        same = x.view(np.uint64) == y.view(np.uint64) if k == "llr" else x == y
        if not same.all():
            rows = np.flatnonzero(~same.reshape(len(x), -1).all(axis=1))
            raise AssertionError(f"{what}: {k} differs on {len(rows)} of {len(x)} records, first {rows[:8]}")


# ---- 1. the batch build against the statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("name", qc.MATRICES)
def test_batch_kernel_equals_statement(name, kind):
    H, _, syn, prior = qc.case(name, kind)
    B, n = len(syn), H.shape[1]
    dec = fresh(H)
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = Outputs(B, n)
    for params in qc.PARAMS:
        dec.quant_configure(cfg_of(params))         # (a second, third, fourth configuration on the same handle)
        for max_iter in qc.MAX_ITERS:
            want = qc.statement(name, kind, params, max_iter)
            got = out.run(dec, syn_t, prior_t, B, max_iter)
            assert_same(got, want, f"{name} {kind} {params} max_iter {max_iter}")
            assert dec.info("last_kernel") == 5 and dec.info("threads") == 256
            wide = params[0] > 8
            assert dec.info("lds_bytes") % 4 == 0 and dec.info("lds_bytes") >= quant.lds_bytes(*H.shape, int(H.sum()), 1, wide)


def test_issue_records_and_host_entry():
    H, _, syn, prior = qc.issue_case()
    dec = fresh(H)
    for params in qc.PARAMS:
        want = qo.decode_batch(H, syn, prior, 30, *params)
        hard, conv, iters, llr, post = quant.performQuantMinSumBatch(H, syn, prior, cfg_of(params), 30)
        assert_same((hard, conv, iters, post, llr), want, f"host entry {params}")
        dec.quant_configure(cfg_of(params))
        one = dec.quant_decode(syn[7:8], prior, 30, want_posterior=False, want_llr=False)
        assert one[3] is None and one[4] is None
        assert np.array_equal(one[0], want[0][7:8]) and one[1][0] == want[1][7] and one[2][0] == want[2][7]
    h, c, v, it = quant.performQuantMinSum(H, syn[5], prior, cfg_of(qc.PARAMS[1]), 30)
    want = qo.decode_batch(H, syn[5:6], prior, 30, *qc.PARAMS[1])
    assert h.dtype == np.int8 and np.array_equal(h, want[0][0]) and c == bool(want[1][0]) and it == int(want[2][0])
    assert np.array_equal(v, want[4][0])
    # a NaN prior: refused at the host entry, rule 1 (P = 0) at the device entry
    nan = prior.copy(); nan[9] = np.nan
    with pytest.raises(_lib.QbpError) as e:
        dec.quant_decode(syn, nan, 30)
    assert e.value.code == _lib.E_INVALID
    dec.quant_configure(cfg_of(qc.PARAMS[2]))
    got = Outputs(len(syn), 72).run(dec, gu.to_device(syn), gu.to_device(nan), len(syn), 30)
    assert_same(got, qo.decode_batch(H, syn, nan, 30, *qc.PARAMS[2]), "NaN prior, device entry")


def test_float_min_sum_on_integer_priors():
    """q = 16, scale 1, alpha 1 / 1, beta 0 on integer priors equals qbp_decode_batch(QBP_MIN_SUM, 1.0, 1.0, 32767): hard,
    converged and iters equal, llr numerically equal."""
    H = qc.matrix("72")
    rng = np.random.default_rng(11)
    errors = (rng.random((60, 72)) < 0.08).astype(np.uint8)
    prior = rng.integers(2, 6, 72).astype(np.float64)
    syn = qc.syndromes_of(H, errors)
    dec = fresh(H)
    f_hard, f_conv, f_iters, f_llr = dec.decode(syn, prior, 30, _lib.MIN_SUM, 1.0, 1.0, 32767.0)
    dec.quant_configure(quant.QuantConfig(16, 1.0))
    hard, conv, iters, post, llr = dec.quant_decode(syn, prior, 30)
    print("classes", qc.classes(conv, iters))
    assert min(qc.classes(conv, iters)) >= 4
    assert np.array_equal(hard, f_hard) and np.array_equal(conv, f_conv) and np.array_equal(iters, f_iters)
    assert np.array_equal(llr, f_llr) and np.array_equal(post.astype(np.float64), llr)


# ---- 2. launch geometry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72", "irr37", "disjoint70"])
def test_outputs_do_not_depend_on_batch_grid_slots_or_stream(name):
    H, _, syn0, prior = qc.case(name, "mixed")
    n = H.shape[1]
    dec = fresh(H)
    cus = dec.info("num_cu")
    big = 3 * 2 * cus * 3 + 5                       # several passes of a grid of 2 workgroups per CU with 3 slots
    syn = syn0[np.arange(big) % len(syn0)]
    prior_t = gu.to_device(prior)
    side = gu.torch().cuda.Stream()
    for params in (qc.PARAMS[0], qc.PARAMS[3]):
        dec.quant_configure(cfg_of(params))
        w = qc.statement(name, "mixed", params, 30)
        want = tuple(x[np.arange(big) % len(syn0)] for x in w)
        for slots, per_cu, B, stream in ((0, 0, big, None), (1, 1, cus - 1, None), (3, 2, big, None), (0, 0, 1, None),
                                         (2, 0, 37, side.cuda_stream), (32, 0, len(syn0), None)):
            dec.set_option(_lib.OPT_QUANT_SLOTS, slots)
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
            rows = np.arange(big - B, big)
            out = Outputs(B, n)
            got = out.run(dec, gu.to_device(syn[rows]), prior_t, B, 30, stream=stream)
            assert_same(got, tuple(x[rows] for x in want), f"{name} {params} slots {slots} per_cu {per_cu} B {B}")
            if per_cu:
                assert dec.info("grid") <= per_cu * cus
            # null optional outputs stay untouched, the others are the same
            got = out.run(dec, gu.to_device(syn[rows]), prior_t, B, 30, nulls=("converged", "iters", "posterior_q", "llr"))
            assert np.array_equal(got[0], want[0][rows])
            got = out.run(dec, gu.to_device(syn[rows]), prior_t, B, 30, nulls=("posterior_q",))
            assert_same(got, tuple(x[rows] for x in want), "posterior_q null")
        dec.set_option(_lib.OPT_QUANT_SLOTS, 0)
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)


@pytest.mark.parametrize("name", ["72", "rows"])
def test_force_full_returns_the_early_exit_bits(name):
    H, _, syn, prior = qc.case(name, "uniform")
    B, n = len(syn), H.shape[1]
    dec = fresh(H)
    syn_t, prior_t = gu.to_device(syn), gu.to_device(prior)
    out = Outputs(B, n)
    for params in qc.PARAMS:
        dec.quant_configure(cfg_of(params))
        for max_iter in (1, 30):
            got = out.run(dec, syn_t, prior_t, B, max_iter, flags=_lib.FLAG_FORCE_FULL | _lib.FLAG_FAST_MATH)
            assert_same(got, qc.statement(name, "uniform", params, max_iter), f"{name} forced {params} {max_iter}")


# ---- 3. Monte-Carlo -------------------------------------------------------------------------------------------------------------
MC_ITERS = 12
MC_PARAMS = qc.PARAMS[1]                    # 6 bits: bp_quant_kernel<int8_t, true>
MC_PARAMS_WIDE = qc.PARAMS[3]               # 16 bits: bp_quant_kernel<int16_t, true>


def mc_case(name):
    """(H, L, distance, errors, prior, probs)"""
    if name == "pheno":
        Hs, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.03, 0.06)          # two-valued column probabilities
        H = np.asarray(Hs.todense()).astype(np.uint8)
        d = 6
    else:
        H = qc.matrix(name)
        if name == "irr37":
            L, d = (np.random.default_rng(3).random((3, 37)) < 0.3).astype(np.uint8), 4
        else:
            c = codes.load_code("[[72, 12, 6]]")
            L, d = np.asarray(c.Lx).astype(np.uint8), c.distance
        probs = np.where(np.arange(H.shape[1]) % 3 == 0, 0.09, 0.05)
    n = H.shape[1]
    prior = np.log((1 - probs) / probs)
    errors = (np.random.default_rng(23).random((160, n)) < probs[None, :] * 1.3).astype(np.uint8)
    return H, np.ascontiguousarray(L, np.uint8), d, errors, prior, probs


def expected(H, L, d, errors, prior, params=MC_PARAMS):
    syn = qc.syndromes_of(H, errors)
    hard, conv, iters, V, llr = qo.decode_batch(H, syn, prior, MC_ITERS, *params)
    return oracle.classify_trials(H, L, d, errors, syn, hard, conv, iters), (syn, hard, conv, iters, llr)


MC_NAMES = ("72", "irr37", "pheno")
MC_STAGES = ("osd0", "cs7", "lsd", "relay")


def mc_id(*parts, params):
    """The 6-bit runs keep the ids they had before the 16-bit ones (the int16 Monte-Carlo build) joined them."""
    return "-".join(parts) + ("" if params is MC_PARAMS else f"-q{params[0]}")


@pytest.mark.parametrize("name,params", [pytest.param(nm, p, id=mc_id(nm, params=p)) for p in (MC_PARAMS, MC_PARAMS_WIDE)
                                         for nm in MC_NAMES])
def test_mc_counters_equal_statement_and_classification(name, params):
    H, L, d, errors, prior, probs = mc_case(name)
    want, (_, _, conv, _, _) = expected(H, L, d, errors, prior, params)
    dec = fresh(H)
    dec.quant_configure(cfg_of(params))
    # (alpha, damping and the clip of the call are not read)
    kw = dict(max_iter=MC_ITERS, variant=_lib.MIN_SUM, alpha=0.3, damping=0.5, clip_llr=1.0, flags=QUANT)
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert 8 <= int((~conv).sum()) < len(errors)
    assert np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, d, errors[:31], prior, **kw) + dec.mc_run_errors(L, d, errors[31:], prior, **kw), want)
    dec.set_option(_lib.OPT_QUANT_SLOTS, 1)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, flags=QUANT | _lib.FLAG_FORCE_FULL | _lib.FLAG_FAST_MATH,
                                            max_iter=MC_ITERS, variant=_lib.MIN_SUM), want)
    dec.set_option(_lib.OPT_QUANT_SLOTS, 0)
    # the sampled entries on their samplers' errors: the whole range, a split of it, several chunks per call
    T, w = 96, max(2, H.shape[1] // 14)
    runs = [(dec.mc_sample_errors(0.07, 5, T, seed=9), lambda a, b: dec.mc_run(L, d, 0.07, prior, a, b, seed=9, **kw)),
            (dec.mc_sample_errors_probs(probs, 5, T, seed=9), lambda a, b: dec.mc_run_probs(L, d, probs, prior, a, b, seed=9, **kw)),
            (dec.mc_sample_errors_weight(w, 5, T, seed=9), lambda a, b: dec.mc_run_weight(L, d, w, prior, a, b, seed=9, **kw))]
    for errs, run in runs:
        want_s, _ = expected(H, L, d, errs, prior, params)
        assert np.array_equal(run(5, 5 + T), want_s)
        assert np.array_equal(run(5, 6) + run(6, 50) + run(50, 5 + T), want_s)
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 7)
        assert np.array_equal(run(5, 5 + T), want_s)
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)


@pytest.mark.parametrize("name,stage,params", [pytest.param(nm, st, p, id=mc_id(nm, st, params=p))
                                               for p in (MC_PARAMS, MC_PARAMS_WIDE) for st in MC_STAGES for nm in MC_NAMES])
def test_second_stages_act_on_the_quant_failure_records(name, stage, params):
    """Counters = the statement -> qbp_osd_batch / qbp_lsd_batch / qbp_relay_decode_batch on its failures, with
    llr = (double)V -> numpy classification."""
    H, L, d, errors, prior, _ = mc_case(name)
    n = H.shape[1]
    _, (syn, hard, conv, iters, llr) = expected(H, L, d, errors, prior, params)
    f = np.flatnonzero(~conv)
    assert len(f) >= 8
    dec = fresh(H)
    dec.quant_configure(cfg_of(params))
    det = hard.copy()
    if stage == "relay":
        cfg = relay.RelayConfig(relay.relay_gammas(n, 3, 0.125, (-0.24, 0.66), 4), [10] * 3, 1, 0.9)
        r_hard, r_conv = dec.relay_decode(syn[f], prior, cfg)[:2]
        det[f] = r_hard
        invalid = int((~r_conv).sum())
        flags = QUANT | _lib.FLAG_RELAY
    else:
        if stage == "osd0":
            det[f] = dec.osd0(syn[f], llr[f], hard[f])
            flags = QUANT | _lib.FLAG_OSD0
        elif stage == "cs7":
            det[f] = dec.osd(syn[f], llr[f], hard[f], method="cs", order=7)
            flags = QUANT | _lib.FLAG_OSD0 | _lib.osd_flags("cs", 7)
        else:
            det[f] = dec.lsd(syn[f], llr[f], hard[f], 1)[0]
            flags = QUANT | _lib.FLAG_LSD
        invalid = int((qc.syndromes_of(H, det[f]) != syn[f]).any(1).sum())
    want = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    want[10] = invalid
    got = dec.mc_run_errors(L, d, errors, prior, max_iter=MC_ITERS, variant=_lib.MIN_SUM, flags=flags)
    print(stage, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[6] == len(f)
    assert np.array_equal(got, want)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_are_host_only_and_leave_outputs_untouched():
    H, _, syn, prior = qc.issue_case()
    n = 72
    c = codes.load_code("[[72, 12, 6]]")
    L, d = np.ascontiguousarray(c.Lx, np.uint8), c.distance
    lib = _lib.load()
    dec = fresh(H)
    fill = np.full(12, 7, np.int64)
    probs = np.full(n, 0.05)
    MS = _lib.MIN_SUM

    def code_of(fn):
        with pytest.raises(_lib.QbpError) as e:
            fn()
        return e.value.code

    def mc_rc(flags, variant=MS, pr=prior):
        counters = fill.copy()
        rc = lib.qbp_mc_run(dec._h, L.ctypes.data, L.shape[0], d, 0.05, 1, 0, 0, 50, pr.ctypes.data, 8, variant, 1.0, 1.0,
                            20.0, flags, counters.ctypes.data)
        assert rc == 0 or np.array_equal(counters, fill)
        return rc

    def batch_rc(flags=0, pr=prior, max_iter=8):
        hard = np.full((len(syn), n), 0xEE, np.uint8)
        rc = lib.qbp_quant_decode_batch(dec._h, syn.ctypes.data, pr.ctypes.data, len(syn), max_iter, flags, hard.ctypes.data,
                                        None, None, None, None)
        assert rc == 0 or (hard == 0xEE).all()
        return rc

    # without a configuration
    assert batch_rc() == _lib.E_INVALID and b"qbp_quant_configure" in lib.qbp_last_error()
    assert mc_rc(QUANT) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_errors(L, d, np.zeros((4, n), np.uint8), prior, variant=MS, flags=QUANT)) == _lib.E_INVALID
    # parameters out of range configure nothing
    for bad in ((1, 1.0, 1, 0, 0), (17, 1.0, 1, 0, 0), (4, 0.0, 1, 0, 0), (4, float("inf"), 1, 0, 0), (4, float("nan"), 1, 0, 0),
                (4, 1.0, 0, 2, 0), (4, 1.0, 5, 2, 0), (4, 1.0, 1, 16, 0), (4, 1.0, 1, -1, 0), (4, 1.0, 1, 0, 8), (4, 1.0, 1, 0, -1)):
        assert lib.qbp_quant_configure(dec._h, *bad) == _lib.E_INVALID, bad
    assert mc_rc(QUANT) == _lib.E_INVALID
    dec.quant_configure(cfg_of(qc.PARAMS[1]))
    assert mc_rc(QUANT) == 0 and batch_rc() == 0
    # the other first stage, other variants, column-sum orders, unknown bits of the batch entry, max_iter
    dec.layered_configure(None)
    assert mc_rc(QUANT | _lib.FLAG_LAYERED) == _lib.E_INVALID
    assert mc_rc(QUANT, variant=_lib.SUM_PRODUCT) == _lib.E_INVALID and mc_rc(QUANT, variant=_lib.DAMPED_SP) == _lib.E_INVALID
    for colsum in (_lib.FLAG_PAIRWISE_COLSUM, _lib.FLAG_DENSE_F_COLSUM, _lib.FLAG_DENSE_F_COLSUM_ITER0):
        assert mc_rc(QUANT | colsum) == _lib.E_INVALID
        assert batch_rc(colsum) == _lib.E_INVALID
    assert batch_rc(QUANT) == _lib.E_INVALID and batch_rc(_lib.FLAG_OSD0) == _lib.E_INVALID and batch_rc(max_iter=0) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_weight(L, d, 3, prior, 0, 10, variant=_lib.SUM_PRODUCT, flags=QUANT)) == _lib.E_INVALID
    # a NaN prior at the host entries (+-inf are legal)
    nan = prior.copy(); nan[5] = np.nan
    inf = prior.copy(); inf[5] = np.inf
    assert batch_rc(pr=nan) == _lib.E_INVALID and batch_rc(pr=inf) == 0
    assert mc_rc(QUANT, pr=nan) == _lib.E_INVALID and mc_rc(QUANT, pr=inf) == 0
    assert code_of(lambda: dec.mc_run_errors(L, d, np.zeros((4, n), np.uint8), nan, variant=MS, flags=QUANT)) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_probs(L, d, probs, nan, 0, 10, variant=MS, flags=QUANT)) == _lib.E_INVALID
    assert code_of(lambda: dec.mc_run_weight(L, d, 3, nan, 0, 10, variant=MS, flags=QUANT)) == _lib.E_INVALID
    # entries without a fixed-point build
    for fn in (lambda: dec.mc_run_budgets(L, d, probs, prior, (4, 8), 0, 100, variant=MS, flags=QUANT),
               lambda: dec.mc_run_spectrum(L, d, probs, prior, 0, 100, max_iter=8, variant=MS, flags=QUANT),
               lambda: dec.mc_run_errors_spectrum(L, d, np.zeros((10, n), np.uint8), prior, max_iter=8, variant=MS, flags=QUANT),
               lambda: dec.mc_run_errors_llr_hist(L, d, np.zeros((10, n), np.uint8), prior, (4, 8), 16, (-30.0, 30.0),
                                                  variant=MS, flags=QUANT),
               lambda: dec.decode_shots(L, np.zeros((10, 5), np.uint8), prior, max_iter=8, variant=MS, flags=QUANT),
               lambda: dec.check_messages(syn[:2], prior, MS, flags=QUANT),
               lambda: dec.decode(syn, prior, 8, MS, flags=QUANT),
               lambda: dec.decode_cond(syn, np.zeros((len(syn), n), np.uint8), prior, prior, 8, MS, flags=QUANT)):
        assert code_of(fn) == _lib.E_UNSUPPORTED
    # the option's range
    assert code_of(lambda: dec.set_option(_lib.OPT_QUANT_SLOTS, 33)) == _lib.E_INVALID
    assert code_of(lambda: dec.set_option(_lib.OPT_QUANT_SLOTS, -1)) == _lib.E_INVALID


def test_window_and_css_entries_refuse_the_flag():
    from qldpc_amd import window
    Hs, L, probs = dem.phenomenological("[[72, 12, 6]]", 3, 0.03)
    H = np.asarray(Hs.todense()).astype(np.uint8)
    rounds = np.repeat(np.arange(3), 36).astype(np.int32)
    wdec = window.decoder_for(H, rounds, 2, 1, device=bp.DEVICE)
    prior = np.log((1 - probs) / probs)
    with pytest.raises(_lib.QbpError) as e:
        wdec.decode(np.zeros((2, H.shape[0]), np.uint8), prior, 8, variant=_lib.MIN_SUM, flags=QUANT)
    assert e.value.code == _lib.E_UNSUPPORTED
    c = codes.load_code("[[72, 12, 6]]")
    cdec = _lib.CssDecoder(fresh(np.asarray(c.Hx, np.uint8)), fresh(np.asarray(c.Hz, np.uint8)))
    pa = np.full(72, 3.0)
    with pytest.raises(_lib.QbpError) as e:
        cdec.decode(np.zeros((2, 36), np.uint8), np.zeros((2, 36), np.uint8), pa, pa, pa, 8, _lib.MIN_SUM, flags=QUANT)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_matrix_just_past_the_lds_limit_is_refused():
    """QBP_INFO_LDS_BYTES' formula restated: 4 * (even(n + S * (n + ceil(E * w / 4))) + 32 + S * slot_words(m)) bytes,
    w = 1 for q <= 8 and 2 above, even() rounds up to even, slot_words(m) = (10 + ceil(m / 32) + 1) rounded down to even."""
    def lds(m, n, E, S, wide):
        state = (n + S * (n + (E * (2 if wide else 1) + 3) // 4) + 1) & ~1
        return 4 * (state + 32 + S * ((10 + (m + 31) // 32 + 1) & ~1))
    assert lds(36, 72, 216, 1, False) == quant.lds_bytes(36, 72, 216, 1, False)
    assert lds(72, 216, 540, 1, False) == quant.lds_bytes(72, 216, 540, 1, False) == 4 * (568 + 32 + 14)
    limit = 160 * 1024
    m = 4
    # one entry per column: E = n; the largest n that fits at 16 bits, and the next one
    n_fit = max(n for n in range(15000, 20000) if lds(m, n, n, 1, True) <= limit)
    assert lds(m, n_fit + 2, n_fit + 2, 1, True) > limit
    for n, ok in ((n_fit, True), (n_fit + 2, False)):
        H = np.zeros((m, n), np.uint8)
        H[np.arange(n) % m, np.arange(n)] = 1
        dec = fresh(H)
        if ok:
            dec.quant_configure(quant.QuantConfig(16, 4.0, (3, 2)))
            syn = np.zeros((2, m), np.uint8); syn[1, 2] = 1
            prior = np.full(n, 1.5)
            got = dec.quant_decode(syn, prior, 3)
            assert_same((got[0], got[1], got[2], got[3], got[4]), qo.decode_batch(H, syn, prior, 3, 16, 4.0, 3, 2, 0), "at the limit")
            assert dec.info("lds_bytes") == lds(m, n, n, 1, True)
        else:
            with pytest.raises(_lib.QbpError) as e:
                dec.quant_configure(quant.QuantConfig(16, 4.0, (3, 2)))
            assert e.value.code == _lib.E_UNSUPPORTED
            dec.quant_configure(quant.QuantConfig(8, 4.0, (3, 2)))          # (int8 messages still fit)
