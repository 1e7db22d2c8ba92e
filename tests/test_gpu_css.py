"""GPU: the two-stage CSS decoder (qbp_css_*) against its numpy statement (tests/css_oracle.py): the Pauli sampler
bit for bit, the Monte-Carlo counters [3][12] digit for digit, the decode against the composition of the ordinary
calls, and mc.run_depolarizing against the C call."""
import ctypes

import numpy as np
import pytest

import css_oracle as co
from qldpc_amd import _lib, bp, codes, css, mc

pytestmark = pytest.mark.gpu

MAX_ITER = 30
OSD = {"none": None, "osd0": 0, "cs7": ("cs", 7)}
# depolarizing strength per code, 2000 trials each: chosen on the CPU so that both sectors of the statement have at least
# five trials BP converges on and five it does not (asserted below)
CODES = {"72": ("[[72, 12, 6]]", 0.06, 2000), "hgp": (None, 0.06, 2000), "144": ("[[144, 12, 12]]", 0.07, 2000)}
CS7_TRIALS = 1000       # the numpy statement of order-w OSD takes up to 6 ms per record and sector B leaves most records
                        # to it: the first 1000 trials keep the test at a few seconds and the five of each
SEED, BEGIN = (9 << 32) + 5, (1 << 32) - 100


def flags_of(osd):
    return 0 if osd is None else _lib.osd_flags("cs", 0) if osd == 0 else _lib.osd_flags(osd[0], osd[1])


_SETUP = {}


def setup(tag):
    if tag not in _SETUP:
        name, p, T = CODES[tag]
        if name is None:
            Hx, Hz, Lx, Lz = co.hgp_steane()
            d = 3
        else:
            c = codes.load_code(name)
            Hx, Hz, Lx, Lz = (np.asarray(a, np.uint8) for a in (c.Hx, c.Hz, c.Lx, c.Lz))
            d = int(c.distance)
        n = Hx.shape[1]
        dec = _lib.CssDecoder(_lib.Decoder(*bp.csr_from_H(Hx), bp.DEVICE), _lib.Decoder(*bp.csr_from_H(Hz), bp.DEVICE))
        ea, eb = co.sample_pauli(n, p / 3, p / 3, p / 3, SEED, BEGIN, T)
        _SETUP[tag] = dict(Hx=Hx, Hz=Hz, Lx=Lx, Lz=Lz, d=d, n=n, p=p, T=T, dec=dec, ea=ea, eb=eb,
                           priors=css.pauli_priors(p / 3, p / 3, p / 3, n))
    return _SETUP[tag]


def test_sampler_equals_the_statement():
    s = setup("hgp")                       # n = 58: no multiple of 4
    dec, n = s["dec"], s["n"]
    for px, py, pz, seed, begin, T in [(0.05, 0.02, 0.11, (7 << 32) + 1, (1 << 32) - 9, 40), (0.0, 0.1, 0.2, 3, 0, 7),
                                       (0.1, 0.0, 0.2, 1 << 40, 5, 64), (0.3, 0.3, 0.4, 11, 1 << 33, 3),
                                       (0.0, 0.0, 0.0, 5, 17, 9), (0.2, 0.1, 0.0, 5, 17, 33)]:      # (buffers reused)
        got = dec.sample_errors(px, py, pz, begin, T, seed=seed)
        want = co.sample_pauli(n, px, py, pz, seed, begin, T)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (px, py, pz, seed, begin, T)
    a = dec.sample_errors(0.05, 0.02, 0.11, BEGIN, 30, seed=SEED)
    b = dec.sample_errors(0.05, 0.02, 0.11, BEGIN + 13, 17, seed=SEED)
    assert np.array_equal(a[0][13:], b[0]) and np.array_equal(a[1][13:], b[1])
    for bad in [(-0.1, 0, 0), (0.5, 0.4, 0.2), (float("nan"), 0, 0)]:
        with pytest.raises(_lib.QbpError) as e:
            dec.sample_errors(*bad, 0, 4)
        assert e.value.code == _lib.E_INVALID


@pytest.mark.parametrize("mode", ["none", "osd0", "cs7", "minsum", "minsum_osd0"])
@pytest.mark.parametrize("tag", list(CODES))
def test_mc_run_errors_equals_the_statement(tag, mode):
    s = setup(tag)
    minsum = mode.startswith("minsum")
    osd = OSD["osd0" if mode == "minsum_osd0" else "none" if minsum else mode]
    T = s["T"] if osd != ("cs", 7) else CS7_TRIALS
    ea, eb = s["ea"][:T], s["eb"][:T]
    kw = dict(max_iter=MAX_ITER, variant=_lib.MIN_SUM if minsum else _lib.SUM_PRODUCT, alpha=0.8 if minsum else 1.0,
              damping=1.0, clip_llr=20.0)
    want = co.counters(s["Hx"], s["Hz"], s["Lx"], s["Lz"], s["d"], ea, eb, *s["priors"], osd=osd, **kw)
    assert all(5 <= want[r][6] <= T - 5 for r in (0, 1)), want
    got = s["dec"].mc_run_errors(s["Lx"], s["Lz"], s["d"], ea, eb, *s["priors"], flags=flags_of(osd), **kw)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("mode", ["none", "osd0"])
def test_mc_run_equals_sampling_then_mc_run_errors(mode):
    """... and does not depend on the chunk size or on how the range is split."""
    s = setup("72")
    dec, p, T = s["dec"], s["p"], 700
    fl = flags_of(OSD[mode])
    ea, eb = co.sample_pauli(s["n"], p / 3, p / 3, p / 3, SEED, BEGIN, T)
    want = dec.mc_run_errors(s["Lx"], s["Lz"], s["d"], ea, eb, *s["priors"], max_iter=MAX_ITER, flags=fl)
    run = lambda a, b, counters=None: dec.mc_run(s["Lx"], s["Lz"], s["d"], p / 3, p / 3, p / 3, *s["priors"], BEGIN + a,
                                                 BEGIN + b, seed=SEED, max_iter=MAX_ITER, flags=fl, counters=counters)
    assert np.array_equal(run(0, T), want)
    split = run(0, 101)
    run(101, 102, split)
    run(102, T, split)
    assert np.array_equal(split, want)
    try:
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 129)           # six chunks
        assert np.array_equal(run(0, T), want)
        assert np.array_equal(dec.mc_run_errors(s["Lx"], s["Lz"], s["d"], ea, eb, *s["priors"], max_iter=MAX_ITER, flags=fl),
                              want)
    finally:
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)
    assert np.array_equal(run(5, 5), np.zeros((3, 12), np.int64))


@pytest.mark.parametrize("mode", ["none", "osd0", "minsum"])
@pytest.mark.parametrize("tag", ["72", "hgp"])
def test_equal_priors_are_two_independent_runs(tag, mode):
    """With prior_b1 == prior_b0 rows 0 and 1 are qbp_mc_run_errors on (Hx, Lx, e_a) and on (Hz, Lz, e_b), digit for
    digit -- [7] included: both sum the 0-based iteration of the BP stage.  [10] follows the sliding-window decoder's
    rule here (every correction that misses its syndrome) and qbp_mc_run_errors' there (OSD outputs only): without OSD
    it is [6] here and 0 there, and the test says so instead of skipping the counter."""
    s = setup(tag)
    minsum = mode == "minsum"
    fl = flags_of(OSD["none" if minsum else mode])
    kw = dict(max_iter=MAX_ITER, variant=_lib.MIN_SUM if minsum else _lib.SUM_PRODUCT, alpha=0.8 if minsum else 1.0,
              damping=1.0, clip_llr=20.0, flags=fl)
    p = s["p"]
    pa = s["priors"][0]
    pb = css.marginal_prior_b(p / 3, p / 3, p / 3, s["n"])
    got = s["dec"].mc_run_errors(s["Lx"], s["Lz"], s["d"], s["ea"], s["eb"], pa, pb, pb, **kw)
    for row, dec, L, e, prior in ((0, s["dec"].a, s["Lx"], s["ea"], pa), (1, s["dec"].b, s["Lz"], s["eb"], pb)):
        want = dec.mc_run_errors(L, s["d"], e, prior, **kw)
        assert want[10] == 0
        if not fl:
            want[10] = want[6]
        assert np.array_equal(got[row], want), (row, got[row], want)
    assert 5 <= got[0][6] and 5 <= got[1][6]


@pytest.mark.parametrize("mode", ["none", "osd0", "cs7"])
def test_decode_batch_is_the_composition_of_the_ordinary_calls(mode):
    s = setup("hgp")
    dec, osd = s["dec"], OSD[mode]
    B = 200
    rng = np.random.default_rng(4)
    syn_a = ((s["ea"][:B].astype(np.int64) @ s["Hx"].T) % 2).astype(np.uint8)
    syn_b = ((s["eb"][:B].astype(np.int64) @ s["Hz"].T) % 2).astype(np.uint8)
    syn_b[::17] ^= (rng.random((len(syn_b[::17]), syn_b.shape[1])) < 0.2).astype(np.uint8)    # (any syndrome is legal)
    pa, b0, b1 = s["priors"]
    xa, xb, ca, cb = dec.decode(syn_a, syn_b, pa, b0, b1, MAX_ITER, flags=flags_of(osd))

    def stage(d, syn, out):
        hard, conv, _, llr = out
        x = hard.copy()
        bad = np.flatnonzero(~conv)
        if osd is not None and bad.size:
            x[bad] = d.osd0(syn[bad], llr[bad], hard[bad]) if osd == 0 else d.osd(syn[bad], llr[bad], hard[bad], *osd)
        return x, conv
    want_a, conv_a = stage(dec.a, syn_a, dec.a.decode(syn_a, pa, MAX_ITER))
    want_b, conv_b = stage(dec.b, syn_b, dec.b.decode_cond(syn_b, want_a, b0, b1, MAX_ITER))
    assert np.array_equal(xa, want_a) and np.array_equal(ca, conv_a)
    assert np.array_equal(xb, want_b) and np.array_equal(cb, conv_b)
    assert 5 <= (~ca).sum() <= B - 5 and 5 <= (~cb).sum() <= B - 5
    # the wrapper of qldpc_amd.css decodes the same
    hi = css.CssDecoder(s["Hx"], s["Hz"])
    again = hi.decode(syn_a, syn_b, pa, b0, b1, MAX_ITER, osd=osd is not None, osd_method=osd[0] if osd else "cs",
                      osd_order=osd[1] if osd else 0)
    assert all(np.array_equal(x, y) for x, y in zip(again, (xa, xb, ca, cb)))
    got = css.performBeliefPropagationCond(s["Hz"], syn_b, want_a, b0, b1, MAX_ITER)
    assert all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in
               zip(got, dec.b.decode_cond(syn_b, want_a, b0, b1, MAX_ITER)))


def test_refusals():
    s = setup("hgp")
    dec = s["dec"]
    args = (s["Lx"], s["Lz"], s["d"], s["ea"][:8], s["eb"][:8], *s["priors"])
    for kw, code in [(dict(variant=_lib.DAMPED_SP), _lib.E_UNSUPPORTED), (dict(flags=_lib.FLAG_RELAY), _lib.E_UNSUPPORTED),
                     (dict(flags=_lib.FLAG_GD), _lib.E_UNSUPPORTED), (dict(flags=_lib.FLAG_LSD), _lib.E_UNSUPPORTED),
                     (dict(flags=_lib.FLAG_LAYERED), _lib.E_UNSUPPORTED), (dict(flags=_lib.FLAG_OSD_CS), _lib.E_INVALID),
                     (dict(max_iter=0), _lib.E_INVALID)]:
        with pytest.raises(_lib.QbpError) as e:
            dec.mc_run_errors(*args, **kw)
        assert e.value.code == code, kw
    nan = s["priors"][2].copy()
    nan[0] = np.nan
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_errors(*args[:5], s["priors"][0], s["priors"][1], nan)
    assert e.value.code == _lib.E_INVALID
    other = _lib.Decoder(*bp.csr_from_H(setup("72")["Hx"]), bp.DEVICE)
    with pytest.raises(ValueError):
        _lib.CssDecoder(dec.a, other)
    h = _lib._VP()
    assert _lib.load().qbp_css_create(dec.a._h, other._h, ctypes.byref(h)) == _lib.E_INVALID and not h.value


@pytest.mark.parametrize("correlated", [True, False])
def test_run_depolarizing_is_the_c_call(correlated):
    name, _, _ = CODES["72"]
    s = setup("72")
    ps, T = [0.03, 0.06], 400
    got = mc.run_depolarizing(name, ps, T, osd=True, correlated=correlated, seed=21, max_iter=MAX_ITER, device=bp.DEVICE)
    assert got.shape == (2, 3, 12) and got.dtype == np.int64
    for i, p in enumerate(ps):
        pa, b0, b1 = css.pauli_priors(p / 3, p / 3, p / 3, s["n"])
        if not correlated:
            b0 = b1 = css.marginal_prior_b(p / 3, p / 3, p / 3, s["n"])
        want = s["dec"].mc_run(s["Lx"], s["Lz"], s["d"], *mc.pauli_rates(p), pa, b0, b1, 0, T, seed=21, max_iter=MAX_ITER,
                               flags=_lib.FLAG_OSD0)
        assert np.array_equal(got[i], want), (p, got[i], want)
        if not correlated:      # the baseline path: sector B is an ordinary Monte-Carlo run on its own errors
            eb = s["dec"].sample_errors(*mc.pauli_rates(p), 0, T, seed=21)[1]
            assert np.array_equal(got[i][1], s["dec"].b.mc_run_errors(s["Lz"], s["d"], eb, b0, max_iter=MAX_ITER,
                                                                      flags=_lib.FLAG_OSD0))
