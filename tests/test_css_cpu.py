"""CPU: the numpy statement of the two-stage CSS decoder (tests/css_oracle.py) and the host-side pieces of
qldpc_amd.css -- no GPU."""
import numpy as np
import pytest

import css_oracle as co
from oracle import oracle
from qldpc_amd import codes, css, mc


@pytest.mark.parametrize("p", [0.003, 0.01, 0.03, 0.1])
def test_pauli_priors_depolarizing(p):
    pa, b0, b1 = css.pauli_priors(p / 3, p / 3, p / 3, 5)
    assert pa.shape == b0.shape == b1.shape == (5,)
    assert (b1 == 0.0).all() and not np.signbit(b1).any()
    # Equality of bits cannot hold: pauli_priors sees px, py, pz, not p.  p / 3 is rounded, 1 - px - py - pz is three
    # rounded subtractions of it and the quotient a fifth rounding, where 3 (1 - p) / p has three roundings of other
    # values: the two arguments of the log differ by at most 8 half-ulps, 8 * 2^-53 relative, which is at most that much
    # absolute in the log, plus the log's own rounding on either side.  The values lie in [3.3, 6.9], where an ulp is
    # 2^-51 or 2^-50: four ulp bound it.
    def within_ulps(x, ref, k):
        return bool((np.abs(x - ref) <= k * np.spacing(np.abs(ref))).all())
    assert within_ulps(b0, np.log(3 * (1 - p) / p), 4)
    assert within_ulps(pa, np.log((1 - 2 * p / 3) / (2 * p / 3)), 4)
    assert within_ulps(css.marginal_prior_b(p / 3, p / 3, p / 3, 5), pa, 4)


def test_pauli_priors_biased_and_refusals():
    pa, b0, b1 = css.pauli_priors(0.01, 0.002, 0.03, 2)
    assert np.allclose(pa, np.log((1 - 0.032) / 0.032)) and np.allclose(b0, np.log((1 - 0.042) / 0.01))
    assert np.allclose(b1, np.log(0.03 / 0.002))
    assert css.pauli_priors(0.0, 0.0, 0.1, 1)[1][0] == np.inf          # no X: sector B is certain without a flag
    for bad in [(-0.1, 0, 0), (0.5, 0.4, 0.2)]:
        with pytest.raises(ValueError):
            css.pauli_priors(*bad, 3)
    assert np.allclose(mc.pauli_rates(0.03), (0.01, 0.01, 0.01)) and mc.pauli_rates(0.1, (0, 0, 1)) == (0.0, 0.0, 0.1)
    with pytest.raises(ValueError):
        mc.pauli_rates(0.1, (0, 0, 0))


def test_sampler_frequencies():
    px, py, pz = 0.05, 0.02, 0.11
    n, T = 500, 400                                     # 2e5 qubits
    ea, eb = co.sample_pauli(n, px, py, pz, seed=(5 << 32) + 17, trial_begin=3, T=T)
    N = n * T
    got = {"x": int((eb & ~ea & 1).sum()), "y": int((ea & eb).sum()), "z": int((ea & ~eb & 1).sum())}
    for name, p in (("x", px), ("y", py), ("z", pz)):
        sigma = np.sqrt(N * p * (1 - p))
        assert abs(got[name] - N * p) < 5 * sigma, (name, got[name], N * p, sigma)
    none = N - sum(got.values())
    p0 = 1 - px - py - pz
    assert abs(none - N * p0) < 5 * np.sqrt(N * p0 * (1 - p0))


def test_sampler_rows_do_not_depend_on_the_split():
    n, begin, T = 37, (1 << 32) - 5, 11                 # trial indices across 2^32, n no multiple of 4
    args = (n, 0.1, 0.05, 0.2, 1234567890123)
    ea, eb = co.sample_pauli(*args, begin, T)
    assert ea.any() and eb.any() and (ea != eb).any()
    for cut in (1, 5, 6, 10):
        a0, b0 = co.sample_pauli(*args, begin, cut)
        a1, b1 = co.sample_pauli(*args, begin + cut, T - cut)
        assert np.array_equal(np.vstack([a0, a1]), ea) and np.array_equal(np.vstack([b0, b1]), eb)
    # the stream is this sampler's own: counter word 3, not the Bernoulli draws' 0 and 1
    assert not np.array_equal(ea, oracle.mc_errors(n, 0.3, 1, args[-1], begin, T))
    z_only = co.sample_pauli(n, 0.0, 0.0, 0.3, args[-1], begin, T)
    assert not z_only[1].any() and z_only[0].any()
    assert not any(x.any() for x in co.sample_pauli(n, 0.0, 0.0, 0.0, 1, 0, 4))


def test_hgp_helper():
    Hx, Hz, Lx, Lz = co.hgp_steane()
    assert Hx.shape == Hz.shape == (21, 58) and Lx.shape == Lz.shape == (16, 58)
    i64 = lambda a: a.astype(np.int64)
    assert not (i64(Hx) @ i64(Hz).T % 2).any()
    assert not (i64(Hx) @ i64(Lz).T % 2).any() and not (i64(Hz) @ i64(Lx).T % 2).any()
    assert co.gf2_rank(i64(Lx) @ i64(Lz).T % 2) == 16
    for H in (Hx, Hz):
        w = H.sum(axis=0)
        assert w.min() >= 1 and len(set(w.tolist())) > 1      # irregular column weights


def test_hgp_steane_is_the_product_of_the_steane_matrix_with_itself():
    """hgp(STEANE, STEANE) returns the four arrays of the construction hgp_steane() had before hgp() existed, stated
    here again, byte for byte (shape and dtype included)."""
    H = co.STEANE_H
    r, n = H.shape
    Hx = np.hstack([np.kron(H, np.eye(n, dtype=np.uint8)), np.kron(np.eye(r, dtype=np.uint8), H.T)]) & 1
    Hz = np.hstack([np.kron(np.eye(n, dtype=np.uint8), H), np.kron(H.T, np.eye(r, dtype=np.uint8))]) & 1
    old = (Hx.astype(np.uint8), Hz.astype(np.uint8), co.logicals(Hz, Hx), co.logicals(Hx, Hz))
    for got in (co.hgp_steane(), co.hgp(co.STEANE_H, co.STEANE_H)):
        assert len(got) == 4
        for x, y in zip(got, old):
            assert x.dtype == y.dtype == np.uint8 and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("tag", ["wide_a", "wide_b"])
def test_hgp_asymmetric_pair(tag):
    Hx, Hz, Lx, Lz = co.hgp_asymmetric(tag)
    small, large = ((15, 47), (28, 47))
    assert (Hx.shape, Hz.shape) == ((small, large) if tag == "wide_a" else (large, small))
    assert Lx.shape == Lz.shape == (4, 47) and all(a.dtype == np.uint8 for a in (Hx, Hz, Lx, Lz))
    i64 = lambda a: a.astype(np.int64)
    assert not (i64(Hx) @ i64(Hz).T % 2).any()
    assert not (i64(Hx) @ i64(Lz).T % 2).any() and not (i64(Hz) @ i64(Lx).T % 2).any()
    k = 47 - co.gf2_rank(Hx) - co.gf2_rank(Hz)
    assert k == 4 and co.gf2_rank(i64(Lx) @ i64(Lz).T % 2) == k
    # the 15-row matrix: column weights 1 .. 3, rows up to 6; the 28-row matrix: columns 1 .. 4, rows up to 5
    H15, H28 = (Hx, Hz) if tag == "wide_a" else (Hz, Hx)
    assert (H15.sum(axis=0).min(), H15.sum(axis=0).max(), H15.sum(axis=1).max()) == (1, 3, 6)
    assert (H28.sum(axis=0).min(), H28.sum(axis=0).max(), H28.sum(axis=1).max()) == (1, 4, 5)
    # the sizes the kernels' loops do not divide
    assert 47 % 4 and 47 % 64 and 15 % 32 and 28 % 32
    other = co.hgp_asymmetric("wide_b" if tag == "wide_a" else "wide_a")
    assert other[0].shape == Hz.shape and other[1].shape == Hx.shape


def test_biased_priors():
    """The per-qubit priors of the asymmetric tests: three different vectors, none constant, prior_b1 of both signs --
    and the values the formulas of css.pauli_priors give qubit by qubit."""
    pa, b0, b1 = co.biased_priors(47)
    assert pa.shape == b0.shape == b1.shape == (47,) and all(np.isfinite(p).all() for p in (pa, b0, b1))
    assert (b1 < 0).sum() == 3 and (b1 > 0).sum() == 44
    assert abs(b1.min() - -0.108) < 1e-3 and abs(b1.max() - 1.310) < 1e-3
    assert not np.array_equal(pa, b0) and not np.array_equal(pa, b1) and not np.array_equal(b0, b1)
    assert all(len(set(p.tolist())) == 47 for p in (pa, b0, b1))
    rng = np.random.default_rng(7)
    px, py, pz = (0.02 * rng.uniform(0.8, 1.25, 47), 0.015 * rng.uniform(0.5, 2.0, 47), 0.03 * rng.uniform(0.8, 1.25, 47))
    for v in range(47):
        one = css.pauli_priors(px[v], py[v], pz[v], 1)
        assert (one[0][0], one[1][0], one[2][0]) == (pa[v], b0[v], b1[v])


def test_classify_is_the_tail_of_counters():
    Hx, Hz, Lx, Lz = co.hgp_asymmetric("wide_b")
    pri = co.biased_priors(47)
    ea, eb = co.sample_pauli(47, *co.BIASED_RATES, 5, 0, 150)
    dec = co.decode(Hx, Hz, co._syn(Hx, ea), co._syn(Hz, eb), *pri, max_iter=10, osd=0)
    want = co.counters(Hx, Hz, Lx, Lz, 3, ea, eb, *pri, max_iter=10, osd=0)
    assert np.array_equal(co.classify(Hx, Hz, Lx, Lz, 3, ea, eb, dec), want) and want[2][1] > 0
    none = co.classify(Hx, Hz, Lx[:0], Lz, 3, ea, eb, dec)
    assert not none[0][[1, 3, 4, 8]].any() and np.array_equal(none[1], want[1]) and none[2][1] == want[1][1]


@pytest.mark.parametrize("mode", ["none", "osd0", "cs7", "minsum", "minsum_osd0"])
def test_asymmetric_inputs_tell_the_sectors_apart(mode):
    """The inputs of tests/test_gpu_css_shapes.py on the statement alone: both orientations leave at least five trials
    to either outcome of BP in both sectors, their counters differ, and so do rows 0 and 1 of each."""
    got = {}
    for tag in ("wide_a", "wide_b"):
        s = co.asym_inputs(tag)
        want = co.asym_statement(tag, mode)
        assert all(5 <= want[r][6] <= co.ASYM_T - 5 for r in (0, 1)), (tag, want)
        assert want[0][0] == want[1][0] == want[2][0] == co.ASYM_T
        assert not np.array_equal(want[0], want[1]), (tag, want)
        assert want[0][6] != want[1][6] and want[0][1] != want[1][1]
        assert s["Hx"].shape[0] != s["Hz"].shape[0]
        got[tag] = want
    assert not np.array_equal(got["wide_a"], got["wide_b"])
    assert not np.array_equal(got["wide_a"][0], got["wide_b"][0]) and not np.array_equal(got["wide_a"][1], got["wide_b"][1])


@pytest.mark.parametrize("tag", ["wide_a", "wide_b"])
def test_asymmetric_decode_batch_inputs(tag):
    """The perturbed syndromes of the decode test leave five records to either outcome in both sectors."""
    s = co.asym_inputs(tag)
    syn_a, syn_b = co.asym_batch_syndromes(s)
    assert syn_a.shape == (co.ASYM_B, s["Hx"].shape[0]) and syn_b.shape == (co.ASYM_B, s["Hz"].shape[0])
    assert (syn_a[::13] != co._syn(s["Hx"], s["ea"][:co.ASYM_B])[::13]).any(axis=1).sum() >= 5
    assert (syn_b[::17] != co._syn(s["Hz"], s["eb"][:co.ASYM_B])[::17]).any(axis=1).sum() >= 5
    _, _, ca, cb, _, _ = co.decode(s["Hx"], s["Hz"], syn_a, syn_b, *s["priors"], max_iter=co.ASYM_MAX_ITER)
    assert 5 <= (~ca).sum() <= co.ASYM_B - 5 and 5 <= (~cb).sum() <= co.ASYM_B - 5


@pytest.mark.parametrize("name", ["[[72, 12, 6]]", "hgp"])
def test_code_identities(name):
    if name == "hgp":
        Hx, Hz, Lx, Lz = co.hgp_steane()
    else:
        c = codes.load_code(name)
        Hx, Hz, Lx, Lz = (np.asarray(a, np.uint8) for a in (c.Hx, c.Hz, c.Lx, c.Lz))
    i64 = lambda a: a.astype(np.int64)
    assert not (i64(Hx) @ i64(Hz).T % 2).any()
    assert not (i64(Hx) @ i64(Lz).T % 2).any() and not (i64(Hz) @ i64(Lx).T % 2).any()


@pytest.mark.parametrize("osd", [None, 0])
def test_equal_priors_decode_the_sectors_independently(osd):
    """With prior_b1 == prior_b0 the statement is two independent classifications on the same errors."""
    c = codes.load_code("[[72, 12, 6]]")
    Hx, Hz, Lx, Lz = (np.asarray(a, np.uint8) for a in (c.Hx, c.Hz, c.Lx, c.Lz))
    p = 0.09
    ea, eb = co.sample_pauli(c.n, p / 3, p / 3, p / 3, 7, 0, 120)
    pa, _, _ = css.pauli_priors(p / 3, p / 3, p / 3, c.n)
    pb = css.marginal_prior_b(p / 3, p / 3, p / 3, c.n)
    got = co.counters(Hx, Hz, Lx, Lz, c.distance, ea, eb, pa, pb, pb, max_iter=20, osd=osd)

    def alone(H, L, e, prior):
        s = (e.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
        hard, conv, iters, llr = oracle.decode_batch(H, s, prior, 20)
        if osd is not None:
            hard = hard.copy()
            for i in np.flatnonzero(~conv):
                hard[i] = oracle.osd0(H, s[i], llr[i], hard[i])
        cnt = oracle.classify_trials(H, L, c.distance, e, s, hard, conv, iters)
        cnt[10] = int(((hard.astype(np.int64) @ H.T.astype(np.int64) % 2) != s).any(axis=1).sum())
        return cnt
    assert np.array_equal(got[0], alone(Hx, Lx, ea, pa)) and np.array_equal(got[1], alone(Hz, Lz, eb, pb))
    assert got[0][6] >= 3 and got[0][6] < 120       # some converge, some do not
    assert got[2][0] == 120 and got[2][1] >= max(got[0][1], got[1][1]) and got[2][6] >= max(got[0][6], got[1][6])
    assert got[2][1] <= got[0][1] + got[1][1]
    # a conditioned second stage is another computation
    _, b0, b1 = css.pauli_priors(p / 3, p / 3, p / 3, c.n)
    other = co.counters(Hx, Hz, Lx, Lz, c.distance, ea, eb, pa, b0, b1, max_iter=20, osd=osd)
    assert np.array_equal(other[0], got[0]) and not np.array_equal(other[1], got[1])
