"""GPU: BP with a prior per record (qbp_decode_batch_cond, bp_cond_kernel) against qbp_decode_batch and the CPU
oracle, record by record with the record's own prior vector -- bit for bit (NaN equal to NaN), outputs in poisoned
buffers."""
import numpy as np
import pytest

import css_oracle as co
import geometry_util as gu
import lsd_util
from qldpc_amd import _lib, bp, codes

pytestmark = pytest.mark.gpu

B = 48
ALPHA, CLIP = 0.8, 20.0
VARIANTS = {"sp": _lib.SUM_PRODUCT, "ms": _lib.MIN_SUM}
NAMES = ("steane", "72z", "74", "rand37", "longrow", "hgpz", "144z")


def matrix(name):
    if name == "72z":
        return np.asarray(codes.load_code("[[72, 12, 6]]").Hz, np.uint8)
    if name == "144z":
        return np.asarray(codes.load_code("[[144, 12, 12]]").Hz, np.uint8)
    if name == "hgpz":
        return co.hgp_steane()[1]
    if name == "longrow":       # 6 x 30: a check of weight 12 and one of weight 9 beside short ones, columns of weight 1 .. 3
        rng = np.random.default_rng(12)
        H = np.zeros((6, 30), np.uint8)
        for r, w in enumerate((12, 9, 6, 5, 4, 3)):
            H[r, rng.choice(30, w, replace=False)] = 1
        H[rng.integers(0, 6, 30), np.arange(30)] = 1
        assert H.sum(1).max() > 8
        return H
    return lsd_util.matrix(name)


_CASE = {}


def case(name):
    """Decoder, 48 syndromes from errors of mixed rates (records that converge at once, later and never), a non-uniform
    prior0, the depolarizing prior1 = 0 and a prior1 with a +inf and a negative entry, selectors of density 0.05 / 0.5."""
    if name not in _CASE:
        H = matrix(name)
        m, n = H.shape
        rng = np.random.default_rng(sum(map(ord, name)))
        rates = np.linspace(0.0, 0.16, B)[:, None]
        errors = (rng.random((B, n)) < rates).astype(np.uint8)
        syn = gu.syndromes_of(H, errors)
        prior0 = np.log((1 - 0.04) / 0.04) * rng.uniform(0.8, 1.25, n)
        wild = rng.uniform(0.2, 1.0, n)
        wild[rng.integers(0, n)] = np.inf
        wild[(np.flatnonzero(np.isinf(wild))[0] + 1) % n] = -0.7
        sels = {d: ((rng.random((B, n)) < d) * rng.choice([1, 3, 255], (B, n))).astype(np.uint8) for d in (0.05, 0.5)}
        _CASE[name] = dict(H=H, m=m, n=n, dec=_lib.Decoder(*bp.csr_from_H(H), bp.DEVICE), syn=syn, prior0=prior0,
                           prior1={"zero": np.zeros(n), "wild": wild}, sels=sels)
    return _CASE[name]


def launch(dec, syn_t, sel_t, p0_t, p1_t, rows, out, max_iter, variant, nulls=(), stream=None, flags=0):
    out.poison()
    dec.decode_cond_device(syn_t.data_ptr(), sel_t.data_ptr(), p0_t.data_ptr(), p1_t.data_ptr(), rows, max_iter, variant,
                           ALPHA, CLIP, flags, out.ptr("hard", nulls), out.ptr("converged", nulls),
                           out.ptr("iters", nulls), out.ptr("llr", nulls), stream if stream is not None else gu.stream_ptr())


def cond(c, sel, prior1, max_iter, variant, what, nulls=()):
    out = gu.Outputs(B, c["n"])
    launch(c["dec"], gu.to_device(c["syn"]), gu.to_device(sel), gu.to_device(c["prior0"]), gu.to_device(prior1), B, out,
           max_iter, variant, nulls)
    return out.fetch(B, max_iter, what, nulls)


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", NAMES)
def test_constant_selector_is_decode_batch(name, variant, max_iter):
    """sel == 0 is qbp_decode_batch on prior0, sel == 1 on prior1; only bit 0 of a selector byte counts."""
    c = case(name)
    v = VARIANTS[variant]
    for key, prior1 in c["prior1"].items():
        for fill, prior in ((0, c["prior0"]), (1, prior1), (2, c["prior0"]), (0xFD, prior1)):
            what = f"{name} {variant} {max_iter} prior1={key} sel={fill}"
            got = cond(c, np.full((B, c["n"]), fill, np.uint8), prior1, max_iter, v, what)
            want = c["dec"].decode(c["syn"], prior, max_iter, v, ALPHA, 1.0, CLIP)
            gu.assert_same(got, want, what)


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", NAMES)
def test_random_selector_record_by_record(name, variant, max_iter):
    """Record b is qbp_decode_batch on syndromes[b : b + 1] with np.where(sel[b] & 1, prior1, prior0), and the oracle's
    decode of the same."""
    c = case(name)
    v = VARIANTS[variant]
    seen = set()
    for key, prior1 in c["prior1"].items():
        for density, sel in c["sels"].items():
            what = f"{name} {variant} {max_iter} prior1={key} density={density}"
            got = cond(c, sel, prior1, max_iter, v, what)
            pr = co.conditional_prior(sel, c["prior0"], prior1)
            rows = [c["dec"].decode(c["syn"][b:b + 1], pr[b], max_iter, v, ALPHA, 1.0, CLIP) for b in range(B)]
            want = tuple(np.concatenate([r[i] for r in rows]) for i in range(4))
            gu.assert_same(got, want, what + " (qbp_decode_batch)")
            gu.assert_same(got, co.decode_cond(c["H"], c["syn"], sel, c["prior0"], prior1, max_iter, v, ALPHA, CLIP),
                           what + " (oracle)")
            if key == "zero":
                seen |= {("never" if not cv else "first" if it == 0 else "later") for cv, it in zip(got[1], got[2])}
    if max_iter == 50 and name in ("72z", "144z", "hgpz"):
        assert seen == {"never", "first", "later"}, seen


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_many_edges_per_thread_with_infinite_priors(variant):
    """1000 x 3000 with about 6000 messages: a dozen edges per thread of the workgroup, so the wavefronts are far apart
    when the record's first check step begins.  One prior1 entry in twenty is +inf: min-sum has to send NaN on exactly
    those edges, as qbp_decode_batch and the oracle do."""
    rng = np.random.default_rng(1000)
    m, n, rows = 1000, 3000, 12
    H = np.zeros((m, n), np.uint8)
    H[np.repeat(np.arange(m), 6), np.concatenate([rng.permutation(n), rng.permutation(n)])] = 1
    assert H.sum(0).min() >= 1 and H.sum() > 11 * 512
    dec = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    syn = gu.syndromes_of(H, (rng.random((rows, n)) < 0.01).astype(np.uint8))
    prior0 = np.log((1 - 0.02) / 0.02) * rng.uniform(0.8, 1.25, n)
    prior1 = np.where(rng.random(n) < 0.05, np.inf, rng.uniform(0.0, 1.0, n))
    sel = (rng.random((rows, n)) < 0.5).astype(np.uint8)
    v = VARIANTS[variant]
    out = gu.Outputs(rows, n)
    launch(dec, gu.to_device(syn), gu.to_device(sel), gu.to_device(prior0), gu.to_device(prior1), rows, out, 4, v)
    got = out.fetch(rows, 4, "1000 x 3000")
    assert dec.info("threads") <= 512
    if variant == "ms":
        assert np.isnan(got[3]).any() and not np.isnan(got[3]).all()
    pr = co.conditional_prior(sel, prior0, prior1)
    parts = [dec.decode(syn[b:b + 1], pr[b], 4, v, ALPHA, 1.0, CLIP) for b in range(rows)]
    gu.assert_same(got, tuple(np.concatenate([r[i] for r in parts]) for i in range(4)), "1000 x 3000 (qbp_decode_batch)")
    gu.assert_same(got, co.decode_cond(H, syn, sel, prior0, prior1, 4, v, ALPHA, CLIP), "1000 x 3000 (oracle)")


def test_null_outputs_stay_untouched():
    c = case("72z")
    sel = c["sels"][0.5]
    full = cond(c, sel, c["prior1"]["zero"], 50, _lib.SUM_PRODUCT, "all outputs")
    for nulls in (("llr",), ("hard", "iters"), ("hard", "converged", "iters", "llr")):
        got = cond(c, sel, c["prior1"]["zero"], 50, _lib.SUM_PRODUCT, f"nulls {nulls}", nulls)
        gu.assert_same(got, full, f"nulls {nulls}")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_independence_of_batch_grid_stream_and_history(variant):
    """A record's outputs do not depend on the batch it is in, the grid, the stream, or an earlier call with another
    selector on the same handle."""
    c = case("72z")
    v = VARIANTS[variant]
    dec, n = c["dec"], c["n"]
    cus = dec.info("num_cu")
    big = 8 * cus + 37
    rng = np.random.default_rng(3)
    pick = rng.integers(0, B, big)
    syn, sel = c["syn"][pick], c["sels"][0.5][rng.integers(0, B, big)]
    prior1 = c["prior1"]["wild"]
    syn_t, sel_t, p0_t, p1_t = (gu.to_device(a) for a in (syn, sel, c["prior0"], prior1))
    out = gu.Outputs(big, n)
    launch(dec, syn_t, sel_t, p0_t, p1_t, big, out, 50, v)
    ref = out.fetch(big, 50, "the whole batch")
    # the reference itself: 48 of its records against qbp_decode_batch with the record's prior
    pr = co.conditional_prior(sel, c["prior0"], prior1)
    for b in np.linspace(0, big - 1, 48).astype(int):
        gu.assert_same(tuple(x[b:b + 1] for x in ref), dec.decode(syn[b:b + 1], pr[b], 50, v, ALPHA, 1.0, CLIP), f"record {b}")
    other = gu.to_device(np.ascontiguousarray(1 - (sel & 1)))
    for rows in (1, cus - 1, big):
        launch(dec, syn_t, other, p0_t, p1_t, rows, out, 50, v)      # (another selector first)
        out.fetch(rows, 50, "the other selector")
        launch(dec, syn_t, sel_t, p0_t, p1_t, rows, out, 50, v)
        gu.assert_same(out.fetch(rows, 50, f"B = {rows}"), tuple(x[:rows] for x in ref), f"B = {rows}")
    with gu.options(dec, blocks=1):
        launch(dec, syn_t, sel_t, p0_t, p1_t, big, out, 50, v)
        gu.assert_same(out.fetch(big, 50, "one workgroup per CU"), ref, "one workgroup per CU")
        assert dec.info("grid") == cus
    t = gu.torch()
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        launch(dec, syn_t, sel_t, p0_t, p1_t, big, out, 50, v, stream=side.cuda_stream)
    side.synchronize()
    gu.assert_same(out.fetch(big, 50, "another stream"), ref, "another stream")


def _host_call(dec, syn, sel, p0, p1, max_iter=5, variant=_lib.SUM_PRODUCT, flags=0, rows=None):
    """The host entry with poisoned outputs -> (return code, outputs untouched)."""
    rows = B if rows is None else rows
    n = dec.n
    hard = np.full((max(rows, 1), n), 0xEE, np.uint8)
    conv = np.full(max(rows, 1), 0xEE, np.uint8)
    iters = np.full(max(rows, 1), -7, np.int32)
    llr = np.full((max(rows, 1), n), gu.LLR_POISON)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().qbp_decode_batch_cond(dec._h, ptr(syn), ptr(sel), ptr(p0), ptr(p1), rows, max_iter, variant, ALPHA, CLIP,
                                           flags, hard.ctypes.data, conv.ctypes.data, iters.ctypes.data, llr.ctypes.data)
    untouched = bool((hard == 0xEE).all() and (conv == 0xEE).all() and (iters == -7).all() and (llr == gu.LLR_POISON).all())
    return rc, untouched


def test_refusals_leave_the_outputs_untouched():
    c = case("steane")
    dec, syn, sel, p0, p1 = c["dec"], c["syn"], c["sels"][0.5], c["prior0"], c["prior1"]["zero"]
    assert _host_call(dec, syn, sel, p0, p1) == (0, False)
    assert _host_call(dec, syn, sel, p0, p1, rows=0) == (0, True)
    nan = p0.copy()
    nan[3] = np.nan
    invalid = [dict(syn=None), dict(sel=None), dict(p0=None), dict(p1=None), dict(p0=nan), dict(p1=nan),
               dict(max_iter=0), dict(variant=7), dict(flags=_lib.FLAG_OSD0), dict(flags=1 << 14), dict(rows=-1)]
    for kw in invalid:
        args = dict(syn=syn, sel=sel, p0=p0, p1=p1)
        args.update(kw)
        assert _host_call(dec, **args) == (_lib.E_INVALID, True), kw
    inf = p0.copy()
    inf[2] = -np.inf
    assert _host_call(dec, syn, sel, inf, p1) == (0, False)          # +-inf are legal
    unsupported = [dict(variant=_lib.DAMPED_SP), dict(flags=_lib.FLAG_PAIRWISE_COLSUM), dict(flags=_lib.FLAG_DENSE_F_COLSUM),
                   dict(flags=_lib.FLAG_LAYERED), dict(flags=_lib.FLAG_FAST_MATH), dict(flags=_lib.FLAG_GD)]
    for kw in unsupported:
        assert _host_call(dec, syn, sel, p0, p1, **kw) == (_lib.E_UNSUPPORTED, True), kw
    with pytest.raises(_lib.QbpError) as e:
        dec.decode_cond(syn, sel, p0, p1, variant=_lib.DAMPED_SP)
    assert e.value.code == _lib.E_UNSUPPORTED
    # the device entry refuses the same before any GPU work (null pointers: nothing is read)
    rc = _lib.load().qbp_decode_batch_cond_device(dec._h, None, None, None, None, 4, 5, 0, ALPHA, CLIP, 0, None, None, None,
                                                  None, None)
    assert rc == _lib.E_INVALID


def test_a_matrix_beyond_the_lds_is_unsupported():
    """2592 x 7776 (the space-time size of the record-kernel tests' refusals): 46656 messages do not fit 160 KiB."""
    rng = np.random.default_rng(1)
    m, n = 2592, 7776
    row_ptr = np.arange(0, m * 3 + 1, 3, dtype=np.int32)
    col_idx = np.sort(rng.permutation(n)[:m * 3].reshape(m, 3), axis=1).astype(np.int32).ravel()
    dec = _lib.Decoder(row_ptr, col_idx, m, n, bp.DEVICE)
    syn = np.zeros((2, m), np.uint8)
    sel = np.zeros((2, n), np.uint8)
    p = np.full(n, 3.0)
    for v in VARIANTS.values():
        assert _host_call(dec, syn, sel, p, p, variant=v) == (_lib.E_UNSUPPORTED, True)
    assert "160 KiB" in _lib.load().qbp_last_error().decode()
