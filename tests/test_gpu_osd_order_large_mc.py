"""GPU: QBP_FLAG_OSD_LARGE through the Monte-Carlo and shot pipelines on the 432 x 1296 phenomenological matrix
([[72,12,6]] over 12 rounds, p = q = 0.03, BP(20), OSD-CS-7): every entry point equals the composition of its parts."""
import functools

import numpy as np
import pytest

import spectrum_oracle
from oracle import oracle
from qldpc_amd import _lib, bp, dem, mc

pytestmark = pytest.mark.gpu

P, ITERS = 0.03, 20
FL = _lib.osd_flags("cs", 7, large=True)
FL_CLEAR = _lib.osd_flags("cs", 7)


@functools.lru_cache(maxsize=None)
def _setup():
    Hs, L, probs = dem.phenomenological("[[72, 12, 6]]", 12, P)
    row_ptr, col_idx, m, n = bp.csr_from_H(Hs)
    dec = _lib.Decoder(row_ptr, col_idx, m, n, bp.DEVICE)
    return Hs.toarray().astype(np.int64), L, probs, mc.dem_prior(probs), dec


def _compose(errors, max_iter=ITERS):
    """decode_batch, then osd(..., large=True) on the failures, then the oracle's classification."""
    H, L, probs, prior, dec = _setup()
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, llr = dec.decode(syn, prior, max_iter)
    det = hard.copy()
    f = np.flatnonzero(~conv)
    if len(f):
        det[f] = dec.osd(syn[f], llr[f], hard[f], method="cs", order=7, large=True)
    cnt = oracle.classify_trials(H, L, 0, errors, syn, det, conv, iters)
    cnt[10] = int(((det[f].astype(np.int64) @ H.T % 2) != syn[f]).any(1).sum())
    return cnt, det, conv, iters


def test_mc_run_errors_equals_the_composition():
    H, L, probs, prior, dec = _setup()
    errors = (np.random.default_rng(5).random((96, H.shape[1])) < P).astype(np.uint8)
    want, _, _, _ = _compose(errors)
    got = dec.mc_run_errors(L, 0, errors, prior, max_iter=ITERS, flags=FL)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[6] == 54
    assert np.array_equal(got, want)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_errors(L, 0, errors, prior, max_iter=ITERS, flags=FL_CLEAR)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_mc_run_probs_budgets_and_spectrum():
    H, L, probs, prior, dec = _setup()
    T = 2000
    errors = dec.mc_sample_errors_probs(probs, 0, T, seed=3)
    want = dec.mc_run_errors(L, 0, errors, prior, max_iter=ITERS, flags=FL)
    got = dec.mc_run_probs(L, 0, probs, prior, 0, T, seed=3, max_iter=ITERS, flags=FL)
    assert got[6] > 0 and np.array_equal(got, want)
    rows = dec.mc_run_budgets(L, 0, probs, prior, (5, ITERS), 0, T, seed=3, flags=FL)
    assert np.array_equal(rows[1], want)
    assert np.array_equal(rows[0], dec.mc_run_probs(L, 0, probs, prior, 0, T, seed=3, max_iter=5, flags=FL))
    cnt, spectrum, hist = dec.mc_run_spectrum(L, 0, probs, prior, 0, T, seed=3, max_iter=ITERS, flags=FL)
    assert np.array_equal(cnt, want)
    _, det, conv, iters = _compose(errors)
    res = det ^ errors
    w = res.sum(1)
    logical = ((res.astype(np.int64) @ L.T.astype(np.int64)) % 2).any(1)
    table = np.zeros_like(spectrum)
    for wi, lg, fd in zip(w, logical, conv):
        if wi:
            table[(0 if fd else 1) + (2 if lg else 0), wi] += 1
    assert np.array_equal(spectrum, table)
    assert np.array_equal(hist, np.bincount(np.where(conv, iters, ITERS), minlength=ITERS + 1))
    spectrum_oracle.check_identities(cnt, spectrum, hist, ITERS, True)
    for call in (lambda: dec.mc_run_probs(L, 0, probs, prior, 0, T, seed=3, max_iter=ITERS, flags=FL_CLEAR),
                 lambda: dec.mc_run_budgets(L, 0, probs, prior, (5, ITERS), 0, T, seed=3, flags=FL_CLEAR),
                 lambda: dec.mc_run_spectrum(L, 0, probs, prior, 0, T, seed=3, max_iter=ITERS, flags=FL_CLEAR)):
        with pytest.raises(_lib.QbpError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED


def test_spectrum_tables_equal_the_cpu_oracle():
    """A reference independent of the library: tests/spectrum_oracle.py on 16 of the 96 error patterns (the oracle's
    order-w OSD costs 0.4 s per failure here)."""
    H, L, probs, prior, dec = _setup()
    errors = (np.random.default_rng(5).random((96, H.shape[1])) < P).astype(np.uint8)[:16]
    want = spectrum_oracle.spectrum_of_errors(H, L, 0, errors, prior, ITERS, osd=True, osd_method="cs", osd_order=7)
    assert want[0][6] >= 4, want[0]
    got = dec.mc_run_errors_spectrum(L, 0, errors, prior, max_iter=ITERS, flags=FL)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
    spectrum_oracle.check_identities(*got, ITERS, True)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_errors_spectrum(L, 0, errors, prior, max_iter=ITERS, flags=FL_CLEAR)
    assert e.value.code == _lib.E_UNSUPPORTED


def _masks(bits):
    return (bits.astype(np.uint64) << np.arange(bits.shape[1], dtype=np.uint64)).sum(1).astype(np.uint64)


def test_decode_shots_equals_the_composition():
    """Predictions, converged flags and every counter (0, 1, 6, 7, 8, 10; the others stay 0) against the composition;
    the recorded observables are those of the errors, with every fifth shot's flipped so that [1] and [8] also count
    shots the decoder got right."""
    H, L, probs, prior, dec = _setup()
    errors = (np.random.default_rng(5).random((96, H.shape[1])) < P).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    _, det, conv, iters = _compose(errors)
    Li = L.astype(np.int64)
    want = _masks((det.astype(np.int64) @ Li.T) % 2)
    actual = _masks((errors.astype(np.int64) @ Li.T) % 2)
    actual[::5] ^= np.uint64(1)
    det_bits = np.packbits(syn, axis=1, bitorder="little")
    cnt, pred, got_conv = dec.decode_shots(L, det_bits, prior, actual=actual, max_iter=ITERS, flags=FL)
    assert np.array_equal(pred, want)
    assert np.array_equal(got_conv, conv)
    wrong = want != actual
    f = np.flatnonzero(~conv)
    exp = np.zeros(_lib.NUM_COUNTERS, np.int64)
    exp[0], exp[6], exp[7] = len(syn), len(f), int(iters.sum())
    exp[1], exp[8] = int(wrong.sum()), int((wrong & ~conv).sum())
    exp[10] = int(((det[f].astype(np.int64) @ H.T % 2) != syn[f]).any(1).sum())
    assert exp[6] == 54 and exp[8] > 0 and exp[1] > exp[8]
    assert np.array_equal(cnt, exp), (cnt, exp)
    with pytest.raises(_lib.QbpError) as e:
        dec.decode_shots(L, det_bits, prior, actual=actual, max_iter=ITERS, flags=FL_CLEAR)
    assert e.value.code == _lib.E_UNSUPPORTED
