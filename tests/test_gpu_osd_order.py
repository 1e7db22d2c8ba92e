"""GPU: order-w OSD (qbp_osd_batch, osd_order_kernel) bit for bit against the numpy statement of the spec
(tests/osd_order_oracle.py), through the batch entry, the device entry and the Monte-Carlo pipeline."""
import os

import numpy as np
import pytest

import osd_order_oracle as ordo
from oracle import oracle
from qldpc_amd import _lib, bp, codes, mc, osd
from test_oracle_osd import TAGS, load_osd

pytestmark = pytest.mark.gpu

CODES = ("[[72, 12, 6]]", "[[90, 8, 10]]", "[[108, 8, 10]]", "[[144, 12, 12]]", "[[288, 12, 18]]")
CONFIGS = [("cs", 1), ("cs", 7), ("cs", 20), ("cs", 64), ("e", 1), ("e", 4), ("e", 8), ("e", 12)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fresh_decoder(H):
    row_ptr, col_idx, m, n = bp.csr_from_H(H)
    return _lib.Decoder(row_ptr, col_idx, m, n, bp.DEVICE)


def _raw_osd(dec, flags, syn, llr, hard):
    """qbp_osd_batch with raw flags: (return code, solutions)."""
    syn = np.ascontiguousarray(syn, np.uint8)
    llr = np.ascontiguousarray(llr, np.float64)
    hard = np.ascontiguousarray(hard, np.uint8)
    out = np.zeros_like(hard)
    rc = _lib.load().qbp_osd_batch(dec._h, flags, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data, len(syn),
                                   out.ctypes.data)
    return rc, out


def _oracle_batch(H, syn, llr, hard, method, order, reds=None):
    reds = reds or [ordo.reduce(H, s, l, h) for s, l, h in zip(syn, llr, hard)]
    return np.stack([ordo.osd_order(H, s, l, h, order, method, red=r)
                     for s, l, h, r in zip(syn, llr, hard, reds)]), reds


def _bp_failures(code, ps=(0.05, 0.08), per_p=120, seed=11):
    dec = bp.decoder_for(code.Hx)
    rng = np.random.default_rng(seed)
    out = []
    for p in ps:
        err = (rng.random((4000, code.n)) < p).astype(np.uint8)
        syn = (err @ code.Hx.T % 2).astype(np.uint8)
        hard, conv, iters, llr = dec.decode(syn, mc.prior_of(p, code.n), 50)
        f = np.flatnonzero(~conv)[:per_p]
        out.append((syn[f], llr[f], hard[f]))
    return tuple(np.concatenate(x) for x in zip(*out))


@pytest.mark.parametrize("tag", TAGS)
def test_zero_flags_is_osd0(tag):
    c = load_osd(tag)
    H = c["H"].astype(np.int64)
    dec = bp.decoder_for(H)
    for flags in (0, _lib.FLAG_OSD0):
        rc, got = _raw_osd(dec, flags, c["syndromes"], c["llr"], c["hard"])
        assert rc == 0 and np.array_equal(got, c["solution"])
    assert np.array_equal(dec.osd(c["syndromes"], c["llr"], c["hard"], order=0), c["solution"])


@pytest.mark.parametrize("name", CODES)
def test_device_equals_oracle_on_bp_failures(name):
    code = codes.load_code(name)
    H = code.Hx.astype(np.int64)
    syn, llr, hard = _bp_failures(code)
    assert len(syn) >= 150, len(syn)
    dec = bp.decoder_for(code.Hx)
    reds = None
    searched = 0
    for method, w in CONFIGS:
        got = dec.osd(syn, llr, hard, method=method, order=w)
        want, reds = _oracle_batch(H, syn, llr, hard, method, w, reds)
        assert np.array_equal((got.astype(np.int64) @ H.T) % 2, syn), (method, w)
        bad = np.flatnonzero((got != want).any(1))
        assert len(bad) == 0, (method, w, bad[:10])
        searched += int((want != np.stack([r.x0 for r in reds])).any(1).sum())
    assert searched > 0                   # the search did change some solutions
    one = osd.performOSD_order(H, syn[0], llr[0], hard[0], 7)
    assert one.dtype == np.int64 and np.array_equal(one, ordo.osd_order(H, syn[0], llr[0], hard[0], 7, red=reds[0]))
    assert np.array_equal(osd.performOSD_order_batch(H, syn[:5], llr[:5], hard[:5], 4, method="e"),
                          _oracle_batch(H, syn[:5], llr[:5], hard[:5], "e", 4, reds[:5])[0])


def _stress_llrs(llr, rng):
    B, n = llr.shape
    sign = np.where(rng.random((B, n)) < 0.5, -1.0, 1.0)
    out = {"equal": np.ones((B, n)),
           "three": rng.choice([0.5, 1.0, 2.0], size=(B, n)) * sign,
           "zeros": np.where(rng.random((B, n)) < 0.3, 0.0, llr) * sign}     # +-0.0 included
    special = llr.copy()
    pick = rng.random((B, n))
    special[pick < 0.02] = np.nan
    special[(pick >= 0.02) & (pick < 0.05)] = np.inf
    special[(pick >= 0.05) & (pick < 0.08)] = -np.inf
    out["nan_inf"] = special
    fewnan = llr.copy()
    fewnan[pick < 0.005] = np.nan
    out["few_nan"] = fewnan
    return out


@pytest.mark.parametrize("name", ("steane", "[[72, 12, 6]]", "[[144, 12, 12]]"))
def test_ties_and_special_values(name):
    code = codes.load_code(name)
    H = code.Hx.astype(np.int64)
    if name == "steane":
        c = load_osd("steane")
        syn, llr, hard = c["syndromes"], c["llr"], c["hard"]
    else:
        syn, llr, hard = _bp_failures(code, ps=(0.06,), per_p=60, seed=5)
    dec = bp.decoder_for(code.Hx)
    rng = np.random.default_rng(3)
    for kind, L in _stress_llrs(llr, rng).items():
        reds = None
        for method, w in (("cs", 7), ("cs", 64), ("e", 4), ("e", 12)):
            got = dec.osd(syn, L, hard, method=method, order=w)
            want, reds = _oracle_batch(H, syn, L, hard, method, w, reds)
            assert np.array_equal(got, want), (kind, method, w, np.flatnonzero((got != want).any(1))[:10])
            assert np.array_equal((got.astype(np.int64) @ H.T) % 2, syn)


@pytest.mark.parametrize("tag", ("72", "144", "288"))
def test_inconsistent_syndromes_get_osd0(tag):
    d = np.load(os.path.join(GOLDEN, "osd_inconsistent.npz"))
    H = d[f"{tag}/H"].astype(np.int64)
    syn, llr, hard, want = (d[f"{tag}/{k}"] for k in ("syndromes", "llr", "hard", "solution"))
    dec = bp.decoder_for(H)
    for method, w in (("cs", 7), ("e", 8)):
        assert np.array_equal(dec.osd(syn, llr, hard, method=method, order=w), want)
    # mixed with syndromes that come from errors
    c = load_osd(tag)
    ms = np.concatenate([syn[:4], c["syndromes"][:6]])
    ml = np.concatenate([llr[:4], c["llr"][:6]])
    mh = np.concatenate([hard[:4], c["hard"][:6]])
    got = dec.osd(ms, ml, mh, method="cs", order=7)
    assert np.array_equal(got[:4], want[:4])
    assert np.array_equal(got[4:], ordo.osd_order_batch(H, ms[4:], ml[4:], mh[4:], 7, "cs"))


_DECODED = {}


def _oracle_pipeline(code, errors, prior, method, order):
    H = code.Hx.astype(np.int64)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    key = (code.n, errors.tobytes(), prior.tobytes())
    if key not in _DECODED:
        _DECODED[key] = oracle.decode_batch(H, syn, prior, 50, threads=16)
    hard, conv, iters, llr = _DECODED[key]
    det = hard.copy()
    f = np.flatnonzero(~conv)
    for i in f:
        det[i] = ordo.osd_order(H, syn[i], llr[i], hard[i], order, method)
    cnt = oracle.classify_trials(H, code.Lx, code.distance, errors, syn, det, conv, iters)
    cnt[10] = sum(not np.array_equal((det[i].astype(np.int64) @ H.T) % 2, syn[i]) for i in f)
    return cnt


@pytest.mark.parametrize("method,order", [("cs", 7), ("e", 8)])
def test_monte_carlo_counters_equal_the_oracle_pipeline(method, order):
    code = codes.load_code("[[144, 12, 12]]")
    p, T, seed = 0.05, 20000, 9
    prior = mc.prior_of(p, code.n)
    errors = oracle.mc_errors(code.n, p, 1, seed, 0, T)
    want = _oracle_pipeline(code, errors, prior, method, order)
    assert want[6] > 100 and want[10] == 0
    dec = bp.decoder_for(code.Hx)
    fl = _lib.osd_flags(method, order)
    got = dec.mc_run_errors(code.Lx, code.distance, errors, prior, max_iter=50, flags=fl)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert np.array_equal(got, want)
    got = dec.mc_run(code.Lx, code.distance, p, prior, 0, T, seed=seed, max_iter=50, flags=fl)
    assert np.array_equal(got, want)
    # OSD-0 alone keeps its meaning
    osd0 = dec.mc_run_errors(code.Lx, code.distance, errors, prior, max_iter=50, flags=_lib.FLAG_OSD0)
    assert np.array_equal(osd0, _oracle_pipeline(code, errors, prior, "cs", 0))


def test_invalid_flag_combinations():
    code = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(code.Hx)
    c = load_osd("72")
    args = (c["syndromes"][:2], c["llr"][:2], c["hard"][:2])
    O = lambda w: w << _lib.OSD_ORDER_SHIFT   # noqa: E731
    for flags in (_lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | O(3), O(3), _lib.FLAG_OSD_CS, _lib.FLAG_OSD_E | O(13),
                  _lib.FLAG_OSD_CS | O(65), _lib.FLAG_OSD_CS | O(3) | _lib.FLAG_FORCE_FULL):
        assert _raw_osd(dec, flags, *args)[0] == -1, hex(flags)
    assert _raw_osd(dec, _lib.FLAG_OSD_CS | O(64), *args)[0] == 0
    assert _raw_osd(dec, _lib.FLAG_OSD0 | _lib.FLAG_OSD_E | O(12), *args)[0] == 0
    prior = mc.prior_of(0.05, code.n)
    counters = np.zeros(_lib.NUM_COUNTERS, np.int64)
    lib = _lib.load()
    Lx = np.ascontiguousarray(code.Lx, np.uint8)
    for flags in (_lib.FLAG_OSD_CS | O(7), _lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | O(7),
                  _lib.FLAG_OSD0 | O(7), _lib.FLAG_OSD0 | _lib.FLAG_OSD_E | O(13)):
        rc = lib.qbp_mc_run(dec._h, Lx.ctypes.data, Lx.shape[0], code.distance, 0.05, 1, 0, 0, 100,
                            prior.ctypes.data, 50, 0, 1.0, 1.0, 20.0, flags, counters.ctypes.data)
        assert rc == -1, hex(flags)
    assert not counters.any()


def test_matrix_beyond_the_lds_limit():
    """Order > 0 needs the one-wavefront kernel: QBP_E_UNSUPPORTED on a matrix beyond it; order 0 still works."""
    from scipy.sparse import block_diag, csr_matrix
    H144 = codes.load_code("[[144, 12, 12]]").Hx
    mm, T = H144.shape[0], 12
    st = np.hstack([np.kron(np.eye(T, dtype=np.int64), H144),
                    (np.eye(mm * T, dtype=np.int64) + np.eye(mm * T, k=-mm, dtype=np.int64)) % 2])
    H = block_diag([csr_matrix(st), csr_matrix(st)]).toarray().astype(np.int64)      # 1728 x 5184
    dec = _fresh_decoder(csr_matrix(H))
    rng = np.random.default_rng(2)
    n = H.shape[1]
    err = (rng.random((6, n)) < 0.02).astype(np.uint8)
    syn = (err @ H.T % 2).astype(np.uint8)
    llr = rng.standard_normal((6, n)) * 3
    hard = (llr < 0).astype(np.uint8)
    for method, w in (("cs", 7), ("e", 4)):
        with pytest.raises(_lib.QbpError) as e:
            dec.osd(syn, llr, hard, method=method, order=w)
        assert e.value.code == _lib.E_UNSUPPORTED
    got = dec.osd(syn, llr, hard, order=0)
    assert np.array_equal(got, dec.osd0(syn, llr, hard))
    assert np.array_equal((got.astype(np.int64) @ H.T) % 2, syn)
    Lx = np.zeros((1, n), np.uint8)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run(Lx, 10, 0.01, mc.prior_of(0.01, n), 0, 64, flags=_lib.osd_flags("cs", 7))
    assert e.value.code == _lib.E_UNSUPPORTED


def test_device_entry_on_torch_buffers():
    import torch
    code = codes.load_code("[[288, 12, 18]]")
    syn, llr, hard = _bp_failures(code, ps=(0.08,), per_p=64, seed=4)
    dec = bp.decoder_for(code.Hx)
    dev = torch.device("cuda", bp.DEVICE)
    d_syn = torch.from_numpy(np.ascontiguousarray(syn)).to(dev)
    d_llr = torch.from_numpy(np.ascontiguousarray(llr)).to(dev)
    d_hard = torch.from_numpy(np.ascontiguousarray(hard)).to(dev)
    d_sol = torch.empty_like(d_hard)
    stream = torch.cuda.current_stream(dev)
    for method, w in (("cs", 7), ("e", 8)):
        dec.osd_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(syn), d_sol.data_ptr(),
                       method=method, order=w, stream=stream.cuda_stream)
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_sol.cpu().numpy(), dec.osd(syn, llr, hard, method=method, order=w))
