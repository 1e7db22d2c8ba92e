"""GPU: recorded shots to observable predictions (qbp_decode_shots) against its definition -- qbp_decode_batch, then
qbp_osd_batch on BP's failures, then Lx x mod 2 in numpy -- against the Monte-Carlo path on the same errors, and
against a fixture decoded by the reference's own functions (tests/golden/shots.npz).  Every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import golden_util
from oracle import oracle
from qldpc_amd import _lib, bp, codes, dem, mc, shots

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OSD_CS7 = _lib.osd_flags("cs", 7)
OSD_BITS = _lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | (0xff << _lib.OSD_ORDER_SHIFT)
CHECKED = (0, 1, 6, 7, 8, 10)          # the counters qbp_decode_shots adds to; all others stay 0


def names(cnt):
    return dict(zip(_lib.COUNTER_NAMES, np.asarray(cnt).tolist()))


def compose(dec, H, L, syn, actual, prior, flags, **kw):
    """The definition of include/qbp.h, shot by shot: (counters, predictions, converged)."""
    Hs = csr_matrix(H).astype(np.int64)
    hard, conv, iters, llr = dec.decode(syn, prior, flags=flags & ~OSD_BITS, **kw)
    x = hard.copy()
    cnt = np.zeros(12, np.int64)
    fails = np.flatnonzero(~conv)
    if (flags & _lib.FLAG_OSD0) and len(fails):
        if flags & (_lib.FLAG_OSD_CS | _lib.FLAG_OSD_E):
            method = "cs" if flags & _lib.FLAG_OSD_CS else "e"
            sol = dec.osd(syn[fails], llr[fails], hard[fails], method, (flags >> _lib.OSD_ORDER_SHIFT) & 0xff)
        else:
            sol = dec.osd0(syn[fails], llr[fails], hard[fails])
        x[fails] = sol
        cnt[10] = int(((Hs @ sol.T.astype(np.int64)).T % 2 != syn[fails]).any(axis=1).sum())
    pred = shots.masks_of((x.astype(np.int64) @ np.asarray(L, np.int64).T) % 2)
    cnt[0], cnt[6], cnt[7] = len(syn), len(fails), int(iters.sum())
    if actual is not None:
        wrong = pred != actual
        cnt[1], cnt[8] = int(wrong.sum()), int((wrong & ~conv).sum())
    return cnt, pred, conv


def draw(H, L, probs, T, seed):
    """T errors with a rate per column -> (syndromes [T, m], actual masks [T])."""
    rng = np.random.default_rng(seed)
    Hs = csr_matrix(H).astype(np.int64)
    e = (rng.random((T, Hs.shape[1])) < probs).astype(np.int64)
    syn = ((Hs @ e.T).T % 2).astype(np.uint8)
    return syn, shots.masks_of((e @ np.asarray(L, np.int64).T) % 2)


def check_parity(dec, H, L, syn, actual, prior, flags, tag, **kw):
    """decode_shots == the composition; where qbp_mc_run refuses the OSD flags (order w beyond the one-wavefront
    kernel), decode_shots refuses them the same way.  Returns the counters (None when refused)."""
    det = shots.pack_bits(syn)
    try:
        want = compose(dec, H, L, syn, actual, prior, flags, **kw)
    except _lib.QbpError as e:
        assert flags == OSD_CS7 and e.code == _lib.E_UNSUPPORTED
        with pytest.raises(_lib.QbpError) as e2:
            dec.decode_shots(L, det, prior, actual, flags=flags, **kw)
        assert e2.value.code == _lib.E_UNSUPPORTED
        return None
    cnt, pred, conv = dec.decode_shots(L, det, prior, actual, flags=flags, **kw)
    print(tag, hex(flags), names(cnt))
    assert np.array_equal(conv, want[2]), (tag, flags)
    assert np.array_equal(pred, want[1]), (tag, flags, np.flatnonzero(pred != want[1])[:8])
    assert np.array_equal(cnt, want[0]), (tag, flags, names(cnt), names(want[0]))
    return cnt


def synthetic_dem_text(seed=3):
    """The synthetic model of tests/test_gpu_dem.py: the phenomenological DEM of [[72,12,6]] over 4 rounds plus hyperedge
    mechanisms of weight 3-6 (some repeated, so that they merge; some flipping observables) and observable-only
    mechanisms -- rows beyond weight 8, columns up to weight 6, three empty columns: the general-H kernel."""
    rng = np.random.default_rng(seed)
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 4, 0.004, 0.008)
    H = H.tocsc()
    lines = []
    for v in range(H.shape[1]):
        dets = H.indices[H.indptr[v]:H.indptr[v + 1]]
        obs = np.flatnonzero(L[:, v])
        lines.append(f"error({float(probs[v])!r}) " + " ".join([f"D{d}" for d in dets] + [f"L{o}" for o in obs]))
    m = H.shape[0]
    hyper = []
    for _ in range(160):
        w = int(rng.integers(3, 7))
        base = int(rng.integers(0, m - 80))
        dets = sorted(set(int(x) for x in base + rng.choice(80, size=w, replace=False)))
        obs = [int(o) for o in np.flatnonzero(rng.random(12) < 0.08)]
        hyper.append((dets, obs))
    for i in range(240):
        dets, obs = hyper[i % 160] if i < 160 else hyper[int(rng.integers(0, 160))]
        p = float(rng.uniform(1e-4, 4e-3))
        toks = [f"D{d}" for d in dets]
        if len(toks) > 3:
            toks.insert(2, "^")
        lines.append(f"error({p!r}) " + " ".join(toks + [f"L{o}" for o in obs]))
    for o in (0, 5, 11, 5):
        lines.append(f"error(0.0005) L{o}")
    lines.append("error(0.01) D3 ^ D3")
    return "\n".join(lines) + "\n"


def parity_cases():
    """(id, H, L, probs, T, decoder keywords, kernel kind)"""
    st = codes.load_code("steane")
    yield "steane", st.Hx, np.ones((1, st.n), np.uint8), np.full(st.n, 0.1), 257, {}, 1
    c72 = codes.load_code("[[72, 12, 6]]")
    for T in (1, 63, 1001):
        yield f"72-T{T}", c72.Hx, c72.Lx, np.full(c72.n, 0.05), T, {}, 1
    c144 = codes.load_code("[[144, 12, 12]]")
    yield "144-sp", c144.Hx, c144.Lx, np.full(c144.n, 0.05), 400, {}, 1
    yield "144-minsum", c144.Hx, c144.Lx, np.full(c144.n, 0.05), 400, dict(variant=_lib.MIN_SUM, alpha=0.8, damping=0.7,
                                                                            clip_llr=25.0), 1
    yield ("st144",) + dem.phenomenological("[[144, 12, 12]]", 12, 0.004, 0.01) + (300, {}, 1)
    yield ("synthetic",) + dem.parse_dem(synthetic_dem_text()) + (500, {}, 2)
    rand = next(iter(golden_util.load("rand")))["H"]
    L64 = (np.random.default_rng(64).random((64, rand.shape[1])) < 0.5).astype(np.uint8)
    yield "rand-k64", rand, L64, np.full(rand.shape[1], 0.02), 300, {}, 2


@pytest.mark.parametrize("case", list(parity_cases()), ids=lambda c: c[0])
def test_composition_parity(case):
    tag, H, L, probs, T, kw, kind = case
    m, n = H.shape
    assert tag != "steane" or (m == 3 and L.shape[0] == 1)
    assert not tag.startswith("72") or (m + 7) // 8 == 5        # rows start at odd addresses
    dec = bp.decoder_for(H)
    syn, actual = draw(H, L, probs, T, seed=len(tag) + T)
    prior = mc.dem_prior(probs)
    ran = 0
    for flags in (0, _lib.FLAG_OSD0, OSD_CS7):
        cnt = check_parity(dec, H, L, syn, actual, prior, flags, tag, **kw)
        if cnt is not None:
            ran += 1
            assert dec.info("last_kernel") == kind
            assert cnt[0] == T
    assert ran >= 2
    if tag == "synthetic":
        Hd = np.asarray(csr_matrix(H).toarray())
        assert (Hd.sum(axis=0) == 0).sum() == 3 and Hd.sum(axis=1).max() > 8


def test_forced_iterations_and_fast_math():
    """FLAG_FORCE_FULL: outputs of the first converged iteration, as qbp_decode_batch; FLAG_FAST_MATH: its build."""
    c = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(c.Hx)
    probs = np.full(c.n, 0.05)
    syn, actual = draw(c.Hx, c.Lx, probs, 300, seed=5)
    for flags in (_lib.FLAG_FORCE_FULL, _lib.FLAG_FORCE_FULL | _lib.FLAG_OSD0, _lib.FLAG_FAST_MATH | _lib.FLAG_OSD0):
        check_parity(dec, c.Hx, c.Lx, syn, actual, mc.dem_prior(probs), flags, "144-forced", max_iter=20)


def test_wrap_around_and_split_calls():
    """Few slots, many shots: every slot decodes hundreds of shots one after the other; two calls add up."""
    c = codes.load_code("[[72, 12, 6]]")
    dec = _lib.Decoder(*bp.csr_from_H(c.Hx))
    dec.set_option(_lib.OPT_SLOTS_PER_BLOCK, 3)
    dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
    T = 20000
    probs = np.full(c.n, 0.01)
    syn, actual = draw(c.Hx, c.Lx, probs, T, seed=9)
    prior = mc.dem_prior(probs)
    det = shots.pack_bits(syn)
    for flags in (0, _lib.FLAG_OSD0):
        whole = check_parity(dec, c.Hx, c.Lx, syn, actual, prior, flags, "72-wrap")
        assert T > 8 * dec.info("grid") * 3
        cnt = np.zeros(12, np.int64)
        a = 7777
        _, p1, c1 = dec.decode_shots(c.Lx, det[:a], prior, actual[:a], flags=flags, counters=cnt)
        _, p2, c2 = dec.decode_shots(c.Lx, det[a:], prior, actual[a:], flags=flags, counters=cnt)
        _, pw, cw = dec.decode_shots(c.Lx, det, prior, actual, flags=flags)
        assert np.array_equal(np.concatenate([p1, p2]), pw) and np.array_equal(np.concatenate([c1, c2]), cw)
        assert np.array_equal(cnt, whole)
    dec.close()


@pytest.mark.parametrize("model", ["144", "st144"])
def test_against_monte_carlo_path(model):
    """The same errors through qbp_mc_run_errors (which forms H e and L (x ^ e) itself) and through decode_shots."""
    if model == "144":
        c = codes.load_code("[[144, 12, 12]]")
        H, L, probs = c.Hx, c.Lx, np.full(c.n, 0.05)
    else:
        H, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.01)
    dec = bp.decoder_for(H)
    prior = mc.dem_prior(probs)
    T = 1500
    e = dec.mc_sample_errors_probs(probs, 2 ** 33 + 1, T, seed=12).astype(np.int64)
    Hs = csr_matrix(H).astype(np.int64)
    det = shots.pack_bits((Hs @ e.T).T % 2)
    actual = shots.masks_of((e @ np.asarray(L, np.int64).T) % 2)
    for flags in (0, _lib.FLAG_OSD0):
        want = dec.mc_run_errors(L, 0, e.astype(np.uint8), prior, flags=flags)
        got, _, _ = dec.decode_shots(L, det, prior, actual, flags=flags)
        print(model, flags, names(got))
        assert [got[i] for i in CHECKED] == [want[i] for i in CHECKED], (names(got), names(want))
        assert not got[[2, 3, 4, 5, 9, 11]].any()
        assert got[6] > 0


def test_syndromes_outside_the_column_space():
    """Uniformly random syndromes: Hx of [[72,12,6]] has dependent rows, so most are no error's syndrome.  The OSD
    kernel lists them for the kernel that follows the reference's row swaps, which must predict them too."""
    c = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(c.Hx)
    rng = np.random.default_rng(41)
    T = 600
    syn = (rng.random((T, c.Hx.shape[0])) < 0.5).astype(np.uint8)
    actual = rng.integers(0, 1 << 12, T, dtype=np.uint64)
    prior = mc.prior_of(0.05, c.n)
    for flags in (_lib.FLAG_OSD0, OSD_CS7):
        cnt = check_parity(dec, c.Hx, c.Lx, syn, actual, prior, flags, "72-random-syndromes", max_iter=10)
        assert cnt[10] > T // 2 and cnt[6] >= cnt[10]


def test_actual_none():
    c = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(c.Hx)
    probs = np.full(c.n, 0.06)
    syn, actual = draw(c.Hx, c.Lx, probs, 700, seed=2)
    det = shots.pack_bits(syn)
    prior = mc.dem_prior(probs)
    for flags in (0, _lib.FLAG_OSD0):
        with_a = dec.decode_shots(c.Lx, det, prior, actual, flags=flags)
        without = dec.decode_shots(c.Lx, det, prior, None, flags=flags)
        assert with_a[0][1] > 0 and with_a[0][6] > 0
        assert np.array_equal(with_a[1], without[1]) and np.array_equal(with_a[2], without[2])
        assert without[0][1] == 0 and without[0][8] == 0
        assert [without[0][i] for i in (0, 6, 7, 10)] == [with_a[0][i] for i in (0, 6, 7, 10)]
        assert np.array_equal(without[0], compose(dec, c.Hx, c.Lx, syn, None, prior, flags)[0])


def test_invalid_arguments_leave_outputs_untouched():
    c = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(c.Hx)
    lib = _lib.load()
    n, T = c.n, 50
    Lx = np.ascontiguousarray(c.Lx, np.uint8)
    syn, actual = draw(c.Hx, c.Lx, np.full(n, 0.05), T, seed=1)
    det = shots.pack_bits(syn)
    prior = mc.prior_of(0.05, n)
    nan_prior = prior.copy()
    nan_prior[n // 3] = np.nan
    big_L = np.zeros((65, n), np.uint8)

    def call(Lp=Lx.ctypes.data, k=Lx.shape[0], dp=det.ctypes.data, t=T, pp=prior.ctypes.data, max_iter=50, variant=0,
             flags=0, counters=True):
        pred = np.full(T, 0xABCD, np.uint64)
        conv = np.full(T, 7, np.uint8)
        cnt = np.arange(12, dtype=np.int64) + 3
        rc = lib.qbp_decode_shots(dec._h, Lp, k, dp, actual.ctypes.data, t, pp, max_iter, variant, 1.0, 1.0, 20.0, flags,
                                  pred.ctypes.data, conv.ctypes.data, cnt.ctypes.data if counters else None)
        assert (pred == 0xABCD).all() and (conv == 7).all() and np.array_equal(cnt, np.arange(12) + 3)
        return rc

    assert call(Lp=None) == -1
    assert call(dp=None) == -1
    assert call(pp=None) == -1
    assert call(counters=False) == -1
    assert call(k=0) == -1 and call(k=-1) == -1
    assert call(Lp=big_L.ctypes.data, k=65) == -1
    assert call(t=-1) == -1
    assert call(pp=nan_prior.ctypes.data) == -1
    # whatever qbp_mc_run refuses
    assert call(max_iter=0) == -1 and call(variant=3) == -1
    assert call(flags=_lib.FLAG_OSD_CS | (7 << 16)) == -1                     # a method bit without FLAG_OSD0
    assert call(flags=_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | (3 << 16)) == -1
    assert call(flags=_lib.FLAG_OSD0 | (3 << 16)) == -1                       # an order without a method
    assert call(flags=_lib.FLAG_OSD0 | _lib.FLAG_OSD_E | (13 << 16)) == -1
    assert call(flags=_lib.FLAG_OSD0, t=_lib.MC_OSD_MAX_TRIALS + 1) == -1     # the record rule (never dereferenced)
    assert call(t=0) == 0                                                     # a no-op that succeeds
    # the device entry refuses the same before it looks at a pointer
    for kw in (dict(d_det_bits=0), dict(d_prior=0), dict(d_counters=0), dict(T=-1)):
        args = dict(d_det_bits=8, d_actual=0, T=4, d_prior=8, d_predictions=0, d_converged=0, d_counters=8)
        args.update(kw)
        with pytest.raises(_lib.QbpError) as e:
            dec.decode_shots_device(Lx, **args)
        assert e.value.code == -1
    dec.decode_shots_device(Lx, 8, 0, 0, 8, 0, 0, 8)                          # T = 0
    # order-w OSD beyond the one-wavefront kernel stays unsupported
    H, L, probs = dem.phenomenological("[[288, 12, 18]]", 18, 0.004)
    big = bp.decoder_for(H)
    with pytest.raises(_lib.QbpError) as e:
        big.decode_shots(L, np.zeros((4, (H.shape[0] + 7) // 8), np.uint8), mc.dem_prior(probs), flags=OSD_CS7)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_fixture_pinned_by_the_reference():
    """tests/golden/shots.npz: shots decoded by the reference's performBeliefPropagationFast (maxIter 20) and
    performOSD on its failures (tests/golden/make_golden_shots.py).  Every shot, no exclusions."""
    d = np.load(os.path.join(GOLDEN, "shots.npz"))
    H, L, probs = dem.phenomenological(str(d["code"]), int(d["rounds"]), float(d["p"]), float(d["q"]))
    assert str(d["h_order"]) == "C"
    Hd = np.ascontiguousarray(H.toarray())
    to_device = {0: 0, oracle.FLAG_PAIRWISE_COLSUM: _lib.FLAG_PAIRWISE_COLSUM,
                 oracle.FLAG_DENSE_F_COLSUM: _lib.FLAG_DENSE_F_COLSUM,
                 oracle.FLAG_DENSE_F_COLSUM_ITER0: _lib.FLAG_DENSE_F_COLSUM_ITER0}
    colsum = to_device[oracle.colsum_flags("fast4", Hd)]
    dec = bp.decoder_for(H)
    conv_ref = d["converged"].astype(bool)
    assert (~conv_ref).sum() >= 16 and conv_ref.sum() >= 16
    cnt, pred, conv = dec.decode_shots(L, d["detections"], mc.dem_prior(probs), d["actual"], max_iter=int(d["max_iter"]),
                                       flags=colsum | _lib.FLAG_OSD0)
    print(names(cnt))
    assert np.array_equal(conv, conv_ref)
    assert np.array_equal(pred, d["predictions"]), np.flatnonzero(pred != d["predictions"])
    wrong = d["predictions"] != d["actual"]
    assert cnt[0] == len(conv_ref) and cnt[1] == wrong.sum() and cnt[6] == (~conv_ref).sum()
    assert cnt[7] == d["iters"].sum() and cnt[8] == (wrong & ~conv_ref).sum() and cnt[10] == 0


def test_run_shots_and_cli_end_to_end(tmp_path):
    text = synthetic_dem_text()
    H, L, probs = dem.parse_dem(text)
    m, k = H.shape[0], L.shape[0]
    syn, actual = draw(H, L, probs * 3, 700, seed=17)
    obs = shots.obs_of(actual, k)
    f = tmp_path / "synthetic.dem"
    f.write_text(text)
    shots.write_shots(tmp_path / "dets.b8", syn, "b8")
    shots.write_shots(tmp_path / "obs.b8", obs, "b8")
    want = mc.run_shots(H, L, syn, obs, prior=mc.dem_prior(probs), osd=True)
    assert np.array_equal(want[0], compose(bp.decoder_for(H), H, L, syn, actual, mc.dem_prior(probs), _lib.FLAG_OSD0)[0])
    packed = mc.run_shots(H, L, shots.pack_bits(syn), actual, prior=mc.dem_prior(probs), osd=True)
    assert all(np.array_equal(a, b) for a, b in zip(want, packed))
    out = tmp_path / "pred.npy"
    r = subprocess.run([sys.executable, "-m", "qldpc_amd.mc", "--dem", str(f), "--shots", str(tmp_path / "dets.b8"),
                        "--obs", str(tmp_path / "obs.b8"), "--osd", "--predictions-out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert [row["counters"][name] for name in _lib.COUNTER_NAMES] == want[0].tolist()
    assert row["m"] == m and row["k"] == k and row["observables"] is True
    assert np.array_equal(np.load(out), want[1])
