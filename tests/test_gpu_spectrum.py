"""GPU: residual-weight spectra and the iteration histogram of the Monte-Carlo loop (qbp_mc_run_spectrum).  Equality
everywhere, no tolerance: the counters are those of qbp_mc_run_probs, the tables those of tests/spectrum_oracle.py
and, on the reference-made fixture, those of rework/main.py's own loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

from qldpc_amd import _lib, bp, codes, dem, mc
from spectrum_oracle import check_identities, spectrum_counters
from test_gpu_fuzz import capped_matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spectrum.npz")
OSD_CS7, OSD_E8 = _lib.osd_flags("cs", 7), _lib.osd_flags("e", 8)
CODES = ("[[72, 12, 6]]", "[[90, 8, 10]]", "[[108, 8, 10]]", "[[144, 12, 12]]", "[[288, 12, 18]]")


def check_case(dec, L, distance, probs, prior, T, max_iter=50, begin=0, **kw):
    """One spectrum call against qbp_mc_run_probs with the same arguments, and the identities of the tables."""
    want = dec.mc_run_probs(L, distance, probs, prior, begin, begin + T, max_iter=max_iter, **kw)
    cnt, spec, hist = dec.mc_run_spectrum(L, distance, probs, prior, begin, begin + T, max_iter=max_iter, **kw)
    print(kw, "counters", cnt.tolist(), "rows", spec.sum(axis=1).tolist(), "hist", hist[:4].tolist(), int(hist[-1]))
    assert np.array_equal(cnt, want), (cnt, want)
    assert spec.shape == (4, dec.n + 1) and hist.shape == (max_iter + 1,)
    check_identities(cnt, spec, hist, max_iter, osd=bool(kw.get("flags", 0) & _lib.FLAG_OSD0))
    return cnt, spec, hist


@pytest.mark.parametrize("name", CODES)
def test_codes_draws_forced_fast(name):
    code = codes.load_code(name)
    dec = bp.decoder_for(code.Hx)
    p = 0.06 if code.n < 200 else 0.05
    prior, probs = mc.prior_of(p, code.n), np.full(code.n, p)
    T = 4000
    base = None
    for draws in (1, 2):
        for flags in (0, _lib.FLAG_FORCE_FULL, _lib.FLAG_FAST_MATH, _lib.FLAG_OSD0):
            got = check_case(dec, code.Lx, code.distance, probs, prior, T, seed=4, begin=17, draws=draws, flags=flags)
            assert dec.info("last_kernel") == 1
            if draws == 1 and flags == 0:
                base = got
            if draws == 1 and flags == _lib.FLAG_FORCE_FULL:       # forced iterations change no output
                assert all(np.array_equal(a, b) for a, b in zip(got, base))
    assert base[1].sum() > 0 and base[2][-1] > 0
    # a scalar p is probs filled with p
    a = dec.mc_run_spectrum(code.Lx, code.distance, p, prior, 0, 500)
    b = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, 0, 500)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_steane_padded_rows():
    code = codes.load_code("steane")                    # rows of weight 4 in the (6, 3) build: padded
    dec = bp.decoder_for(code.Hx)
    L = np.ones((1, 7), np.uint8)
    p = 0.1
    for draws in (1, 2):
        for flags in (0, _lib.FLAG_OSD0):
            check_case(dec, L, 3, np.full(7, p), mc.prior_of(p, 7), 4000, max_iter=20, seed=3, draws=draws, flags=flags)


@pytest.mark.parametrize("variant,kw", [
    (_lib.SUM_PRODUCT, {}),
    (_lib.DAMPED_SP, dict(alpha=0.9, damping=0.8)),
    (_lib.MIN_SUM, dict(alpha=0.8, damping=0.7, clip_llr=25.0)),
])
def test_variants_and_osd_orders(variant, kw):
    code = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(code.Hx)
    p = 0.05
    prior, probs = mc.prior_of(p, code.n), np.full(code.n, p)
    for flags in (0, _lib.FLAG_FORCE_FULL, _lib.FLAG_FAST_MATH, _lib.FLAG_OSD0, OSD_CS7, OSD_E8):
        cnt, spec, hist = check_case(dec, code.Lx, code.distance, probs, prior, 3000, seed=6, variant=variant,
                                     flags=flags, **kw)
        if flags & _lib.FLAG_OSD0:
            assert cnt[6] > 0 and cnt[10] == 0 and spec[1].sum() + spec[3].sum() > 0


@pytest.fixture(scope="module")
def st144():
    return dem.phenomenological("[[144, 12, 12]]", 12, 0.006, 0.01)      # 864 x 2592: the fused wide shape


@pytest.mark.parametrize("generic", [False, True], ids=["on_chip_8_4", "force_generic"])
def test_space_time_dem(st144, generic):
    H, L, probs = st144
    assert H.shape == (864, 2592)
    dec = _lib.Decoder(*bp.csr_from_H(H))
    if generic:
        dec.set_option(_lib.OPT_FORCE_GENERIC, 1)
    prior = mc.dem_prior(probs)
    for variant, flags, T in ((_lib.SUM_PRODUCT, 0, 1500), (_lib.MIN_SUM, 0, 800), (_lib.SUM_PRODUCT, _lib.FLAG_OSD0, 600)):
        check_case(dec, L, 0, probs, prior, T, seed=12, variant=variant, flags=flags, alpha=0.9)
        assert dec.info("last_kernel") == (2 if generic else 1)
    if not generic:
        for big in (1, 2):                               # the blocked kernel and the row-swapping one
            dec.set_option(_lib.OPT_OSD_BIG, big)
            check_case(dec, L, 0, probs, prior, 300, seed=12, flags=_lib.FLAG_OSD0)
    dec.close()


def test_osd_big_kernels_on_a_code():
    code = codes.load_code("[[144, 12, 12]]")
    p = 0.05
    prior, probs = mc.prior_of(p, code.n), np.full(code.n, p)
    ref = None
    for big in (0, 1, 2):
        dec = _lib.Decoder(*bp.csr_from_H(code.Hx))
        dec.set_option(_lib.OPT_OSD_BIG, big)
        got = check_case(dec, code.Lx, code.distance, probs, prior, 2000, seed=2, flags=_lib.FLAG_OSD0)
        ref = got if ref is None else ref
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))       # the three OSD-0 kernels agree
        dec.close()


def test_random_irregular_matrices():
    rng = np.random.default_rng(5)
    wide = (rng.random((40, 90)) < 0.12).astype(np.int64)
    Lw = (rng.random((5, 90)) < 0.3).astype(np.uint8)
    capped = capped_matrix(rng, 150, 260, 6, 3, 0.8)
    Lc = (rng.random((5, 260)) < 0.3).astype(np.uint8)
    probs = rng.uniform(0.01, 0.05, 260)
    for force in (0, 1):
        dec = _lib.Decoder(*bp.csr_from_H(capped))
        dec.set_option(_lib.OPT_FORCE_GENERIC, force)
        for flags in (0, _lib.FLAG_OSD0):
            check_case(dec, Lc, 0, probs, mc.dem_prior(probs), 1500, seed=3, flags=flags)
            assert dec.info("last_kernel") == (2 if force else 1)
        dec.close()
    probs = rng.uniform(0.01, 0.05, 90)
    for mem in (0, 1, 2):
        dec = _lib.Decoder(*bp.csr_from_H(wide))
        dec.set_option(_lib.OPT_GENERAL_MEM, mem)
        for variant in (_lib.SUM_PRODUCT, _lib.DAMPED_SP, _lib.MIN_SUM):
            for flags in (0, _lib.FLAG_OSD0, _lib.FLAG_FORCE_FULL):
                check_case(dec, Lw, 0, probs, mc.dem_prior(probs), 1500, seed=3, variant=variant, flags=flags,
                           damping=0.8, alpha=0.9)
                assert dec.info("last_kernel") == 2
        dec.close()


@pytest.mark.parametrize("T,kw", [(20000, dict(osd=False)), (20000, dict(osd=True)),
                                  (3000, dict(osd=True, osd_method="cs", osd_order=7))], ids=["bp", "osd0", "cs7"])
def test_tables_equal_the_cpu_oracle(T, kw):
    code = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(code.Hx)
    p = 0.05
    prior = mc.prior_of(p, code.n)
    flags = mc.osd_run_flags(kw["osd"], kw.get("osd_method", "cs"), kw.get("osd_order", 0))
    got = check_case(dec, code.Lx, code.distance, np.full(code.n, p), prior, T, seed=9, flags=flags)
    want = spectrum_counters(code.Hx, code.Lx, code.distance, p, prior, 0, T, seed=9, max_iter=50, **kw)
    for a, b, what in zip(got, want, ("counters", "spectrum", "iter_hist")):
        assert np.array_equal(a, b), (what, a, b)
    assert got[1][0].sum() > 0 and got[1][3].sum() > 0 and (not kw["osd"] or got[1][1].sum() > 0)


def test_split_invariance_accumulation_and_device_entry():
    import torch
    code = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(code.Hx)
    p, T, a = 0.05, 30000, 12345
    prior, probs = mc.prior_of(p, code.n), np.full(code.n, p)
    for flags in (0, _lib.FLAG_OSD0):
        cnt, spec, hist = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, 0, T, seed=8, flags=flags)
        # [0, T) = [0, a) + [a, T) accumulated into the same buffers, which start non-zero
        s0 = np.arange(4 * (code.n + 1), dtype=np.int64).reshape(4, code.n + 1) + 5
        h0 = np.arange(51, dtype=np.int64) + 3
        s, h = s0.copy(), h0.copy()
        c1, _, _ = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, 0, a, seed=8, flags=flags, spectrum=s,
                                       iter_hist=h)
        c2, _, _ = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, a, T, seed=8, flags=flags, spectrum=s,
                                       iter_hist=h)
        assert np.array_equal(c1 + c2, cnt) and np.array_equal(s - s0, spec) and np.array_equal(h - h0, hist)
        # the _device entry on torch buffers, on the caller's stream, in two ranges; iter_hist is optional
        dev = torch.device("cuda", 0)
        d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
        d_spec = torch.from_numpy(s0).to(dev)
        d_hist = torch.from_numpy(h0).to(dev)
        d_spec2 = torch.zeros((4, code.n + 1), dtype=torch.int64, device=dev)
        d_prior = torch.from_numpy(prior).to(dev)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            for lo, hi in ((0, a), (a, T)):
                dec.mc_run_spectrum_device(code.Lx, code.distance, probs, d_prior.data_ptr(), lo, hi, d_cnt.data_ptr(),
                                           d_spec.data_ptr(), d_hist.data_ptr(), seed=8, flags=flags,
                                           stream=side.cuda_stream)
            dec.mc_run_spectrum_device(code.Lx, code.distance, probs, d_prior.data_ptr(), 0, T, d_cnt.data_ptr(),
                                       d_spec2.data_ptr(), 0, seed=8, flags=flags, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(d_cnt.cpu().numpy(), 2 * cnt)
        assert np.array_equal(d_spec.cpu().numpy() - s0, spec) and np.array_equal(d_hist.cpu().numpy() - h0, hist)
        assert np.array_equal(d_spec2.cpu().numpy(), spec)
        got = mc.run_spectrum("[[72, 12, 6]]", [p], T, seed=8, osd=flags != 0)
        assert np.array_equal(got[0][0], cnt) and np.array_equal(got[1][0], spec) and np.array_equal(got[2][0], hist)
    # a trial range longer than the library's OSD step: several chunks
    T = dec.mc_osd_step() + dec.mc_osd_step() // 3
    p = 0.02
    check_case(dec, code.Lx, code.distance, np.full(code.n, p), mc.prior_of(p, code.n), T, seed=1, flags=_lib.FLAG_OSD0)
    H, L, pr = dem.phenomenological("[[72, 12, 6]]", 3, 0.01, 0.02)
    decd = bp.decoder_for(H)
    want = decd.mc_run_spectrum(L, 0, pr, mc.dem_prior(pr), 0, 5000, seed=2, max_iter=30, flags=_lib.FLAG_OSD0)
    got = mc.run_dem_spectrum(H, L, pr, 5000, seed=2, max_iter=30, osd=True)
    assert all(np.array_equal(g[0], w) for g, w in zip(got, want))


def test_reference_fixture_through_the_product_path():
    """tests/golden/spectrum.npz: error patterns drawn and classified by the reference's own rework/main.py loop;
    qbp_mc_run_errors_spectrum reproduces its four weight lists and its iteration list exactly."""
    z = np.load(GOLDEN)
    for name in z["names"]:
        code = codes.load_code(str(z[f"{name}/code"]))
        p, max_iter, osd = float(z[f"{name}/meta"][0]), int(z[f"{name}/meta"][1]), bool(z[f"{name}/meta"][2])
        errors = np.unpackbits(z[f"{name}/errors"], axis=1)[:, :code.n]
        dec = bp.decoder_for(code.Hx)
        cnt, spec, hist = dec.mc_run_errors_spectrum(code.Lx, code.distance, errors, mc.prior_of(p, code.n),
                                                     max_iter=max_iter, flags=_lib.FLAG_OSD0 if osd else 0)
        print(name, cnt.tolist(), spec.sum(axis=1).tolist())
        assert np.array_equal(spec, z[f"{name}/weights"]), name
        its = z[f"{name}/iterations"].astype(np.int64)              # per trial, the reference's `iteration`
        assert cnt[0] == len(errors) and cnt[7] == its.sum()
        ref_hist = np.bincount(its, minlength=max_iter + 1)
        ref_hist[max_iter - 1] -= cnt[6]                            # unconverged trials report max_iter - 1
        ref_hist[max_iter] += cnt[6]
        assert np.array_equal(hist, ref_hist), name
        assert np.array_equal(cnt, dec.mc_run_errors(code.Lx, code.distance, errors, mc.prior_of(p, code.n),
                                                     max_iter=max_iter, flags=_lib.FLAG_OSD0 if osd else 0))
        check_identities(cnt, spec, hist, max_iter, osd)


def test_invalid_arguments_leave_the_buffers_untouched():
    code = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(code.Hx)
    n = code.n
    prior, probs = mc.prior_of(0.05, n), np.full(n, 0.05)
    Lx = np.ascontiguousarray(code.Lx)
    lib = _lib.load()
    c0 = np.arange(12, dtype=np.int64) + 7
    s0 = np.arange(4 * (n + 1), dtype=np.int64) + 11
    h0 = np.arange(1100, dtype=np.int64) + 13

    def call(max_iter=50, flags=0, spectrum=True):
        c, s, h = c0.copy(), s0.copy(), h0.copy()
        rc = lib.qbp_mc_run_spectrum(dec._h, Lx.ctypes.data, Lx.shape[0], code.distance, probs.ctypes.data, 1, 0, 0,
                                     1000, prior.ctypes.data, max_iter, 0, 1.0, 1.0, 20.0, flags, c.ctypes.data,
                                     s.ctypes.data if spectrum else None, h.ctypes.data)
        assert np.array_equal(c, c0) and np.array_equal(s, s0) and np.array_equal(h, h0)
        return rc

    assert call(spectrum=False) == -1 and b"spectrum" in lib.qbp_last_error()
    assert call(max_iter=_lib.MC_SPECTRUM_MAX_ITER + 1) == -1
    assert call(flags=_lib.FLAG_OSD_CS | (3 << 16)) == -1 and call(flags=_lib.FLAG_OSD0 | (3 << 16)) == -1
    assert call(max_iter=0) == -1
    errs = np.zeros((10, n), np.uint8)
    for kw in (dict(spec=False), dict(max_iter=1025), dict(flags=_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS)):
        c, s, h = c0.copy(), s0.copy(), h0.copy()
        rc = lib.qbp_mc_run_errors_spectrum(dec._h, Lx.ctypes.data, Lx.shape[0], code.distance, errs.ctypes.data, 10,
                                            prior.ctypes.data, kw.get("max_iter", 50), 0, 1.0, 1.0, 20.0,
                                            kw.get("flags", 0), c.ctypes.data,
                                            s.ctypes.data if kw.get("spec", True) else None, h.ctypes.data)
        assert rc == -1 and np.array_equal(c, c0) and np.array_equal(s, s0) and np.array_equal(h, h0)
    with pytest.raises(_lib.QbpError) as e:                  # the _device entry: before any launch
        dec.mc_run_spectrum_device(Lx, code.distance, probs, 0, 0, 1000, 0, 0)
    assert e.value.code == -1
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_spectrum(Lx, code.distance, probs, prior, 0, 1000, max_iter=1025)
    assert e.value.code == -1
    # (the limit itself is accepted)
    cnt, spec, hist = dec.mc_run_spectrum(Lx, code.distance, probs, prior, 0, 2000, max_iter=_lib.MC_SPECTRUM_MAX_ITER)
    check_identities(cnt, spec, hist, _lib.MC_SPECTRUM_MAX_ITER, False)
    # unsupported exactly where qbp_mc_run_probs is: order-w OSD beyond the one-wavefront kernel
    H, L, pr = dem.phenomenological("[[288, 12, 18]]", 18, 0.004)
    big = bp.decoder_for(H)
    with pytest.raises(_lib.QbpError) as e:
        big.mc_run_spectrum(L, 0, pr, mc.dem_prior(pr), 0, 100, flags=OSD_CS7)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_stabilizer_spectrum_and_rework_results():
    name = "[[72, 12, 6]]"
    spectra = mc.stabilizer_spectrum([name], trials=20000, seed=3)
    cnt, weights, its = mc.run_spectrum(name, [0.005], 20000, seed=3, osd=True)
    assert np.array_equal(spectra[name], weights[0, 0] + weights[0, 1])
    assert spectra[name][0] == 0 and spectra[name].sum() == cnt[0, 5]
    res = mc.rework_results([{"code": name, "name": "72", "physicalErrorRates": [0.06, 0.03]}], trials=5000, max_iter=40)
    cnt, weights, its = mc.run_spectrum(name, [0.06, 0.03], 5000, max_iter=40, osd=True)
    for i, p in enumerate((0.06, 0.03)):
        pt = res["72"][p]
        assert pt["logical"] == cnt[i, 1] / 5000 and pt["osd"] == cnt[i, 6] / 5000
        assert pt["average_iterations"] == cnt[i, 7] / 5000
        for r, key in enumerate(mc.REWORK_WEIGHT_LISTS):
            assert np.array_equal(np.bincount(pt[key], minlength=73), weights[i, r])


def test_cli_two_rank_self_launch(tmp_path):
    """`python -m qldpc_amd.mc --spectrum out.npz --gpus 2` over gloo: counters and both tables equal the one-rank run
    and the library's own."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    outs = []
    for gpus in (1, 2):
        f = str(tmp_path / f"spectrum{gpus}.npz")
        cmd = [sys.executable, "-m", "qldpc_amd.mc", "--code", "72", "--p", "0.05", "0.02", "--trials", "30001", "--osd",
               "--max-iter", "40", "--spectrum", f, "--gpus", str(gpus), "--backend", "gloo", "--share-device"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(f))
    code = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(code.Hx)
    for i, p in enumerate((0.05, 0.02)):
        want = dec.mc_run_spectrum(code.Lx, code.distance, p, mc.prior_of(p, code.n), 0, 30001, max_iter=40,
                                   flags=_lib.FLAG_OSD0)
        for z in outs:
            assert np.array_equal(z["counters"][i], want[0]) and np.array_equal(z["weights"][i], want[1])
            assert np.array_equal(z["iterations"][i], want[2])
