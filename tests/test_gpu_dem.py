"""GPU: Monte-Carlo on detector error models (qbp_mc_run_probs: a probability per column) against the numpy
statement of the sampler (tests/dem_sampler.py), the uniform path (qbp_mc_run) and the CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dem_sampler import errors_probs
from oracle import oracle
from qldpc_amd import _lib, bp, codes, dem, mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSD_CS7 = _lib.osd_flags("cs", 7)


def decoder(H):
    return bp.decoder_for(H)


def synthetic_dem_text(seed=3):
    """Phenomenological DEM of [[72,12,6]] over 4 rounds (data rate p, measurement rate q) plus hyperedge mechanisms
    of weight 3-6 (some repeated, so that they merge; some flipping observables) and observable-only mechanisms."""
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
    for i in range(240):                                   # 160 distinct, 80 repeats that merge
        dets, obs = hyper[i % 160] if i < 160 else hyper[int(rng.integers(0, 160))]
        p = float(rng.uniform(1e-4, 4e-3))
        toks = [f"D{d}" for d in dets]
        if len(toks) > 3:                                  # some written with '^' components
            toks.insert(2, "^")
        lines.append(f"error({p!r}) " + " ".join(toks + [f"L{o}" for o in obs]))
    for o in (0, 5, 11, 5):
        lines.append(f"error(0.0005) L{o}")                # undetectable logical mechanisms (L5 merges)
    lines.append("error(0.01) D3 ^ D3")                   # flips nothing: dropped
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def synthetic():
    H, L, probs = dem.parse_dem(synthetic_dem_text())
    Hd = H.toarray()
    assert Hd.sum(axis=0).max() == 6 and Hd.sum(axis=1).max() > 8
    assert (Hd.sum(axis=0) == 0).sum() == 3
    return H, L, probs


@pytest.fixture(scope="module")
def st144():
    return dem.phenomenological("[[144, 12, 12]]", 12, 0.01)


# ---- 1. the sampler, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steane", "[[72, 12, 6]]", "[[144, 12, 12]]"])
def test_sampler_bit_exact(name):
    code = codes.load_code(name)
    n = code.n
    dec = decoder(code.Hx)
    rng = np.random.default_rng(1)
    cases = [np.zeros(n), np.ones(n), np.full(n, 2.0 ** -30), np.full(n, 0.5),
             rng.choice([0.0, 1.0, 2.0 ** -30, 0.5, 0.03, 0.2], size=n),
             rng.uniform(0, 0.3, size=n)]
    for probs in cases:
        for draws, seed, begin in ((1, 0, 0), (2, 0xDEADBEEF12345, 2 ** 33 + 5), (1, 7, 2 ** 32 - 100)):
            got = dec.mc_sample_errors_probs(probs, begin, 300, draws=draws, seed=seed)
            assert np.array_equal(got, errors_probs(probs, draws, seed, begin, 300)), (name, draws, begin)


def test_sampler_equal_probs_is_uniform_sampler():
    code = codes.load_code("[[288, 12, 18]]")
    dec = decoder(code.Hx)
    got = dec.mc_sample_errors_probs(np.full(code.n, 0.07), 2 ** 33, 500, draws=2, seed=11)
    assert np.array_equal(got, dec.mc_sample_errors(0.07, 2 ** 33, 500, draws=2, seed=11))


# ---- 2. all-equal probabilities: the counters of qbp_mc_run, digit for digit --------------------------------------
def equal_prob_cases():
    c144 = codes.load_code("[[144, 12, 12]]")
    yield "144", c144.Hx, c144.Lx, c144.distance, 0.05, 4000, 1
    H, L, _ = dem.phenomenological("[[144, 12, 12]]", 12, 0.0)
    yield "st144", H, L, 12, 0.01, 3000, 1
    H, L, _ = dem.phenomenological("[[288, 12, 18]]", 18, 0.0)
    yield "st288", H, L, 18, 0.006, 1500, 2


@pytest.mark.parametrize("case", list(equal_prob_cases()), ids=lambda c: c[0])
def test_equal_probs_equal_mc_run(case):
    tag, H, L, distance, p, T, draws = case
    dec = decoder(H)
    n = H.shape[1]
    prior = mc.prior_of(p, n)
    probs = np.full(n, p)
    expect_kind = {"144": 1, "st144": 1, "st288": 2}[tag]
    for flags in (0, _lib.FLAG_OSD0, OSD_CS7):
        try:
            want = dec.mc_run(L, distance, p, prior, 100, 100 + T, draws=draws, seed=21, flags=flags)
        except _lib.QbpError as e:
            assert flags == OSD_CS7 and e.code == _lib.E_UNSUPPORTED
            with pytest.raises(_lib.QbpError) as e2:
                dec.mc_run_probs(L, distance, probs, prior, 100, 100 + T, draws=draws, seed=21, flags=flags)
            assert e2.value.code == _lib.E_UNSUPPORTED
            continue
        got = dec.mc_run_probs(L, distance, probs, prior, 100, 100 + T, draws=draws, seed=21, flags=flags)
        assert dec.info("last_kernel") == expect_kind
        print(tag, flags, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
        assert np.array_equal(got, want), (tag, flags)
        assert got[0] == T


def test_equal_probs_all_variants_and_forced(st144):
    H, L, _ = st144
    dec = decoder(H)
    n = H.shape[1]
    p = 0.012
    probs = np.full(n, p)
    prior = mc.prior_of(p, n)
    for variant, kw in ((_lib.SUM_PRODUCT, {}), (_lib.DAMPED_SP, dict(damping=0.7)),
                        (_lib.MIN_SUM, dict(alpha=0.8))):
        for flags in (0, _lib.FLAG_FORCE_FULL, _lib.FLAG_FAST_MATH):
            want = dec.mc_run(L, 12, p, prior, 0, 1500, seed=4, variant=variant, flags=flags, **kw)
            got = dec.mc_run_probs(L, 12, probs, prior, 0, 1500, seed=4, variant=variant, flags=flags, **kw)
            assert np.array_equal(got, want), (variant, flags)


def test_equal_probs_general_kernel_memory_modes(synthetic):
    H, L, probs = synthetic
    n = H.shape[1]
    p = 0.003
    prior = mc.prior_of(p, n)
    for mem in (1, 2, 0):
        dec = _lib.Decoder(*bp.csr_from_H(H))
        dec.set_option(_lib.OPT_GENERAL_MEM, mem)
        for variant in (_lib.SUM_PRODUCT, _lib.DAMPED_SP, _lib.MIN_SUM):
            want = dec.mc_run(L, 0, p, prior, 0, 2000, seed=8, variant=variant, damping=0.8, alpha=0.9)
            got = dec.mc_run_probs(L, 0, np.full(n, p), prior, 0, 2000, seed=8, variant=variant, damping=0.8,
                                   alpha=0.9)
            assert dec.info("last_kernel") == 2
            assert np.array_equal(got, want), (mem, variant)
        dec.close()


# ---- 3. different rates: the device pipeline against mc_run_errors and the CPU oracle ----------------------------
def oracle_counters(H, L, errors, prior, osd):
    Hd = np.asarray(H.toarray(), np.int64)
    syn = (errors.astype(np.int64) @ Hd.T % 2).astype(np.uint8)
    hard, conv, iters, llr = oracle.decode_batch(Hd, syn, prior, 50)
    if osd:
        hard = hard.copy()
        for i in np.flatnonzero(~conv):
            hard[i] = oracle.osd0(Hd, syn[i], llr[i], hard[i])
    cnt = oracle.classify_trials(Hd, L, 0, errors, syn, hard, conv, iters)
    if osd:
        cnt[10] = sum(not np.array_equal((hard[i].astype(np.int64) @ Hd.T) % 2, syn[i]) for i in np.flatnonzero(~conv))
    return cnt


@pytest.mark.parametrize("model", ["st144_pq", "synthetic"])
def test_per_column_rates_match_oracle(model, synthetic):
    if model == "synthetic":
        H, L, probs = synthetic
        T, kind = 2500, 2
    else:
        H, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.006, 0.02)
        T, kind = 2000, 1
    dec = decoder(H)
    prior = mc.dem_prior(probs)
    begin, seed = 2 ** 32 + 3, 77
    errors = errors_probs(probs, 1, seed, begin, T)
    assert np.array_equal(dec.mc_sample_errors_probs(probs, begin, T, seed=seed), errors)
    for flags in (0, _lib.FLAG_OSD0):
        # (the oracle's OSD-0 eliminates dense byte matrices: fewer trials on the 864 x 2592 matrix)
        Tf = T if (flags == 0 or model == "synthetic") else 300
        got = dec.mc_run_probs(L, 0, probs, prior, begin, begin + Tf, seed=seed, flags=flags)
        assert dec.info("last_kernel") == kind
        print(model, flags, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
        assert np.array_equal(got, dec.mc_run_errors(L, 0, errors[:Tf], prior, flags=flags))
        assert np.array_equal(got, oracle_counters(H, L, errors[:Tf], prior, flags != 0))
        assert got[4] == got[1] and got[3] == 0       # distance 0: every logical error counts as incorrectable


def test_undetectable_mechanism_is_drawn():
    """An observable-only column (no check) still fails at its rate: a logical error BP cannot see."""
    H, L, probs = dem.parse_dem("error(0.01) D0 D1\nerror(0.01) D1 D2\nerror(0.01) D2 D3\nerror(0.25) L0\n")
    dec = decoder(H)
    T = 20000
    got = dec.mc_run_probs(L, 0, probs, mc.dem_prior(probs), 0, T, seed=3)
    errors = errors_probs(probs, 1, 3, 0, T)
    assert np.array_equal(got, dec.mc_run_errors(L, 0, errors, mc.dem_prior(probs)))
    assert abs(got[1] / T - 0.25) < 0.02


# ---- 4. ranges, shards, the device entry, the threshold cache ----------------------------------------------------
def test_ranges_compose_and_device_entry(st144):
    import torch
    H, L, _ = st144
    n = H.shape[1]
    probs = np.where(np.arange(n) < 1728, 0.008, 0.015)
    prior = mc.dem_prior(probs)
    dec = decoder(H)
    a, b, c = 5, 1234, 3000
    whole = dec.mc_run_probs(L, 0, probs, prior, a, c, seed=1)
    assert np.array_equal(whole, dec.mc_run_probs(L, 0, probs, prior, a, b, seed=1) +
                          dec.mc_run_probs(L, 0, probs, prior, b, c, seed=1))
    dev = torch.device("cuda", 0)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    d_prior = torch.from_numpy(prior).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for lo, hi in ((a, b), (b, c)):
        dec.mc_run_probs_device(L, 0, probs, d_prior.data_ptr(), lo, hi, d_cnt.data_ptr(), seed=1, stream=stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_cnt.cpu().numpy(), whole)
    # run_dem: one rank, and seven shards summed by an injected reduction, equal the host entry
    assert np.array_equal(mc.run_dem(H, L, probs, c - a, seed=1, prior=prior), dec.mc_run_probs(
        L, 0, probs, prior, 0, c - a, seed=1))
    # changed probabilities are noticed (thresholds re-uploaded), and changing back restores the counters
    other = probs[::-1].copy()
    first = dec.mc_run_probs(L, 0, other, prior, a, c, seed=1)
    assert np.array_equal(first, dec.mc_run_errors(L, 0, errors_probs(other, 1, 1, a, c - a), prior))
    assert np.array_equal(dec.mc_run_probs(L, 0, probs, prior, a, c, seed=1), whole)


# ---- 5. errors ---------------------------------------------------------------------------------------------------
def test_bad_probs_invalid_and_counters_untouched():
    code = codes.load_code("[[72, 12, 6]]")
    dec = decoder(code.Hx)
    n = code.n
    prior = mc.prior_of(0.05, n)
    Lx = np.ascontiguousarray(code.Lx)
    lib = _lib.load()
    for bad in (np.nan, -0.1, 1.5, -np.inf, np.inf):
        probs = np.full(n, 0.05)
        probs[n // 2] = bad
        counters = np.arange(12, dtype=np.int64) + 7
        rc = lib.qbp_mc_run_probs(dec._h, Lx.ctypes.data, Lx.shape[0], 6, probs.ctypes.data, 1, 0, 0, 1000,
                                  prior.ctypes.data, 50, 0, 1.0, 1.0, 20.0, 0, counters.ctypes.data)
        assert rc == -1 and np.array_equal(counters, np.arange(12) + 7)
        out = np.zeros((4, n), np.uint8)
        assert lib.qbp_mc_sample_errors_probs(dec._h, probs.ctypes.data, 1, 0, 0, 4, out.ctypes.data) == -1
        with pytest.raises(_lib.QbpError) as e:
            dec.mc_run_probs_device(Lx, 6, probs, 0, 0, 1000, 0)
        assert e.value.code == -1
    counters = np.zeros(12, np.int64)
    assert lib.qbp_mc_run_probs(dec._h, Lx.ctypes.data, Lx.shape[0], 6, None, 1, 0, 0, 1000, prior.ctypes.data, 50,
                                0, 1.0, 1.0, 20.0, 0, counters.ctypes.data) == -1
    out = np.zeros((4, n), np.uint8)
    assert lib.qbp_mc_sample_errors_probs(dec._h, None, 1, 0, 0, 4, out.ctypes.data) == -1
    assert not counters.any()


def test_cs7_beyond_one_wavefront_unsupported():
    H, L, probs = dem.phenomenological("[[288, 12, 18]]", 18, 0.004)
    dec = decoder(H)
    prior = mc.dem_prior(probs)
    for call in (lambda: dec.mc_run(L, 18, 0.004, prior, 0, 64, flags=OSD_CS7),
                 lambda: dec.mc_run_probs(L, 18, probs, prior, 0, 64, flags=OSD_CS7)):
        with pytest.raises(_lib.QbpError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED


# ---- 6. end to end -----------------------------------------------------------------------------------------------
def test_cli_dem_end_to_end(tmp_path, synthetic):
    import json
    f = tmp_path / "synthetic.dem"
    f.write_text(synthetic_dem_text())
    out = tmp_path / "out.json"
    r = subprocess.run([sys.executable, "-m", "qldpc_amd.mc", "--dem", str(f), "--trials", "3000", "--seed", "5",
                        "--osd", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "dem=" in r.stdout and "LER=" in r.stdout and "trials/s" in r.stdout
    row = json.loads(out.read_text())["points"][0]
    H, L, probs = synthetic
    want = decoder(H).mc_run_probs(L, 0, probs, mc.dem_prior(probs), 0, 3000, seed=5, flags=_lib.FLAG_OSD0)
    assert [row[k] for k in _lib.COUNTER_NAMES] == want.tolist()
