"""GPU: Monte-Carlo over a ladder of BP iteration budgets in one pass (qbp_mc_run_budgets).  The acceptance test is
equality, no tolerance anywhere: row j of the ladder is what qbp_mc_run_probs returns with max_iter = budgets[j]."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from qldpc_amd import _lib, bp, codes, dem, mc
from test_gpu_fuzz import capped_matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENS = tuple(range(10, 100, 10))                       # the reference script's ladder (BP_per_Iteration.py:17)
FULL = tuple(range(1, _lib.MC_MAX_BUDGETS + 1))        # the maximum count
OSD_CS7, OSD_E8 = _lib.osd_flags("cs", 7), _lib.osd_flags("e", 8)


def check_ladder(dec, L, distance, probs, prior, budgets, T, uniform_p=None, begin=0, **kw):
    """One ladder call against one qbp_mc_run_probs call per budget (and qbp_mc_run for a uniform p).  The rows
    must differ: not_converged is non-increasing along them and, with more than one row, strictly larger in the
    first than in the last (a single budget has nothing to differ from: it pins the last-row path alone)."""
    got = dec.mc_run_budgets(L, distance, probs, prior, budgets, begin, begin + T, **kw)
    want = np.stack([dec.mc_run_probs(L, distance, probs, prior, begin, begin + T, max_iter=b, **kw) for b in budgets])
    print(budgets, kw, "not_converged", got[:, 6].tolist(), "sum_iterations", got[:, 7].tolist())
    assert got.shape == (len(budgets), 12)
    assert np.array_equal(got, want), (got, want)
    if uniform_p is not None:
        runs = np.stack([dec.mc_run(L, distance, uniform_p, prior, begin, begin + T, max_iter=b, **kw) for b in budgets])
        assert np.array_equal(got, runs)
    assert (got[:, 0] == T).all()
    assert (np.diff(got[:, 6]) <= 0).all()
    if len(budgets) > 1:
        assert got[0, 6] > got[-1, 6]
    return got


@pytest.mark.parametrize("name,p,T,sets", [
    ("[[72, 12, 6]]", 0.06, 4000, ((50,), (1, 2, 3), (10, 11, 12), TENS, FULL)),
    ("[[144, 12, 12]]", 0.05, 4000, ((50,), (1, 2, 3), (10, 11, 12), TENS, FULL)),
    ("[[288, 12, 18]]", 0.05, 3000, ((10, 11, 12), TENS)),
])
def test_codes_every_budget_set(name, p, T, sets):
    code = codes.load_code(name)
    dec = bp.decoder_for(code.Hx)
    prior = mc.prior_of(p, code.n)
    for budgets in sets:
        check_ladder(dec, code.Lx, code.distance, np.full(code.n, p), prior, budgets, T, uniform_p=p, seed=4, begin=17)
        assert dec.info("last_kernel") == 1
    # a scalar p is probs filled with p
    assert np.array_equal(dec.mc_run_budgets(code.Lx, code.distance, p, prior, (3, 9), 0, 500),
                          dec.mc_run_budgets(code.Lx, code.distance, np.full(code.n, p), prior, (3, 9), 0, 500))


def test_steane_padded_rows():
    code = codes.load_code("steane")                    # rows of weight 4 in the (6, 3) build: padded
    dec = bp.decoder_for(code.Hx)
    L = np.ones((1, 7), np.uint8)                       # the logical X of the Steane code
    p = 0.1
    for budgets in ((1, 2, 3), FULL):
        for draws in (1, 2):
            check_ladder(dec, L, 3, np.full(7, p), mc.prior_of(p, 7), budgets, 4000, uniform_p=p, seed=3, draws=draws)


@pytest.mark.parametrize("variant,kw", [
    (_lib.SUM_PRODUCT, {}),
    (_lib.DAMPED_SP, dict(alpha=0.9, damping=0.8)),
    (_lib.MIN_SUM, dict(alpha=0.8, damping=0.7, clip_llr=25.0)),
])
def test_variants_draws_and_forced(variant, kw):
    code = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(code.Hx)
    p = 0.05
    prior = mc.prior_of(p, code.n)
    probs = np.full(code.n, p)
    for draws, budgets in ((1, (1, 2, 3)), (2, (10, 11, 12)), (2, TENS)):
        free = check_ladder(dec, code.Lx, code.distance, probs, prior, budgets, 3000, uniform_p=p, seed=6, draws=draws,
                            variant=variant, **kw)
        forced = dec.mc_run_budgets(code.Lx, code.distance, probs, prior, budgets, 0, 3000, seed=6, draws=draws,
                                    variant=variant, flags=_lib.FLAG_FORCE_FULL, **kw)
        assert np.array_equal(free, forced)
    fast = _lib.FLAG_FAST_MATH
    check_ladder(dec, code.Lx, code.distance, probs, prior, (5, 10, 20), 2000, seed=6, variant=variant, flags=fast, **kw)


@pytest.mark.parametrize("flags", [_lib.FLAG_OSD0, OSD_CS7, OSD_E8], ids=["osd0", "cs7", "e8"])
def test_osd_flags_on_144(flags):
    code = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(code.Hx)
    p = 0.05
    prior = mc.prior_of(p, code.n)
    for budgets in ((50,), (1, 2, 3), (10, 11, 12), TENS):
        got = check_ladder(dec, code.Lx, code.distance, np.full(code.n, p), prior, budgets, 2000, uniform_p=p, seed=2,
                           flags=flags)
        assert got[0, 6] > 0 and not got[:, 10].any()


def test_osd0_pipeline_matches_cpu_oracle():
    """[[144,12,12]], p = 0.05, 20 000 trials, seed 9, OSD-0: every row equals the CPU oracle pipeline at that budget."""
    code = codes.load_code("[[144, 12, 12]]")
    dec = bp.decoder_for(code.Hx)
    p, T, budgets = 0.05, 20000, (5, 10, 20, 50)
    prior = mc.prior_of(p, code.n)
    got = dec.mc_run_budgets(code.Lx, code.distance, p, prior, budgets, 0, T, seed=9, flags=_lib.FLAG_OSD0)
    print(got)
    assert got[-1, 6] > 100 and (np.diff(got[:, 6]) < 0).all()
    for j, b in enumerate(budgets):
        want = oracle.mc_counters(code.Hx, code.Lx, code.distance, p, prior, 0, T, seed=9, max_iter=b, osd=True)
        assert np.array_equal(got[j], want), (b, got[j], want)


@pytest.fixture(scope="module")
def st144():
    return dem.phenomenological("[[144, 12, 12]]", 12, 0.006, 0.01)      # 864 x 2592, rates p (data) and q


@pytest.mark.parametrize("generic", [False, True], ids=["on_chip_8_4", "force_generic"])
def test_space_time_dem(st144, generic):
    H, L, probs = st144
    assert H.shape == (864, 2592)
    dec = _lib.Decoder(*bp.csr_from_H(H))
    if generic:
        dec.set_option(_lib.OPT_FORCE_GENERIC, 1)
    prior = mc.dem_prior(probs)
    for variant, flags, T in ((_lib.SUM_PRODUCT, 0, 1500), (_lib.MIN_SUM, 0, 800), (_lib.SUM_PRODUCT, _lib.FLAG_OSD0, 600)):
        check_ladder(dec, L, 0, probs, prior, (5, 10, 20, 50), T, seed=12, variant=variant, flags=flags, alpha=0.9)
        assert dec.info("last_kernel") == (2 if generic else 1)
    dec.close()


def test_random_irregular_matrices():
    """Matrices of the fuzzer's kind: a capped (6, 3) one on the on-chip kernel (padded rows, isolated columns) and a
    wide one (row weights beyond 8, column weights beyond 4) on the general-H kernel in its three memory modes."""
    rng = np.random.default_rng(5)
    wide = (rng.random((40, 90)) < 0.12).astype(np.int64)
    Lw = (rng.random((5, 90)) < 0.3).astype(np.uint8)
    assert wide.sum(axis=1).max() > 8 and wide.sum(axis=0).max() > 4
    capped = capped_matrix(rng, 150, 260, 6, 3, 0.8)
    Lc = (rng.random((5, 260)) < 0.3).astype(np.uint8)
    dec = bp.decoder_for(capped)
    probs = rng.uniform(0.01, 0.05, 260)
    for flags in (0, _lib.FLAG_OSD0):
        for budgets in ((1, 2, 3), (5, 10, 20, 50)):
            check_ladder(dec, Lc, 0, probs, mc.dem_prior(probs), budgets, 1500, seed=3, flags=flags)
            assert dec.info("last_kernel") == 1
    probs = rng.uniform(0.01, 0.05, 90)
    for mem in (0, 1, 2):
        dec = _lib.Decoder(*bp.csr_from_H(wide))
        dec.set_option(_lib.OPT_GENERAL_MEM, mem)
        for variant in (_lib.SUM_PRODUCT, _lib.DAMPED_SP, _lib.MIN_SUM):
            for flags, budgets in ((0, (1, 2, 3)), (_lib.FLAG_OSD0, (10, 11, 12)), (0, FULL)):
                check_ladder(dec, Lw, 0, probs, mc.dem_prior(probs), budgets, 1500, seed=3, variant=variant, flags=flags,
                             damping=0.8, alpha=0.9)
                assert dec.info("last_kernel") == 2
        dec.close()


def test_shards_chunks_and_device_entry():
    import torch
    code = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(code.Hx)
    p, budgets = 0.04, (2, 5, 10, 40)
    prior = mc.prior_of(p, code.n)
    probs = np.full(code.n, p)
    for flags in (0, _lib.FLAG_OSD0):
        T, a = 30000, 12345
        whole = dec.mc_run_budgets(code.Lx, code.distance, probs, prior, budgets, 0, T, seed=8, flags=flags)
        parts = (dec.mc_run_budgets(code.Lx, code.distance, probs, prior, budgets, 0, a, seed=8, flags=flags) +
                 dec.mc_run_budgets(code.Lx, code.distance, probs, prior, budgets, a, T, seed=8, flags=flags))
        assert np.array_equal(whole, parts)
        # the _device entry on torch buffers, on the caller's stream, in two ranges
        dev = torch.device("cuda", 0)
        d_tab = torch.zeros((len(budgets), 12), dtype=torch.int64, device=dev)
        d_prior = torch.from_numpy(prior).to(dev)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            for lo, hi in ((0, a), (a, T)):
                dec.mc_run_budgets_device(code.Lx, code.distance, probs, d_prior.data_ptr(), budgets, lo, hi,
                                          d_tab.data_ptr(), seed=8, flags=flags, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(d_tab.cpu().numpy(), whole)
        assert np.array_equal(mc.run_budgets("[[72, 12, 6]]", p, T, budgets, seed=8, osd=flags != 0), whole)
    # a trial range longer than the library's OSD step: several chunks
    step = dec.mc_budgets_step(len(budgets))
    assert step == dec.mc_osd_step() // len(budgets)
    T = step + step // 3
    p = 0.02
    prior = mc.prior_of(p, code.n)
    got = check_ladder(dec, code.Lx, code.distance, np.full(code.n, p), prior, budgets, T, seed=1, flags=_lib.FLAG_OSD0)
    assert np.array_equal(mc.run_budgets("[[72, 12, 6]]", p, T, budgets, seed=1, osd=True), got)
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 3, 0.01, 0.02)
    decd = bp.decoder_for(H)
    want = decd.mc_run_budgets(L, 0, probs, mc.dem_prior(probs), (3, 8, 30), 0, 5000, seed=2, flags=_lib.FLAG_OSD0)
    assert np.array_equal(mc.run_dem_budgets(H, L, probs, 5000, (3, 8, 30), seed=2, osd=True), want)
    assert want[0, 6] > want[-1, 6]


def test_invalid_arguments_leave_the_counters_untouched():
    code = codes.load_code("[[72, 12, 6]]")
    dec = bp.decoder_for(code.Hx)
    n = code.n
    prior = mc.prior_of(0.05, n)
    probs = np.full(n, 0.05)
    Lx = np.ascontiguousarray(code.Lx)
    lib = _lib.load()
    fill = np.arange(16 * 12, dtype=np.int64).reshape(16, 12) + 7

    def call(budgets, flags=0, n_budgets=None, probs=probs, bud_ptr=True):
        bud = np.asarray(budgets, np.int32)
        counters = fill.copy()
        rc = lib.qbp_mc_run_budgets(dec._h, Lx.ctypes.data, Lx.shape[0], code.distance,
                                    None if probs is None else probs.ctypes.data, 1, 0, 0, 1000, prior.ctypes.data,
                                    bud.ctypes.data if bud_ptr else None, len(bud) if n_budgets is None else n_budgets,
                                    0, 1.0, 1.0, 20.0, flags, counters.ctypes.data)
        assert np.array_equal(counters, fill)
        return rc

    assert call([0, 5]) == -1 and b"budgets" in lib.qbp_last_error()
    assert call([10, 10]) == -1 and call([20, 10]) == -1 and call([-3]) == -1
    assert call([5], n_budgets=0) == -1 and call(list(range(1, 18))) == -1
    assert call([5, 6], bud_ptr=False) == -1 and call([5, 6], probs=None) == -1
    # every flag combination qbp_mc_run refuses
    for flags in (_lib.FLAG_OSD_CS | (3 << 16), _lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | (3 << 16),
                  _lib.FLAG_OSD0 | (3 << 16), _lib.FLAG_OSD0 | _lib.FLAG_OSD_CS, _lib.FLAG_OSD0 | _lib.FLAG_OSD_E | (13 << 16)):
        assert call([5, 6], flags=flags) == -1
        one = np.zeros(12, np.int64)
        assert lib.qbp_mc_run(dec._h, Lx.ctypes.data, Lx.shape[0], code.distance, 0.05, 1, 0, 0, 1000, prior.ctypes.data,
                              50, 0, 1.0, 1.0, 20.0, flags, one.ctypes.data) == -1
    with pytest.raises(_lib.QbpError) as e:                  # the _device entry: before any launch
        dec.mc_run_budgets_device(Lx, code.distance, np.full(n, 1.5), 0, (5, 6), 0, 1000, 0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        dec.mc_run_budgets(Lx, code.distance, probs, prior, (6, 5), 0, 1000)
    # unsupported exactly where qbp_mc_run_probs is: order-w OSD beyond the one-wavefront kernel
    H, L, pr = dem.phenomenological("[[288, 12, 18]]", 18, 0.004)
    big = bp.decoder_for(H)
    for fn in (lambda: big.mc_run_probs(L, 0, pr, mc.dem_prior(pr), 0, 100, flags=OSD_CS7),
               lambda: big.mc_run_budgets(L, 0, pr, mc.dem_prior(pr), (5, 10), 0, 100, flags=OSD_CS7)):
        with pytest.raises(_lib.QbpError) as e:
            fn()
        assert e.value.code == _lib.E_UNSUPPORTED


def test_cli_two_rank_self_launch(tmp_path):
    """`python -m qldpc_amd.mc --budgets ... --gpus 2` starts its own ranks; the table equals the one-rank run and the
    library's own rows."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    outs = []
    for gpus in (1, 2):
        f = str(tmp_path / f"ladder{gpus}.json")
        cmd = [sys.executable, "-m", "qldpc_amd.mc", "--code", "72", "--p", "0.05", "--trials", "30001", "--osd",
               "--budgets", "3", "10", "11", "40", "--gpus", str(gpus), "--backend", "gloo", "--share-device", "--out", f]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count("max_iter=") == 4
        outs.append(json.load(open(f)))
    assert outs[1]["world_size"] == 2 and outs[0]["budgets"] == [3, 10, 11, 40]
    code = codes.load_code("[[72, 12, 6]]")
    table = bp.decoder_for(code.Hx).mc_run_budgets(code.Lx, code.distance, 0.05, mc.prior_of(0.05, code.n),
                                                   (3, 10, 11, 40), 0, 30001, flags=_lib.FLAG_OSD0)
    for j, (a, b) in enumerate(zip(outs[0]["points"], outs[1]["points"])):
        for k in _lib.COUNTER_NAMES:
            assert a[k] == b[k] == int(table[j][_lib.COUNTER_NAMES.index(k)]), (j, k)
        assert a["max_iter"] == (3, 10, 11, 40)[j]
    res = mc.bp_per_iteration(["[[72, 12, 6]]"], 0.05, (3, 10, 11, 40), 30001)
    assert np.allclose(res["[[72, 12, 6]]"]["OSD_invocations"], table[:, 6] / 30001)
