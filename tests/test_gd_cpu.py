"""CPU: the statement of BP guided decimation (tests/gd_oracle.py) anchored to the reference's decoders, its decimation
rule on hand-checked cases, the Python argument checks and the C ABI without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import gd_oracle as go
from oracle import oracle
from qldpc_amd import _lib, codes, gd, mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]], np.uint8)


def irregular37():
    """An irregular 20 x 37 matrix (row weights 1 .. 13, column weights 1 .. 7: long rows and long columns)."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.3, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1          # (no empty row)
    return H


def syndromes_of(H, p, seed, B):
    errors = (np.random.default_rng(seed).random((B, H.shape[1])) < p).astype(np.uint8)
    return (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)


# ---- 1. max_rounds = 0: the reference's decoders ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72", "rand37"])
@pytest.mark.parametrize("variant,alpha", [(go.SUM_PRODUCT, 1.0), (go.MIN_SUM, 1.0), (go.MIN_SUM, 0.8)])
def test_statement_without_decimation_is_the_references_decoder(name, variant, alpha):
    H = np.asarray(codes.load_code("[[72, 12, 6]]").Hx if name == "72" else irregular37())
    n = H.shape[1]
    syn = syndromes_of(H, 0.05, 5, 300)
    prior = np.full(n, np.log(0.95 / 0.05))
    hard, conv, iters, llr = oracle.decode_batch(H, syn, prior, 30, variant=variant, alpha=alpha, damping=1.0)
    r = go.gd_decode_batch(H, syn, prior, 30, 0, 25.0, variant, alpha=alpha)
    assert 20 < conv.sum() < 300                            # (both outcomes present)
    assert np.array_equal(r["hard"], hard) and np.array_equal(r["converged"], conv)
    assert np.array_equal(r["iters"], np.where(conv, iters + 1, 30))
    assert go.same(r["llr"], llr)
    assert np.all(r["rounds"] == 0) and np.all(r["cls"][~conv] == 2) and np.all(r["cls"][conv] == 0)
    one = go.gd_decode(H, syn[7], prior, 30, 0, 25.0, variant, alpha=alpha)
    assert np.array_equal(one["hard"], hard[7]) and go.same(one["llr"], llr[7])


# ---- 2. the decimation rule -------------------------------------------------------------------------------------------------
def test_decimation_on_steane_by_hand():
    """Min-sum, alpha = 1, one iteration per round, syndrome (1, 0, 0).  Rows {3,4,5,6}, {1,2,5,6}, {0,2,4,6}; all priors
    positive, so R[c, j] = syndrome sign * the smallest prior of the row's other variables.
    P = (1,2,3,9,5,6,7): R0 = (-5,-6,-5,-5), R1 = (3,2,2,2), R2 = (3,1,1,1), V = (4,5,6,4,0,3,5): no solution (hard = 0),
    variable 2 has the largest |V| and is frozen at +25.
    P = (1,2,2,9,5,6,7): R1 = (2,2,2,2), R2 = (2,1,1,1), V = (3,4,5,4,0,3,5): variables 2 and 6 tie at 5, the lower wins."""
    s = np.array([1, 0, 0], np.uint8)
    for P, V1 in (([1, 2, 3, 9, 5, 6, 7], [4, 5, 6, 4, 0, 3, 5]), ([1, 2, 2, 9, 5, 6, 7], [3, 4, 5, 4, 0, 3, 5])):
        P = np.array(P, np.float64)
        r0 = go.gd_decode(STEANE, s, P, 1, 0, 25.0, go.MIN_SUM)
        assert np.array_equal(r0["llr"], np.array(V1, np.float64)) and not r0["converged"] and r0["iters"] == 1
        r1 = go.gd_decode(STEANE, s, P, 1, 1, 25.0, go.MIN_SUM)
        assert r1["rounds"] == 1 and r1["iters"] == 2
        assert np.flatnonzero(r1["decimated"]).tolist() == [2]
        want_w = P.copy()
        want_w[2] = 25.0
        assert np.array_equal(r1["working_prior"], want_w)


def test_sign_of_the_frozen_prior_follows_the_posterior():
    """Uniform priors freeze a variable at + (the most reliable posterior agrees with the prior); a prior that is sure
    of a flip on variable 5 freezes that one at -."""
    H = np.asarray(codes.load_code("[[72, 12, 6]]").Hx)
    syn = syndromes_of(H, 0.1, 1, 256)
    uniform = np.full(72, np.log(0.9 / 0.1))
    flipped = uniform.copy()
    flipped[5] = -12.0
    signs = set()
    for prior in (uniform, flipped):
        before = go.gd_decode_batch(H, syn, prior, 8, 0, 25.0, go.MIN_SUM, alpha=0.9)
        after = go.gd_decode_batch(H, syn, prior, 8, 1, 25.0, go.MIN_SUM, alpha=0.9)
        assert (after["rounds"] == 1).sum() >= 8
        for b in np.flatnonzero(after["rounds"] == 1):
            v = np.flatnonzero(after["decimated"][b])
            assert len(v) == 1 and v[0] == go.choose(before["llr"][b], np.zeros(72, bool), H.sum(0))
            neg = before["llr"][b, v[0]] < 0
            assert after["working_prior"][b, v[0]] == (-25.0 if neg else 25.0)
            assert np.array_equal(np.delete(after["working_prior"][b], v[0]), np.delete(prior, v[0]))
            signs.add(bool(neg))
        assert np.array_equal(after["rounds"] == 0, before["converged"])
    assert signs == {True, False}


def test_choose_skips_nan_zero_columns_and_decimated():
    w = np.array([1, 1, 0, 1, 1])
    assert go.choose([1.0, -3.0, 9.0, 3.0, np.nan], np.zeros(5, bool), w) == 1         # tie |3|: the lower; 9 is isolated
    assert go.choose([1.0, -3.0, 9.0, 3.0, np.nan], np.array([0, 1, 0, 0, 0], bool), w) == 3
    assert go.choose([np.nan, np.nan, 9.0, np.nan, np.nan], np.zeros(5, bool), w) == -1
    assert go.choose([0.0, -0.0, 9.0, 0.0, 0.0], np.zeros(5, bool), w) == 0
    assert go.choose([1.0, np.inf, 9.0, -np.inf, 0.0], np.zeros(5, bool), w) == 1


def test_nan_posteriors_and_zero_columns_are_never_frozen():
    """The 20 x 37 matrix has rows of weight 1, whose min-sum message is infinite: posteriors turn NaN.  Two all-zero
    columns appended to [[72,12,6]] are isolated variables."""
    H = irregular37()
    assert (H.sum(1) == 1).any()
    prior = np.full(37, np.log(0.9 / 0.1))
    r = go.gd_decode_batch(H, syndromes_of(H, 0.1, 2, 64), prior, 4, 37, 25.0, go.MIN_SUM, alpha=0.9)
    stuck = ~r["converged"]
    assert stuck.sum() >= 8 and np.isnan(r["llr"][stuck]).any()
    # candidates ran out before max_rounds: everything left is NaN
    short = stuck & (r["rounds"] < 37)
    assert short.any()
    assert np.all(np.isnan(r["llr"][short]) | r["decimated"][short])
    H74 = np.concatenate([np.asarray(codes.load_code("[[72, 12, 6]]").Hx), np.zeros((36, 2), np.uint8)], axis=1)
    prior = np.concatenate([np.full(72, np.log(0.9 / 0.1)), [50.0, -60.0]])      # (the largest |prior| by far)
    r = go.gd_decode_batch(H74, syndromes_of(H74, 0.1, 1, 64), prior, 8, 74, 25.0, go.MIN_SUM, alpha=0.9)
    assert (r["rounds"] > 0).sum() >= 8 and not r["decimated"][:, 72:].any()
    assert np.all(r["llr"][:, 72] == 50.0) and np.all(r["llr"][:, 73] == -60.0) and np.all(r["rounds"] <= 72)


# ---- 3. the Python argument checks ----------------------------------------------------------------------------------------
def test_gdconfig_validation():
    c = gd.GDConfig(8, 72, 25.0, gd.MIN_SUM, 0.9, 20.0)
    assert (c.iters_per_round, c.max_rounds, c.decim_llr, c.variant, c.alpha, c.clip_llr) == (8, 72, 25.0, 2, 0.9, 20.0)
    assert gd.GDConfig(1, 0).max_rounds == 0 and gd.GDConfig(variant=gd.SUM_PRODUCT).variant == 0
    for kw in (dict(iters_per_round=0), dict(iters_per_round=2.5), dict(iters_per_round=True), dict(max_rounds=-1),
               dict(max_rounds=1.5), dict(decim_llr=0.0), dict(decim_llr=-1.0), dict(decim_llr=np.inf),
               dict(decim_llr=np.nan), dict(variant=1), dict(variant=3), dict(alpha=np.nan), dict(clip_llr=np.inf),
               dict(iters_per_round=1 << 31)):
        with pytest.raises(ValueError):
            gd.GDConfig(**kw)
    assert gd.as_config(c) is c
    d = gd.as_config(dict(iters_per_round=4, max_rounds=3, decim_llr=30.0))
    assert (d.iters_per_round, d.max_rounds, d.decim_llr, d.variant) == (4, 3, 30.0, gd.MIN_SUM)
    for bad in (dict(typo=1), [c], None, dict(max_rounds=-2)):
        with pytest.raises(ValueError):
            gd.as_config(bad)


def _never(*a):
    raise AssertionError("the runner must not be reached")


def test_gd_excludes_osd_and_relay_before_any_device_work():
    assert mc.gd_run_flags(0, None) == 0 and mc.gd_run_flags(_lib.FLAG_LAYERED, {}) == _lib.FLAG_LAYERED | _lib.FLAG_GD
    assert _lib.FLAG_GD == 2048
    cfg = dict(iters_per_round=8, max_rounds=6)
    rel = dict(legs=2, iters=3, gamma0=0.1, interval=(0, 1))
    code = codes.load_code("[[72, 12, 6]]")
    for extra in (dict(osd=True), dict(osd=True, osd_order=3), dict(relay=rel)):
        with pytest.raises(ValueError):
            mc.run_sweep("[[72, 12, 6]]", [0.05], 100, gd=cfg, runner=_never, **extra)
        with pytest.raises(ValueError):
            mc.run_dem(code.Hx, code.Lx, np.full(72, 0.05), 100, gd=cfg, runner=_never, **extra)
        with pytest.raises(ValueError):
            mc.run_weights("[[72, 12, 6]]", [3], 100, prior_p=0.01, gd=cfg, runner=_never, **extra)
    with pytest.raises(ValueError):
        mc.run_sweep("[[72, 12, 6]]", [0.05], 100, gd=dict(iters_per_round=0), runner=_never)
    # with an injected runner the argument is accepted and the runner decides
    got = mc.run_sweep("[[72, 12, 6]]", [0.05], 100, gd=cfg, runner=lambda code, p, a, b: np.arange(12))
    assert np.array_equal(got[0], np.arange(12))


@pytest.mark.parametrize("argv", [["--gd", "8", "6", "--osd"], ["--gd", "8", "6", "--relay", "5", "12"],
                                  ["--gd", "8", "6", "--budgets", "10", "20"], ["--gd", "8", "6", "--spectrum", "x.npz"],
                                  ["--gd", "8", "6", "--shots", "x.npz"], ["--gd", "0", "6"], ["--gd", "8", "-1"],
                                  ["--gd", "8", "6", "--gd-llr", "0"]])
def test_cli_refuses_bad_gd_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05"] + argv)
    assert e.value.code == 2
    assert "--gd" in capsys.readouterr().err


# ---- 4. the C ABI without a device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    return _lib.load()


def test_null_handle_is_invalid(lib):
    syn = np.zeros((2, 3), np.uint8)
    prior = np.zeros(4)
    hard = np.full((2, 4), 7, np.uint8)
    assert lib.qbp_gd_configure(None, 8, 6, 25.0, 2, 1.0, 20.0) == -1
    assert b"null handle" in lib.qbp_last_error()
    args = (None, syn.ctypes.data, prior.ctypes.data, 2, hard.ctypes.data, None, None, None, None)
    assert lib.qbp_gd_decode_batch(*args) == -1
    assert lib.qbp_gd_decode_batch_device(*args, None) == -1
    assert np.all(hard == 7)


def test_header_binding_and_library_agree(lib):
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for name, nargs in (("qbp_gd_configure", 7), ("qbp_gd_decode_batch", 9), ("qbp_gd_decode_batch_device", 10)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is not None
        assert hasattr(lib, name), name
    m = re.search(r"\bQBP_FLAG_GD\s*=\s*(\d+)u", header)
    assert m and int(m.group(1)) == _lib.FLAG_GD == 2048
    src = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp.hip")).read()
    for name in ("qbp_gd_configure", "qbp_gd_decode_batch", "qbp_gd_decode_batch_device"):
        assert re.search(rf"^int {name}\([^)]*\)\ntry \{{", src, re.M), name      # (no exception crosses the ABI)
