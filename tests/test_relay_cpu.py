"""CPU: the statement of Relay-BP (tests/relay_oracle.py) anchored to the reference's min-sum, the gamma tables, the
Python argument checks and the C ABI without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import relay_oracle as ro
from oracle import oracle
from qldpc_amd import _lib, codes, mc, relay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def irregular37():
    """An irregular 20 x 37 matrix (row weights 1 .. 13, column weights 1 .. 7: long rows and long columns)."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.3, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1          # (no empty row)
    return H


# ---- 1. gammas = 0, one leg, stop_after = 1: performMinSum_Symmetric with damping = 1.0 ----------------------------------
@pytest.mark.parametrize("name", ["72", "rand37"])
@pytest.mark.parametrize("alpha", [1.0, 0.8])
def test_statement_is_the_references_min_sum_without_memory(name, alpha):
    H = np.asarray(codes.load_code("[[72, 12, 6]]").Hx if name == "72" else irregular37())
    n = H.shape[1]
    errors = (np.random.default_rng(5).random((300, n)) < 0.05).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log(0.95 / 0.05))
    hard, conv, iters, llr = oracle.decode_batch(H, syn, prior, 30, variant=2, alpha=alpha, damping=1.0)
    r = ro.relay_decode_batch(H, syn, prior, np.zeros((1, n)), [30], stop_after=1, alpha=alpha)
    assert 20 < conv.sum() < 300                            # (both outcomes present)
    assert np.array_equal(r["hard"], hard) and np.array_equal(r["converged"], conv)
    assert np.array_equal(r["iters"] - 1, iters)
    assert ro.same(r["llr"], llr)
    assert np.all(r["legs"] == 1) and np.array_equal(r["solutions"], conv.astype(np.int32))
    one = ro.relay_decode(H, syn[7], prior, np.zeros((1, n)), [30], alpha=alpha)
    assert np.array_equal(one["hard"], hard[7]) and one["iters"] - 1 == iters[7]


def test_statement_legs_carry_messages_and_keep_the_lightest():
    """Two legs of T iterations with equal gammas are one leg of 2 T for a record that never converges; a record solved
    in leg 0 with stop_after = 1 never enters leg 1."""
    H = np.asarray(codes.load_code("[[72, 12, 6]]").Hx)
    n = H.shape[1]
    errors = (np.random.default_rng(9).random((200, n)) < 0.1).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log(0.9 / 0.1))
    g = np.full((2, n), 0.125)
    two = ro.relay_decode_batch(H, syn, prior, g, [6, 6], stop_after=1, alpha=0.9)
    one = ro.relay_decode_batch(H, syn, prior, g[:1], [12], stop_after=1, alpha=0.9)
    assert ro.same(two["llr"], one["llr"]) and np.array_equal(two["iters"], one["iters"])
    assert np.array_equal(two["legs"], np.where(one["iters"] > 6, 2, 1))
    assert (~one["converged"]).sum() > 0 and np.all(one["iters"][~one["converged"]] == 12)
    many = ro.relay_decode_batch(H, syn, prior, relay.relay_gammas(n, 5, 0.125, (-0.24, 0.66), 3), [12] * 5, 2, alpha=0.9)
    c = ro.classes(many)
    assert c["leg0"] > 0 and c["later"] > 0
    ok = many["converged"]
    assert np.array_equal((many["hard"][ok].astype(np.int64) @ H.T % 2), syn[ok])
    assert np.all(many["solutions"] <= 2) and np.all(many["best_leg"][~ok] == -1)


# ---- 2. the gamma tables -----------------------------------------------------------------------------------------------
def test_relay_gammas_is_reproducible():
    a = relay.relay_gammas(72, 5, 0.125, (-0.24, 0.66), 11)
    b = relay.relay_gammas(72, 5, 0.125, (-0.24, 0.66), 11)
    assert a.shape == (5, 72) and a.dtype == np.float64 and np.array_equal(a, b)
    assert np.all(a[0] == 0.125) and np.all((a[1:] >= -0.24) & (a[1:] <= 0.66)) and a[1:].min() < 0 < a[1:].max()
    assert not np.array_equal(a, relay.relay_gammas(72, 5, 0.125, (-0.24, 0.66), 12))
    # the stated draw: leg by leg from default_rng(seed)
    rng = np.random.default_rng(11)
    assert np.array_equal(a[1], rng.uniform(-0.24, 0.66, 72)) and np.array_equal(a[2], rng.uniform(-0.24, 0.66, 72))
    assert np.array_equal(relay.relay_gammas(7, 1, 0.3, (0, 1), 0), np.full((1, 7), 0.3))
    for bad in ((0, 5, 0.1, (0, 1)), (7, 0, 0.1, (0, 1)), (7, 2, np.nan, (0, 1)), (7, 2, 0.1, (1, 0)),
                (7, 2, 0.1, (0, np.inf))):
        with pytest.raises(ValueError):
            relay.relay_gammas(*bad)


def test_configuration_checks_raise_before_the_library():
    g = relay.relay_gammas(7, 3, 0.1, (0, 1), 0)
    cfg = relay.RelayConfig(g, [4, 5, 6], stop_after=2, alpha=0.9)
    assert cfg.leg_iters.dtype == np.int32 and cfg.n == 7 and cfg.stop_after == 2
    for args in ((g, [4, 5]), (g, [4, 0, 6]), (g, [4.5, 5, 6]), (g[0], [4]), (np.where(g > 0.5, np.nan, g), [4, 5, 6])):
        with pytest.raises(ValueError):
            relay.RelayConfig(*args)
    for kw in (dict(stop_after=0), dict(stop_after=1.5), dict(alpha=np.inf), dict(clip_llr=np.nan)):
        with pytest.raises(ValueError):
            relay.RelayConfig(g, [4, 5, 6], **kw)
    assert relay.as_config(cfg, 7) is cfg
    d = relay.as_config(dict(legs=3, iters=4, gamma0=0.1, interval=(0, 1), seed=0, stop_after=2), 7)
    assert np.array_equal(d.gammas, g) and d.leg_iters.tolist() == [4, 4, 4] and d.stop_after == 2
    with pytest.raises(ValueError):
        relay.as_config(cfg, 8)
    with pytest.raises(ValueError):
        relay.as_config(dict(legs=3, iters=4, gamma0=0.1, interval=(0, 1), typo=1), 7)
    with pytest.raises(ValueError):
        relay.as_config([g], 7)


def _never(*a):
    raise AssertionError("the runner must not be reached")


def test_relay_and_osd_exclude_each_other_before_any_device_work():
    assert mc.relay_run_flags(0, None) == 0 and mc.relay_run_flags(_lib.FLAG_OSD0, None) == _lib.FLAG_OSD0
    assert mc.relay_run_flags(0, {}) == _lib.FLAG_RELAY == 512
    cfg = dict(legs=2, iters=3, gamma0=0.1, interval=(0, 1))
    code = codes.load_code("[[72, 12, 6]]")
    with pytest.raises(ValueError):
        mc.run_sweep("[[72, 12, 6]]", [0.05], 100, osd=True, relay=cfg, runner=_never)
    with pytest.raises(ValueError):
        mc.run_dem(code.Hx, code.Lx, np.full(72, 0.05), 100, osd=True, osd_order=3, relay=cfg, runner=_never)
    with pytest.raises(ValueError):
        mc.run_weights("[[72, 12, 6]]", [3], 100, prior_p=0.01, osd=True, relay=cfg, runner=_never)


@pytest.mark.parametrize("argv", [["--relay", "5", "12", "--osd"], ["--relay", "5", "12", "--budgets", "10", "20"],
                                  ["--relay", "5", "12", "--spectrum", "x.npz"], ["--relay", "0", "12"],
                                  ["--relay", "5", "0"], ["--relay", "5", "12", "--relay-stop", "0"],
                                  ["--relay", "5", "12", "--relay-interval", "1", "0"]])
def test_cli_refuses_bad_relay_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05"] + argv)
    assert e.value.code == 2
    assert "--relay" in capsys.readouterr().err


# ---- 3. the C ABI without a device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    return _lib.load()


def test_null_handle_is_invalid(lib):
    g = np.zeros((1, 4))
    it = np.ones(1, np.int32)
    syn = np.zeros((2, 3), np.uint8)
    prior = np.zeros(4)
    hard = np.full((2, 4), 7, np.uint8)
    assert lib.qbp_relay_configure(None, g.ctypes.data, 1, it.ctypes.data, 1, 1.0, 20.0) == -1
    assert b"null handle" in lib.qbp_last_error()
    args = (None, syn.ctypes.data, prior.ctypes.data, 2, hard.ctypes.data, None, None, None, None, None)
    assert lib.qbp_relay_decode_batch(*args) == -1
    assert lib.qbp_relay_decode_batch_device(*args, None) == -1
    assert np.all(hard == 7)


def test_header_binding_and_library_agree(lib):
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for name, nargs in (("qbp_relay_configure", 7), ("qbp_relay_decode_batch", 10), ("qbp_relay_decode_batch_device", 11)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is not None
        assert hasattr(lib, name), name
    m = re.search(r"\bQBP_FLAG_RELAY\s*=\s*(\d+)u", header)
    assert m and int(m.group(1)) == _lib.FLAG_RELAY == 512
    src = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp.hip")).read()
    for name in ("qbp_relay_configure", "qbp_relay_decode_batch", "qbp_relay_decode_batch_device"):
        assert re.search(rf"^int {name}\([^)]*\)\ntry \{{", src, re.M), name      # (no exception crosses the ABI)
