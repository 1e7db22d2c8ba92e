"""GPU: qbp_mc_run_enum under the second stages and first-stage builds that act on stored rows -- Relay-BP, BP guided
decimation, localized statistics decoding, layered BP and fixed-point min-sum, each configured as its own test file
configures it -- against qbp_mc_run_errors with the same flags on the oracle's rows.  [[72,12,6]], weight 3, all 59 640
patterns, eight iterations of the first stage."""
import functools

import numpy as np
import pytest

import enum_oracle
import quant_cases as qc
from qldpc_amd import _lib, mc
from test_gpu_gd import config as gd_config
from test_gpu_quant import cfg_of as quant_config
from test_gpu_relay import config as relay_config
from test_gpu_weight import fresh, matrices

pytestmark = pytest.mark.gpu

W, C, MC_ITERS, ALPHA = 3, 59640, 8, 0.9
# The prior of p = 0.05: the CPU oracle's sum-product BP(8) leaves 1 824 of the 59 640 patterns unconverged (3.1 %), so
# every second stage has records to work on (tests/enum_oracle.py: kinds_of(..., max_iter=8)).
PRIOR_P = 0.05
ORACLE_UNCONVERGED = 1824


@functools.lru_cache(maxsize=None)
def rows():
    r = enum_oracle.patterns(72, W)
    r.setflags(write=False)
    return r


def configure(dec, stage):
    if stage == "relay":
        dec.relay_configure(relay_config(72, 4))
        return dict(flags=_lib.FLAG_RELAY)
    if stage == "gd":
        dec.gd_configure(gd_config(_lib.MIN_SUM, 6))
        return dict(flags=_lib.FLAG_GD)
    if stage == "lsd":
        dec.lsd_configure(1)
        return dict(flags=_lib.FLAG_LSD)
    if stage == "layered":
        dec.layered_configure(None)
        return dict(flags=_lib.FLAG_LAYERED)
    if stage == "layered_osd0":
        dec.layered_configure(None)
        return dict(flags=_lib.FLAG_LAYERED | _lib.FLAG_OSD0)
    assert stage == "quant"
    dec.quant_configure(quant_config(qc.PARAMS[1]))
    return dict(flags=_lib.FLAG_QUANT, variant=_lib.MIN_SUM)


def test_the_prior_leaves_bp_failures():
    H, L, d = matrices()["72"]
    got = fresh(H).mc_run_enum(L, d, W, mc.prior_of(PRIOR_P, 72), 0, C, max_iter=MC_ITERS)
    assert got[0] == C and got[6] == ORACLE_UNCONVERGED


@pytest.mark.parametrize("stage", ["relay", "gd", "lsd", "layered", "layered_osd0", "quant"])
def test_enum_equals_stored_errors_under_the_stage(stage):
    H, L, d = matrices()["72"]
    prior = mc.prior_of(PRIOR_P, 72)
    dec = fresh(H)
    kw = dict(max_iter=MC_ITERS, alpha=ALPHA)
    kw.update(configure(dec, stage))
    got = dec.mc_run_enum(L, d, W, prior, 0, C, **kw)
    want = dec.mc_run_errors(L, d, rows(), prior, **kw)
    print(stage, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[0] == C and got[6] > 0
    assert np.array_equal(got, want), (stage, got, want)
    a = 31111
    assert np.array_equal(dec.mc_run_enum(L, d, W, prior, 0, a, **kw) + dec.mc_run_enum(L, d, W, prior, a, C, **kw), want)
