"""The inputs of tests/test_gpu_llr_hist.py, and their tables by the numpy statement (tests/llr_hist_oracle.py), computed
once per process.  tests/test_llr_hist_cpu.py checks on the CPU that these inputs reach the interior bins, both outer
columns, the NaN column and values exactly on edges, so that the GPU comparisons cannot pass vacuously.

A case: ``H, L, distance, probs (scalar p or per column), prior, budgets, bins, (lo, hi), T, seed, kw`` (the decoder
arguments variant / alpha / damping / clip_llr)."""
import functools
from collections import namedtuple

import numpy as np

from llr_hist_oracle import dense, llr_hist
from qldpc_amd import _lib, codes, dem, mc

Case = namedtuple("Case", "H L distance probs prior budgets bins range T seed kw")
# 1, a mid value, and a last value most trials never reach
LADDER = (1, 4, 40)


def irregular37():
    """An irregular 20 x 37 matrix (row weights 1 .. 13, column weights 1 .. 7: the general-H kernel) and three
    logical rows."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.3, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1          # (no empty row)
    L = (rng.random((3, 37)) < 0.3).astype(np.uint8)
    return H, L


ZERO_COLUMNS = (5, 40)          # of [[72,12,6]] in the "zero_*" cases: no check, the posterior is the prior
ZERO_BINS, ZERO_RANGE = 20, (-10.0, 10.0)
ZERO_EDGE = 13                  # the interior edge a prior is put on: np.linspace(-10, 10, 21)[13] = 3.0


def _code72(p, **over):
    c = codes.load_code("[[72, 12, 6]]")
    d = dict(H=np.asarray(c.Hx), L=np.asarray(c.Lx), distance=c.distance, probs=p, prior=mc.prior_of(p, c.n),
             budgets=LADDER, bins=128, range=(-25.0, 25.0), T=2000, seed=5, kw={})
    d.update(over)
    return Case(**d)


def _zero_case(values):
    c = _code72(0.06, bins=ZERO_BINS, range=ZERO_RANGE, T=1500)
    H = c.H.copy()
    H[:, ZERO_COLUMNS] = 0
    prior = c.prior.copy()
    prior[list(ZERO_COLUMNS)] = values
    return c._replace(H=H, prior=prior)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "steane":
        c = codes.load_code("steane")
        return Case(np.asarray(c.Hx), np.ones((1, 7), np.uint8), 3, 0.1, mc.prior_of(0.1, 7), (1, 3, 30), 16, (-3.0, 3.0),
                    2000, 3, {})
    if name == "72":
        return _code72(0.06)
    if name == "72_minsum":         # damped min-sum
        return _code72(0.06, range=(-4.0, 8.0), kw=dict(variant=_lib.MIN_SUM, alpha=0.8, damping=0.7, clip_llr=25.0))
    if name == "zero_lo_hi":        # the two priors exactly on lo and on hi
        return _zero_case(ZERO_RANGE)
    if name == "zero_edge_lo":      # ... on an interior edge and on lo
        edge = float(np.linspace(*ZERO_RANGE, ZERO_BINS + 1)[ZERO_EDGE])
        return _zero_case((edge, ZERO_RANGE[0]))
    if name == "dem72":             # three rounds of [[72,12,6]]: row weight 8, the (8, 4) build
        H, L, probs = dem.phenomenological("[[72, 12, 6]]", 3, 0.02, 0.03)
        return Case(dense(H), np.asarray(L, np.uint8), 0, probs, mc.dem_prior(probs), (1, 5, 30), 64, (-20.0, 20.0), 1200, 2, {})
    if name in ("rand37", "rand37_minsum"):
        H, L = irregular37()
        kw = dict(variant=_lib.MIN_SUM, alpha=0.9, damping=0.8) if name.endswith("minsum") else {}
        return Case(H, L, 4, 0.05, mc.prior_of(0.05, 37), (1, 3, 20), 32, (-15.0, 15.0), 2500, 7, kw)
    if name == "inf_nan":
        # damped sum-product with damping = 1 and one prior +inf: 1 * inf + 0 * inf is NaN on that variable's edges,
        # which spreads through its checks (tests/test_extreme_priors.py); the variable's own posterior stays +inf
        c = _code72(0.06, T=800, bins=32, range=(-20.0, 20.0), kw=dict(variant=_lib.DAMPED_SP, alpha=1.0, damping=1.0))
        prior = c.prior.copy()
        prior[17] = np.inf
        return c._replace(prior=prior)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def statement(name, bins=None, llr_range=None, budgets=None):
    """The table of a case by the numpy statement (other bins / range / budgets on request)."""
    c = case(name)
    lo, hi = llr_range or c.range
    return llr_hist(c.H, c.probs if np.ndim(c.probs) == 0 else np.asarray(c.probs), c.prior, 0, c.T, budgets or c.budgets,
                    bins or c.bins, lo, hi, seed=c.seed, **c.kw)
