"""GPU: the on-chip kernel on its variable-major message layout, bit for bit against the CPU oracle.

Matrices: [[72,12,6]] (m = 36: many slots per workgroup), the Steane code (rows of weight 4 and columns of degree 1 - 3
in the (6, 3) build: padding edges, short columns, the zero record), the space-time matrix of tests/golden/bp_st72.npz
((8, 4) build: four-word records, columns of weight 3 and 2 sharing zero words), an irregular (6, 3)-class matrix with an empty check and empty columns, and
the irregular matrices of bp_rand / bp_xrand (rows of weight up to 12: the general-H kernel takes them, which shares
the host tables the layout is built from -- they guard the column order it reads).  Each runs forced (the
one-barrier build where the (6, 3) build applies) and with early exit (first check step from the LDS table), for
max_iter 1, 2 and 50, on batches of 1, of S and of three rounds of every slot plus one, so that slots switch
syndromes; outputs are poisoned before every launch (geometry_util).  One Monte-Carlo call per matrix is compared
with oracle.mc_counters."""
import os

import numpy as np
import pytest

import geometry_util as gu
from oracle import oracle
from qldpc_amd import _lib, bp, codes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("[[72, 12, 6]]", "steane", "bp_st72", "irregular", "bp_rand", "bp_xrand")
GENERAL = ("bp_rand", "bp_xrand")                      # not on-chip matrices
MAX_ITERS = (1, 2, 50)
P = 0.06
SLOTS, ROUNDS = 3, 3             # the several-rounds batch: 3 slots per workgroup, one workgroup per CU, 3 rounds + 1

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def matrix(name):
    def make():
        if name == "irregular":          # the padded (6, 3)-class matrix of tests/test_gpu_geometry.py
            rng = np.random.default_rng(5)
            H = (rng.random((40, 90)) < 0.05).astype(np.int64)
            H[:, 0] = 0
            H[3] = 0
            H[3, :2] = 1
            H = H[(H.sum(1) <= 6)]
            return H[:, H.sum(0) <= 3]
        if name.startswith("bp_"):
            return np.ascontiguousarray(np.load(os.path.join(HERE, "golden", name + ".npz"))["H"]).astype(np.int64) & 1
        return np.ascontiguousarray(codes.load_code(name).Hx).astype(np.int64)
    return cached(("H", name), make)


def decoder(name):
    return cached(("dec", name), lambda: _lib.Decoder(*bp.csr_from_H(matrix(name))))


class Case:
    """The largest batch of one matrix, on the device, with one oracle run per iteration limit; the smaller batches
    are its prefixes."""

    def __init__(self, name):
        self.name, self.H, self.dec = name, matrix(name), decoder(name)
        self.m, self.n = self.H.shape
        self.num_cu = self.dec.info("num_cu")
        self.rows = ROUNDS * self.num_cu * SLOTS + 1
        rng = np.random.default_rng([11, self.m])
        self.syn = gu.syndromes_of(self.H, rng.random((self.rows, self.n)) < P)
        self.prior = np.log((1 - P) / P) * rng.uniform(0.7, 1.3, self.n)
        self.syn_t, self.prior_t = gu.to_device(self.syn), gu.to_device(self.prior)
        self.out = gu.Outputs(self.rows, self.n)
        self.refs = {}

    def oracle(self, max_iter):
        if max_iter not in self.refs:
            self.refs[max_iter] = oracle.decode_batch(self.H, self.syn, self.prior, max_iter, threads=8)
        return self.refs[max_iter]


def case(name):
    return cached(("case", name), lambda: Case(name))


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "early-exit"])
@pytest.mark.parametrize("name", NAMES)
def test_decode_bits_against_the_oracle(name, forced):
    cs = case(name)
    dec = cs.dec
    kind = 2 if name in GENERAL else 1
    assert dec.info("kernel_kind") == kind
    flags = _lib.FLAG_FORCE_FULL if forced else 0
    S_max = gu.FUSED_MAX_THREADS // cs.m                  # one full workgroup
    small = cs.H.sum(1).max() <= 6 and cs.H.sum(0).max() <= 3
    for max_iter in MAX_ITERS:
        want = cs.oracle(max_iter)
        for B, opts in ((1, {}), (S_max, dict(slots=S_max)), (cs.rows, dict(slots=SLOTS, blocks=1))):
            what = f"{name} forced={forced} max_iter={max_iter} B={B} {opts}"
            with gu.options(dec, **opts):
                got = gu.decode(dec, cs.syn_t, cs.prior_t, B, cs.out, what, max_iter=max_iter, flags=flags)
                assert dec.info("last_kernel") == kind, what
                if kind == 1:
                    assert dec.info("one_barrier") == (1 if forced and small else 0), what
                if kind == 1 and B == S_max:
                    assert dec.info("grid") == 1 and dec.info("threads") == gu.threads_of(S_max, cs.m), what
                if kind == 1 and B == cs.rows:
                    assert dec.info("grid") == cs.num_cu and B > ROUNDS * dec.info("grid") * SLOTS, what
            gu.assert_same(got, tuple(x[:B] for x in want), what)
            if name == "steane":
                assert np.isfinite(got[3]).all()          # (an unwritten word of a short column would show here first)


@pytest.mark.parametrize("name", NAMES)
def test_monte_carlo_counters_against_the_oracle(name):
    H, dec = matrix(name), decoder(name)
    n = H.shape[1]
    rng = np.random.default_rng(3)
    Lx = (rng.random((2, n)) < 0.3).astype(np.uint8)
    prior = np.full(n, np.log((1 - P) / P))
    T = 700
    got = dec.mc_run(Lx, 3, P, prior, 5, 5 + T, draws=1, seed=17, max_iter=20)
    assert dec.info("last_kernel") == (2 if name in GENERAL else 1)
    want = oracle.mc_counters(H, Lx, 3, P, prior, 5, 5 + T, draws=1, seed=17, max_iter=20)
    assert np.array_equal(got, want), dict(zip(_lib.COUNTER_NAMES, zip(got.tolist(), want.tolist())))
