"""GPU: the on-chip sum-product kernels after the second instruction diet of the check update (reciprocal-table
offsets by byte select, the one-barrier build's iteration index a scalar, full division on the rare path) against the CPU
oracle: hard decision, converged flag, iteration and every LLR bit.

Forced launches of these codes run the one-barrier build (the headline kernel of bench.py), early-exit launches the
two-barrier build of the same headers.  max_iter 1, 2, 3 and 50: both parities of the loop unrolled by two, and a
syndrome whose last iteration is its first.  The slot-turnover cases pin the launch geometry (slots per workgroup,
one workgroup per CU) and size the batch to at least three syndromes per slot of every workgroup launched, so that
the scalar iteration index and the last-iteration settle are exercised across a change of syndrome.
"""
import numpy as np
import pytest

import golden_util
from oracle import oracle
from qldpc_amd import _lib, bp, codes

pytestmark = pytest.mark.gpu

CODES = ["[[72, 12, 6]]", "[[288, 12, 18]]"]
MAX_ITERS = (1, 2, 3, 50)
_ORACLE = {}


def _batch(name, p, B, seed):
    code = codes.load_code(name)
    rng = np.random.default_rng([seed, code.n, int(p * 1e6), B])
    errors = (rng.random((B, code.n)) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ code.Hx.T % 2).astype(np.uint8)
    return code, syn, np.full(code.n, np.log((1 - p) / p))


def _oracle(key, H, syn, prior, max_iter):
    """one oracle run per (batch, limit), shared by the forced and early-exit cases"""
    k = (key, max_iter)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.decode_batch(H, syn, prior, max_iter, threads=8)
    return _ORACLE[k]


def _same(got, want, what):
    hard, conv, iters, llr = got
    o_hard, o_conv, o_iters, o_llr = want
    assert np.array_equal(conv, o_conv), what
    assert np.array_equal(iters, o_iters), what
    assert np.array_equal(hard, o_hard), what
    bad = ~golden_util.same_bits(llr, o_llr)
    assert not bad.any(), f"{what}: {int(bad.sum())} LLRs differ in bits, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "early-exit"])
@pytest.mark.parametrize("p", [0.01, 0.10])
@pytest.mark.parametrize("name", CODES)
def test_64_syndromes_against_the_oracle(name, p, forced):
    code, syn, prior = _batch(name, p, 64, 1)
    dec = bp.decoder_for(code.Hx)
    assert dec.info("kernel_kind") == 1
    for max_iter in MAX_ITERS:
        got = dec.decode(syn, prior, max_iter, flags=_lib.FLAG_FORCE_FULL if forced else 0)
        assert dec.info("one_barrier") == (1 if forced else 0)
        _same(got, _oracle((name, p, 64), code.Hx, syn, prior, max_iter), (name, p, forced, max_iter))


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "early-exit"])
@pytest.mark.parametrize("name,slots,p", [("[[72, 12, 6]]", 5, 0.10), ("[[288, 12, 18]]", 3, 0.10),
                                          ("[[288, 12, 18]]", 2, 0.01)])
def test_several_syndromes_per_slot(name, slots, p, forced):
    code = codes.load_code(name)
    dec = bp.decoder_for(code.Hx)
    per_slot = 3
    B = per_slot * slots * dec.info("num_cu") + 7          # (+ 7: the last round leaves slots idle)
    code, syn, prior = _batch(name, p, B, 2)
    dec.set_option(_lib.OPT_SLOTS_PER_BLOCK, slots)
    dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
    try:
        for max_iter in MAX_ITERS:
            got = dec.decode(syn, prior, max_iter, flags=_lib.FLAG_FORCE_FULL if forced else 0)
            assert dec.info("one_barrier") == (1 if forced else 0)
            grid = dec.info("grid")
            assert B >= per_slot * slots * grid, (B, slots, grid)
            _same(got, _oracle((name, p, B), code.Hx, syn, prior, max_iter), (name, p, forced, max_iter, grid))
    finally:
        dec.set_option(_lib.OPT_SLOTS_PER_BLOCK, 0)
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "early-exit"])
@pytest.mark.parametrize("name", ["[[72, 12, 6]]", "steane"])
def test_extreme_priors(name, forced):
    """A prior vector with a subnormal, 1e-300, 700.0 (tanh's clamp and constant row) and a zero among ordinary
    values; on the Steane code (rows of weight 4 in the (6, 3) shape) the kernel's own +inf padding priors sit
    beside them in every row."""
    code = codes.load_code(name)
    H = code.Hx
    n = H.shape[1]
    rng = np.random.default_rng(6)
    p = 0.08
    B = 64
    syn = ((rng.random((B, n)) < p).astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.log((1 - p) / p) * rng.uniform(0.5, 1.5, n)
    prior[[0, 1, 2, 3]] = [5e-324 * 1000, 1e-300, 700.0, 0.0]
    if n > 8:
        prior[[n - 1, n - 2, n - 3]] = [-2.5e-310, -1e-300, 2.2250738585072014e-308]
    dec = bp.decoder_for(H)
    assert dec.info("kernel_kind") == 1
    for max_iter in MAX_ITERS:
        got = dec.decode(syn, prior, max_iter, flags=_lib.FLAG_FORCE_FULL if forced else 0)
        assert dec.info("one_barrier") == (1 if forced else 0)
        _same(got, _oracle((name, "extreme"), H, syn, prior, max_iter), (name, forced, max_iter))
