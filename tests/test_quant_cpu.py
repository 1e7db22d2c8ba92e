"""No GPU: the numpy statement of fixed-point min-sum (tests/quant_oracle.py) against the reference-generated min-sum
goldens and ``oracle.decode_batch``, ``quant.quantize_prior`` (rule 1), its edge-indexed twin against it, and the record
classes of the test inputs."""
import numpy as np
import pytest

import golden_util
import quant_cases as qc
import quant_oracle as qo
from oracle import oracle
from qldpc_amd import quant


# ---- rule 1 -------------------------------------------------------------------------------------------------------------
def test_quantize_prior_rounds_half_to_even_and_clamps():
    cfg = quant.QuantConfig(6, 2.0)                     # M = 31
    x = np.array([0.25, 0.75, 1.25, -0.25, -0.75, -1.25, 0.0, -0.0, 15.5, 15.75, 16.0, 1e300, -15.75, -1e300,
                  np.inf, -np.inf, np.nan, 1.2, -1.3])
    want = np.array([0, 2, 2, 0, -2, -2, 0, 0, 31, 31, 31, 31, -31, -31, 31, -31, 0, 2, -3], np.int32)
    got = quant.quantize_prior(x, cfg)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(qo.quantize(x, 6, 2.0), want)
    # the product is one double multiply: 0.1 * 3.0 = 0.30000000000000004, and 2.5 / 4.5 are exact ties
    assert quant.quantize_prior([2.5, 3.5, 4.5, -2.5], quant.QuantConfig(8, 1.0)).tolist() == [2, 4, 4, -2]
    for bits, scale in ((2, 0.5), (4, 1.0), (8, 8.0), (16, 64.0)):
        rng = np.random.default_rng(bits)
        y = np.concatenate([rng.normal(0, 3, 500), rng.integers(-40, 40, 200) / 2.0 / scale, [np.inf, -np.inf, np.nan]])
        got = quant.quantize_prior(y, quant.QuantConfig(bits, scale))
        assert np.array_equal(got, qo.quantize(y, bits, scale))
        assert np.abs(got).max() <= qo.M_of(bits)


def test_config_refuses_what_the_library_refuses():
    for kw in (dict(bits=1, scale=1.0), dict(bits=17, scale=1.0), dict(bits=4, scale=0.0), dict(bits=4, scale=np.inf),
               dict(bits=4, scale=np.nan), dict(bits=4, scale=-1.0), dict(bits=4, scale=1.0, alpha=(0, 2)),
               dict(bits=4, scale=1.0, alpha=(5, 2)), dict(bits=4, scale=1.0, alpha=(1, 16)),
               dict(bits=4, scale=1.0, alpha=(1, -1)), dict(bits=4, scale=1.0, beta=8), dict(bits=4, scale=1.0, beta=-1),
               dict(bits=True, scale=1.0), dict(bits=4.5, scale=1.0)):
        with pytest.raises(ValueError):
            quant.QuantConfig(**kw)
    cfg = quant.as_config(dict(bits=16, scale=64.0, alpha=(7, 3)))
    assert cfg.M == 32767 and cfg.alpha == (7, 3) and cfg.beta == 0
    assert quant.QuantConfig(2, 1.0).M == 1 and quant.QuantConfig(4, 1.0, (4, 2), 7).beta == 7


# ---- the statement against the reference --------------------------------------------------------------------------------
def test_first_iteration_equals_the_min_sum_goldens():
    """The goldens of performMinSum_Symmetric at its defaults (alpha 1, damping 1, clip 20) have a uniform prior L.  With
    scale 1 / L every P is 1, and iteration 0 of both decoders computes V = L * (1 + a sum of +-1): the reference's
    partial sums are 0, +-L, +-2L, 3L or 4L on columns of weight <= 3, exact where the sum is zero, so the hard decision
    of iteration 0 is derivable -- which records converge there, and to what.  Later iterations are not: the reference
    clips at 20, no multiple of L."""
    seen = 0
    for tag in ("steane", "72", "144"):
        for c in golden_util.load(tag):
            if c["fn"] != "minsum" or c["alpha"] != 1.0 or c["damping"] != 1.0:
                continue
            L = float(c["prior"][0])
            assert np.all(c["prior"] == L) and (c["H"] != 0).sum(axis=0).max() <= 3
            hard, conv, iters, V, llr = qo.decode_batch(c["H"], c["syndromes"], c["prior"], 1, 16, 1.0 / L, 1, 0, 0)
            at0 = c["converged"] & (c["iters"] == 0)
            assert np.array_equal(conv, at0), (tag, c["key"])
            assert np.array_equal(hard[at0], c["hard"][at0])
            seen += int(at0.sum())
    assert seen >= 20


@pytest.fixture(scope="module")
def integer_case():
    """60 records on [[72,12,6]] with integer priors from {2..5}: the cross-check of the issue."""
    H = qc.matrix("72")
    rng = np.random.default_rng(11)
    errors = (rng.random((60, 72)) < 0.08).astype(np.uint8)
    prior = rng.integers(2, 6, 72).astype(np.float64)
    return H, qc.syndromes_of(H, errors), prior


def test_integer_priors_equal_the_references_min_sum(integer_case):
    """q = 16, scale 1, alpha 1 / 1, beta 0 on integer priors: every quantity of the reference's
    performMinSum_Symmetric(alpha=1, damping=1, clip_llr=32767) is an integer below 2^53, so its doubles are exact and
    equal the statement's integers -- hard decision, converged flag, iteration and values."""
    H, syn, prior = integer_case
    hard, conv, iters, V, llr = qo.decode_batch(H, syn, prior, 30, 16, 1.0, 1, 0, 0)
    o_hard, o_conv, o_iters, o_llr = oracle.decode_batch(H, syn, prior, 30, 2, 1.0, 1.0, 32767.0)
    counts = qc.classes(conv, iters)
    print("classes", counts)
    assert min(counts) >= 4
    assert np.array_equal(hard, o_hard) and np.array_equal(conv, o_conv.astype(bool)) and np.array_equal(iters, o_iters)
    assert np.array_equal(llr, o_llr) and np.array_equal(V, llr.astype(np.int32))


# ---- the edge-indexed twin of the statement ---------------------------------------------------------------------------------
def assert_twin(got, want, what):
    assert len(got) == len(want) == 5
    for k, x, y in zip(("hard", "converged", "iters", "posterior_q", "llr"), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint64) if k == "llr" else x, y.view(np.uint64) if k == "llr" else y), (what, k)


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("name", qc.MATRICES)
def test_edge_indexed_twin_equals_the_dense_statement(name, kind):
    """decode_batch_edges against decode_batch in all five outputs, on every (name, kind, params, max_iter) the GPU tests
    of the small matrices use: weight-0 and weight-1 rows, empty columns, +-inf priors and the unsatisfiable empty
    check included."""
    H, _, syn, prior = qc.case(name, kind)
    for params in qc.PARAMS:
        for max_iter in qc.MAX_ITERS:
            got = qo.decode_batch_edges(H, syn, prior, max_iter, *params)
            assert_twin(got, qc.statement(name, kind, params, max_iter), f"{name} {kind} {params} max_iter {max_iter}")


def test_edge_indexed_twin_equals_the_dense_statement_on_the_issue_records():
    H, _, syn, prior = qc.issue_case()
    nan = prior.copy(); nan[9] = np.nan
    for params in qc.PARAMS:
        assert_twin(qo.decode_batch_edges(H, syn, prior, 30, *params), qo.decode_batch(H, syn, prior, 30, *params), params)
    assert_twin(qo.decode_batch_edges(H, syn, nan, 30, *qc.PARAMS[2]), qo.decode_batch(H, syn, nan, 30, *qc.PARAMS[2]), "NaN")


# ---- the test inputs hold every record class ------------------------------------------------------------------------------
@pytest.mark.parametrize("params", qc.PARAMS, ids=lambda p: f"q{p[0]}")
def test_issue_records_hold_every_class(params):
    H, _, syn, prior = qc.issue_case()
    hard, conv, iters, V, llr = qo.decode_batch(H, syn, prior, 30, *params)
    at0, later, never = qc.classes(conv, iters)
    print(params, at0, later, never)
    assert 2 <= at0 <= 5 and 15 <= later <= 28 and 9 <= never <= 22
    assert np.array_equal((V < 0).astype(np.uint8), hard) and np.array_equal(llr, V.astype(np.float64))
    ok = (qc.syndromes_of(H, hard) == syn).all(axis=1)
    assert np.array_equal(ok, conv)


def test_gpu_records_hold_saturation_zero_posteriors_and_every_class():
    sat = zero = 0
    for name in ("72", "irr37", "rows"):
        for kind in ("uniform", "mixed"):
            total = np.zeros(3, int)
            for params in qc.PARAMS:
                hard, conv, iters, V, _ = qc.statement(name, kind, params, 30)
                total += qc.classes(conv, iters)
                M = qo.M_of(params[0])
                sat += int((np.abs(V) > M).any(axis=1).sum())           # a posterior beyond M: its messages clamp
                zero += int((V == 0).any(axis=1).sum())
            print(name, kind, total)
            assert total.min() >= 2, (name, kind, total)
    assert sat >= 8 and zero >= 8
