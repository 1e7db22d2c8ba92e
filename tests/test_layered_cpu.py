"""CPU: the statement of layered BP (tests/layered_oracle.py) in its two forms, the host-only plan of the C ABI against
the numpy colouring, and every refusal that needs no device."""
import ctypes as C

import numpy as np
import pytest

import layered_oracle as lo
from oracle import oracle
from qldpc_amd import _lib, bp, layered, mc

MATRICES = ["steane", "72", "irr37", "disjoint70", "144"]
ORDERS = ["default", "ascending", "random"]


def batch(H, ps, per_p, seed):
    """Errors of rate p for every p of `ps` (per_p each), their syndromes, and a non-uniform prior."""
    H = np.asarray(H)
    n = H.shape[1]
    rng = np.random.default_rng(seed)
    errors = np.concatenate([(rng.random((per_p, n)) < p).astype(np.uint8) for p in ps])
    syn = (errors.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    prior = np.log(0.95 / 0.05) * rng.uniform(0.5, 1.5, n)
    return errors, syn, prior


# ---- 1. the two forms of the statement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("kind", ORDERS)
def test_sequential_and_level_forms_agree_in_every_bit(name, kind):
    H = lo.matrix(name)
    _, syn, prior = batch(H, (0.01, 0.05, 0.15), 8, 11)
    order = lo.order_of(H, kind)
    for variant, alpha in ((lo.SUM_PRODUCT, 1.0), (lo.MIN_SUM, 0.8)):
        a = lo.layered_decode_batch(H, syn, prior, 12, variant, alpha, 20.0, order, "sequential")
        b = lo.layered_decode_batch(H, syn, prior, 12, variant, alpha, 20.0, order, "level")
        for x, y, what in zip(a, b, ("hard", "converged", "iters", "llr")):
            assert lo.same(x, y), (name, kind, variant, what)
        assert not np.isnan(a[3]).any()


def test_steane_has_one_level_per_check():
    H = lo.steane()
    assert [len(g) for g in lo.levels_of(H, np.arange(3))] == [1, 1, 1]       # (every pair of rows shares a variable)


# ---- 2. qbp_layered_plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("kind", ORDERS)
def test_plan_levels_are_conflict_free_and_concatenate_to_the_order(name, kind):
    H = lo.matrix(name)
    m, n = H.shape
    row_ptr, col_idx, _, _ = bp.csr_from_H(H)
    order_in = None if kind == "default" else lo.order_of(H, kind)
    order, lptr = _lib.layered_plan(row_ptr, col_idx, m, n, order_in)
    assert lptr[0] == 0 and lptr[-1] == m and np.all(np.diff(lptr) >= 1)
    assert sorted(order.tolist()) == list(range(m))
    Hi = H.astype(np.int64)
    for a, b in zip(lptr[:-1], lptr[1:]):
        assert Hi[order[a:b]].sum(axis=0).max(initial=0) <= 1            # no two checks of a level share a variable
    want = lo.levels_of(H, lo.order_of(H, kind))
    assert len(want) == len(lptr) - 1
    assert np.array_equal(np.concatenate(want), order)                   # the levels, one after another, are the order
    assert [len(g) for g in want] == np.diff(lptr).tolist()
    # every ordered pair of conflicting checks keeps its order
    src = lo.order_of(H, kind)
    pos_in = np.argsort(src)
    pos_out = np.argsort(order)
    share = (Hi @ Hi.T) > 0
    for c in range(m):
        for c2 in np.flatnonzero(share[c]):
            if c != c2:
                assert (pos_in[c] < pos_in[c2]) == (pos_out[c] < pos_out[c2])
    # layered.layered_order is the same plan
    o2, levels = layered.layered_order(H, order_in)
    assert np.array_equal(o2, order) and all(np.array_equal(x, y) for x, y in zip(levels, want))


@pytest.mark.parametrize("name", MATRICES)
def test_default_order_is_the_numpy_greedy_colouring(name):
    H = lo.matrix(name)
    m, n = H.shape
    row_ptr, col_idx, _, _ = bp.csr_from_H(H)
    order, lptr = _lib.layered_plan(row_ptr, col_idx, m, n)
    want, colour = lo.default_order(H)
    assert np.array_equal(order, want)
    assert len(lptr) - 1 == colour.max() + 1                             # a colour is a level
    assert np.array_equal(lo.check_levels(H, want), colour + 1)


def test_default_order_stays_shallow_on_the_bb_codes():
    for name in ("72", "144"):
        H = lo.matrix(name)
        assert len(lo.levels_of(H, lo.default_order(H)[0])) <= 13
        assert len(lo.levels_of(H, np.arange(H.shape[0]))) > 13          # ascending index: long chains


# ---- 3. refusals that need no device ------------------------------------------------------------------------------------
def plan_rc(row_ptr, col_idx, m, n, order_in, order_out=True, level_ptr=True, n_levels=True):
    lib = _lib.load()
    out = np.zeros(max(m, 1), np.int32)
    lptr = np.zeros(max(m, 1) + 1, np.int32)
    nl = C.c_int32(0)
    return lib.qbp_layered_plan(None if row_ptr is None else row_ptr.ctypes.data,
                                None if col_idx is None else col_idx.ctypes.data, m, n,
                                None if order_in is None else np.ascontiguousarray(order_in, np.int32).ctypes.data,
                                out.ctypes.data if order_out else None, lptr.ctypes.data if level_ptr else None,
                                C.byref(nl) if n_levels else None)


def test_plan_rejects_what_is_not_a_permutation_and_bad_arguments():
    H = lo.matrix("72")
    m, n = H.shape
    rp, ci, _, _ = bp.csr_from_H(H)
    assert plan_rc(rp, ci, m, n, None) == 0
    assert plan_rc(rp, ci, m, n, np.arange(m)[::-1]) == 0
    dup = np.arange(m); dup[5] = 4
    low = np.arange(m); low[0] = -1
    high = np.arange(m); high[-1] = m
    for bad in (dup, low, high):
        assert plan_rc(rp, ci, m, n, bad) == _lib.E_INVALID
        assert "order" in _lib.load().qbp_last_error().decode()
    assert plan_rc(None, ci, m, n, None) == _lib.E_INVALID
    assert plan_rc(rp, None, m, n, None) == _lib.E_INVALID
    assert plan_rc(rp, ci, 0, n, None) == _lib.E_INVALID
    assert plan_rc(rp, ci, m, 0, None) == _lib.E_INVALID
    for kw in (dict(order_out=False), dict(level_ptr=False), dict(n_levels=False)):
        assert plan_rc(rp, ci, m, n, None, **kw) == _lib.E_INVALID
    unsorted = ci.copy(); unsorted[[0, 1]] = unsorted[[1, 0]]
    assert plan_rc(rp, unsorted, m, n, None) == _lib.E_INVALID
    wide = ci.copy(); wide[3] = n
    assert plan_rc(rp, wide, m, n, None) == _lib.E_INVALID
    with pytest.raises(_lib.QbpError) as e:
        _lib.layered_plan(rp, ci, m, n, dup)
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        _lib.layered_plan(rp, ci, m, n, np.arange(m - 1))


def test_entries_refuse_a_null_handle():
    lib = _lib.load()
    assert lib.qbp_layered_configure(None, None) == _lib.E_INVALID
    assert lib.qbp_set_option(None, _lib.OPT_LAYERED_SLOTS, 1) == _lib.E_INVALID


def test_python_argument_checks():
    H = lo.matrix("steane")
    with pytest.raises(ValueError):
        layered.performLayeredBP(H, np.zeros(3), np.ones(7), variant="damped")
    with pytest.raises(ValueError):
        layered.performLayeredBP(H, np.zeros(3), np.ones(7), variant=1)
    with pytest.raises(ValueError):
        layered.performLayeredBP(H, np.zeros(3), np.array([1, 1, np.inf, 1, 1, 1, 1.0]))
    with pytest.raises(ValueError):
        mc.layered_run_flags(0, True, _lib.DAMPED_SP)
    assert mc.layered_run_flags(_lib.FLAG_OSD0, True, _lib.MIN_SUM) == _lib.FLAG_OSD0 | _lib.FLAG_LAYERED
    assert mc.layered_run_flags(_lib.FLAG_OSD0, np.arange(3), _lib.SUM_PRODUCT) == _lib.FLAG_OSD0 | _lib.FLAG_LAYERED
    assert mc.layered_run_flags(7, False, _lib.DAMPED_SP) == 7 and mc.layered_run_flags(7, None, 0) == 7
    assert _lib.FLAG_LAYERED == 1024 and _lib.OPT_LAYERED_SLOTS == 15
    with pytest.raises(SystemExit):
        mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05", "--trials", "10", "--layered", "--variant", "damped"])


# ---- 4. the statement on [[72,12,6]] ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [lo.SUM_PRODUCT, lo.MIN_SUM])
def test_statement_outputs_are_consistent(variant, capsys):
    H = lo.matrix("72")
    Hi = H.astype(np.int64)
    n = H.shape[1]
    for p in (0.03, 0.08):
        errors = (np.random.default_rng(int(p * 1000)).random((256, n)) < p).astype(np.uint8)
        syn = (errors.astype(np.int64) @ Hi.T % 2).astype(np.uint8)
        prior = np.full(n, np.log((1 - p) / p))
        hard, conv, iters, llr = lo.layered_decode_batch(H, syn, prior, 50, variant, 0.9)
        assert np.array_equal(hard[conv].astype(np.int64) @ Hi.T % 2, syn[conv])
        assert np.any(hard[~conv].astype(np.int64) @ Hi.T % 2 != syn[~conv], axis=1).all()
        assert np.all(iters[~conv] == 49) and np.all((iters >= 0) & (iters <= 49))
        assert np.array_equal(hard, (llr < 0).astype(np.uint8))
        # a record that converged at iteration t is the same record decoded with max_iter = t + 1 and not with t
        t = int(iters[conv].max())
        h2, c2, i2, l2 = lo.layered_decode_batch(H, syn, prior, t + 1, variant, 0.9)
        assert np.array_equal(c2, conv) and lo.same(l2[conv], llr[conv]) and np.array_equal(i2[conv], iters[conv])
        if t > 0:
            c3 = lo.layered_decode_batch(H, syn, prior, t, variant, 0.9)[1]
            assert c3.sum() == (iters[conv] < t).sum()
        f_hard, f_conv, f_iters, _ = oracle.decode_batch(H, syn, prior, 50, variant, alpha=0.9, damping=1.0)
        with capsys.disabled():
            print(f"\n[[72,12,6]] p = {p} variant {variant}: layered mean iterations {iters.mean():.2f}, unconverged "
                  f"{int((~conv).sum())} / 256; flooding {f_iters.mean():.2f}, {int((~f_conv).sum())} / 256")
