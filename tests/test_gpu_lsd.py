"""GPU: lsd_kernel against the numpy statement of localized statistics decoding (tests/lsd_oracle.py), bit for bit and
through the C ABI -- the batch build on seven matrices and three step sizes, independence of the batch size, the grid,
the stream and an earlier configuration into poisoned buffers, and the records build behind QBP_FLAG_LSD against the
composition of first-stage decode, statement and classification."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lsd_oracle as lo
import lsd_util as lu
from oracle import oracle
from qldpc_amd import _lib, bp, codes, lsd, mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = (0, 1, 3)
# matrix, p of the BP(50) inputs, records
CASES = [("steane", 0.2, 96), ("72", 0.08, 96), ("rand37", 0.08, 96), ("74", 0.08, 96), ("rows70", 0.003, 96),
         ("144", 0.07, 96), ("288", 0.07, 64)]


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def inputs(name, p, B):
    """BP(50) outputs, and four records made special: exact ties and a NaN in the llr, an all-zero residual, and two
    syndromes with one bit flipped (outside the column space wherever H has dependent rows)."""
    H = lu.matrix(name)
    syn, llr, hard, conv = lu.bp_outputs(H, p, 3, B, 50)
    assert 0 < conv.sum() < B, (name, int(conv.sum()))
    syn, llr = syn.copy(), llr.copy()
    f = np.flatnonzero(~conv)
    llr[f[0]] = np.round(llr[f[0]])
    llr[f[0], 1] = np.nan
    syn[f[1]] = hard[f[1]].astype(np.int64) @ H.T % 2
    syn[f[2], 0] ^= 1
    syn[f[3], H.shape[0] - 1] ^= 1
    return H, syn, llr, hard


_REF = {}


def reference(name, g):
    """The statement on a case, computed once."""
    if (name, g) not in _REF:
        p, B = next((p, B) for n_, p, B in CASES if n_ == name)
        if name not in _REF:
            _REF[name] = inputs(name, p, B)
        H, syn, llr, hard = _REF[name]
        _REF[name, g] = lo.lsd_decode_batch(H, syn, llr, hard, g)
    return _REF[name] + (_REF[name, g],)


# ---- 1. the batch kernel against the statement -------------------------------------------------------------------------
@pytest.mark.parametrize("g", G)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_batch_kernel_equals_statement(name, g):
    H, syn, llr, hard, want = reference(name, g)
    print(name, g, lo.presence(want), float(want["stats"][:, 1].mean()))
    dec = fresh(H)
    sol, stats = dec.lsd(syn, llr, hard, g)
    assert np.array_equal(stats, want["stats"])
    assert np.array_equal(sol, want["solution"])
    # no statistics wanted, and a second call on the configured handle
    sol2, none = dec.lsd(syn[:40], llr[:40], hard[:40], want_stats=False)
    assert none is None and np.array_equal(sol2, want["solution"][:40])
    got = lsd.performLSDBatch(H, syn[:8], llr[:8], hard[:8], g)
    assert got[0].dtype == np.int8 and np.array_equal(got[0], want["solution"][:8])
    assert np.array_equal(got[1], want["stats"][:8])
    assert np.array_equal(lsd.performLSD(H, syn[5], llr[5], hard[5], g), want["solution"][5])


def test_inputs_cover_every_situation():
    """On the statement's side, pooled over the cases: records with >= 2 clusters at the end, merged clusters, >= 3
    rounds, a dependent column, an invalid result (valid = 0), and an all-zero residual."""
    pooled = {}
    for name, _, _ in CASES:
        for g in G:
            for k, v in lo.presence(reference(name, g)[4]).items():
                pooled[k] = pooled.get(k, 0) + v
    print(pooled)
    assert all(pooled[k] >= 1 for k in ("two_clusters", "merged", "three_rounds", "skipped", "invalid", "trivial")), pooled


# ---- 2. independence of B, the grid, the stream and an earlier configuration ----------------------------------------------
@pytest.mark.parametrize("B", [1, 65, 1000])
def test_poisoned_outputs_geometry_stream_and_reuse(B):
    import torch as t
    H, syn, llr, hard, _ = reference("72", 1)
    n = H.shape[1]
    idx = (np.arange(B) * 7 + 3) % len(syn)
    dec = fresh(H)
    dev = t.device("cuda", dec.device)
    stream = t.cuda.Stream(dev)
    syn_t, llr_t, hard_t = (t.from_numpy(np.ascontiguousarray(a[idx])).to(dev) for a in (syn, llr, hard))
    for g, per_cu in ((3, 0), (1, 0), (1, 1), (0, 3), (1, 3)):               # (g = 1 follows g = 3 on the same handle)
        want = reference("72", g)[4]
        dec.lsd_configure(g)
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
        try:
            # room for one more record behind every output: it must keep the poison
            sol_t = t.full((B + 1, n), 0xAB, dtype=t.uint8, device=dev)
            st_t = t.full((B + 1, 4), -77, dtype=t.int32, device=dev)
            t.cuda.synchronize(dev)
            with t.cuda.stream(stream):
                dec.lsd_device(syn_t.data_ptr(), llr_t.data_ptr(), hard_t.data_ptr(), B, sol_t.data_ptr(), st_t.data_ptr(),
                               stream=stream.cuda_stream)
            stream.synchronize()
        finally:
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)
        assert np.array_equal(sol_t[:B].cpu().numpy(), want["solution"][idx])
        assert np.array_equal(st_t[:B].cpu().numpy(), want["stats"][idx])
        assert bool((sol_t[B] == 0xAB).all()) and bool((st_t[B] == -77).all())


# ---- 3. QBP_FLAG_LSD: the records build ------------------------------------------------------------------------------------
MC_ITERS, ALPHA = 8, 0.9


def compose(dec, H, L, d, errors, prior, g, variant, layered):
    """qbp_decode_batch (first stage), the statement on its failures, oracle.classify_trials' rules."""
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, llr = dec.decode(syn, prior, MC_ITERS, variant=variant, alpha=ALPHA, layered=layered)
    det = hard.copy()
    f = np.flatnonzero(~conv)
    r = lo.lsd_decode_batch(H, syn[f], llr[f], hard[f], g)
    det[f] = r["solution"]
    cnt = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    cnt[10] = int((r["stats"][:, 3] == 0).sum())
    assert cnt[10] == int(((det[f].astype(np.int64) @ H.T % 2) != syn[f]).any(1).sum())
    return cnt, len(f)


@pytest.mark.parametrize("first", ["sum_product", "min_sum", "layered"])
@pytest.mark.parametrize("name,p,g", [("72", 0.08, 1), ("72", 0.08, 0), ("144", 0.06, 1), ("144", 0.06, 3)])
def test_mc_run_errors_equals_the_composition(name, p, g, first):
    c = codes.load_code(lu.NAMES[name])
    H, L, d = np.asarray(c.Hx, np.uint8), np.asarray(c.Lx, np.uint8), c.distance
    n = H.shape[1]
    errors = (np.random.default_rng(17).random((400, n)) < p).astype(np.uint8)
    prior = mc.prior_of(p, n)
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    layered = first == "layered"
    dec = fresh(H)
    dec.lsd_configure(g)
    if layered:
        dec.layered_configure(None)
    want, failures = compose(dec, H, L, d, errors, prior, g, variant, layered)
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=ALPHA, flags=_lib.FLAG_LSD | (_lib.FLAG_LAYERED if layered else 0))
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), failures)
    assert failures >= 8 and got[6] == failures and got[0] == 400
    assert np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, **kw), want)       # the record buffers reused
    assert np.array_equal(dec.mc_run_errors(L, d, errors[:150], prior, **kw)
                          + dec.mc_run_errors(L, d, errors[150:], prior, **kw), want)


def test_sampled_entries_split_chunk_and_run_sweep():
    c = codes.load_code(lu.NAMES["72"])
    H, L, d = np.asarray(c.Hx, np.uint8), np.asarray(c.Lx, np.uint8), c.distance
    prior = mc.prior_of(0.08, 72)
    dec = fresh(H)
    dec.lsd_configure(1)
    kw = dict(seed=21, max_iter=MC_ITERS, flags=_lib.FLAG_LSD)
    whole = dec.mc_run(L, d, 0.08, prior, 0, 1000, **kw)
    assert whole[0] == 1000 and whole[6] >= 8
    parts = dec.mc_run(L, d, 0.08, prior, 0, 1, **kw) + dec.mc_run(L, d, 0.08, prior, 1, 377, **kw) \
        + dec.mc_run(L, d, 0.08, prior, 377, 1000, **kw)
    assert np.array_equal(parts, whole)
    errors = dec.mc_sample_errors(0.08, 0, 1000, seed=21)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, max_iter=MC_ITERS, flags=_lib.FLAG_LSD), whole)
    want, _ = compose(dec, H, L, d, errors, prior, 1, _lib.SUM_PRODUCT, False)
    assert np.array_equal(whole, want)
    other = fresh(H)
    other.lsd_configure(1)
    assert np.array_equal(other.mc_run_probs(L, d, np.full(72, 0.08), prior, 0, 1000, **kw), whole)
    bp_only = dec.mc_run(L, d, 0.08, prior, 0, 1000, seed=21, max_iter=MC_ITERS)
    assert np.array_equal(bp_only[[0, 6, 7]], whole[[0, 6, 7]])      # the first stage's bookkeeping is untouched
    # fixed weight, whole and in two chunk sizes
    kw = dict(max_iter=MC_ITERS, flags=_lib.FLAG_LSD)
    got = dec.mc_run_weight(L, d, 9, prior, 0, 500, seed=4, **kw)
    werr = dec.mc_sample_errors_weight(9, 0, 500, seed=4)
    assert got[6] >= 8 and np.array_equal(got, dec.mc_run_errors(L, d, werr, prior, **kw))
    dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 64)
    try:
        assert np.array_equal(got, dec.mc_run_weight(L, d, 9, prior, 0, 500, seed=4, **kw))
    finally:
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)
    assert np.array_equal(got, compose(dec, H, L, d, werr, prior, 1, _lib.SUM_PRODUCT, False)[0])
    # mc.run_sweep returns the same row
    table = mc.run_sweep(lu.NAMES["72"], [0.08], 1000, seed=21, max_iter=MC_ITERS, lsd=1)
    assert np.array_equal(table[0], whole)


# ---- 4. QBP_E_INVALID and QBP_E_UNSUPPORTED -----------------------------------------------------------------------------------
def test_invalid_and_unsupported_cases():
    from qldpc_amd import gd, relay
    c = codes.load_code(lu.NAMES["72"])
    H, L, d = np.asarray(c.Hx, np.uint8), np.asarray(c.Lx, np.uint8), c.distance
    Lx = np.ascontiguousarray(L, np.uint8)
    n = 72
    prior = mc.prior_of(0.05, n)
    lib = _lib.load()
    dec = fresh(H)
    fill = np.full(12, 7, np.int64)

    def run(flags):
        counters = fill.copy()
        rc = lib.qbp_mc_run(dec._h, Lx.ctypes.data, Lx.shape[0], d, 0.05, 1, 0, 0, 200, prior.ctypes.data, MC_ITERS, 0, 1.0,
                            1.0, 20.0, flags, counters.ctypes.data)
        assert rc == 0 or np.array_equal(counters, fill)
        return rc

    syn, llr, hard = np.zeros((4, 36), np.uint8), np.zeros((4, n)), np.zeros((4, n), np.uint8)
    sol = np.full((4, n), 9, np.uint8)
    args = (dec._h, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data, 4, sol.ctypes.data, None)
    assert lib.qbp_lsd_batch(*args) == -1 and b"qbp_lsd_configure" in lib.qbp_last_error() and np.all(sol == 9)
    assert lib.qbp_lsd_batch_device(dec._h, 8, 8, 8, 4, 8, None, None) == -1
    assert run(_lib.FLAG_LSD) == -1 and b"qbp_lsd_configure" in lib.qbp_last_error()
    assert lib.qbp_lsd_configure(dec._h, -1) == -1
    assert run(_lib.FLAG_LSD) == -1                         # (a refused configuration configures nothing)
    assert lib.qbp_lsd_configure(dec._h, 2) == 0
    assert run(_lib.FLAG_LSD) == 0
    assert lib.qbp_lsd_batch(dec._h, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data, 4, None, None) == -1
    assert lib.qbp_lsd_batch(dec._h, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data, 0, None, None) == 0
    # one second stage per call
    dec.relay_configure(relay.RelayConfig(np.zeros((1, n)), [3]))
    dec.gd_configure(gd.GDConfig(4, 2))
    for flags in (_lib.FLAG_LSD | _lib.FLAG_OSD0, _lib.FLAG_LSD | _lib.osd_flags("cs", 3),
                  _lib.FLAG_LSD | _lib.FLAG_OSD_E | (2 << 16), _lib.FLAG_LSD | _lib.FLAG_OSD_LARGE,
                  _lib.FLAG_LSD | _lib.FLAG_RELAY, _lib.FLAG_LSD | _lib.FLAG_GD):
        assert run(flags) == -1
        with pytest.raises(_lib.QbpError) as e:
            dec.mc_run_weight(L, d, 3, prior, 0, 100, flags=flags)
        assert e.value.code == -1
    # entries without such a stage
    probs = np.full(n, 0.05)
    for fn in (lambda: dec.mc_run_budgets(L, d, probs, prior, (4, 8), 0, 100, flags=_lib.FLAG_LSD),
               lambda: dec.mc_run_spectrum(L, d, probs, prior, 0, 100, max_iter=8, flags=_lib.FLAG_LSD),
               lambda: dec.mc_run_errors_spectrum(L, d, np.zeros((10, n), np.uint8), prior, max_iter=8,
                                                  flags=_lib.FLAG_LSD),
               lambda: dec.decode_shots(L, np.zeros((10, 5), np.uint8), prior, max_iter=8, flags=_lib.FLAG_LSD)):
        with pytest.raises(_lib.QbpError) as e:
            fn()
        assert e.value.code == _lib.E_UNSUPPORTED
    # the limits: 432 x 1296 fits, 864 x 2592 does not (CSR only, nothing is decoded)
    for m_big, n_big, ok in ((432, 1296, True), (864, 2592, False)):
        rows = np.repeat(np.arange(m_big), 9)
        cols = (np.arange(m_big * 9) * 7 + rows) % n_big
        Hb = np.zeros((m_big, n_big), np.uint8)
        Hb[rows, cols] = 1
        Hb[np.arange(n_big) % m_big, np.arange(n_big)] = 1      # (no empty column)
        big = fresh(Hb)
        rc = lib.qbp_lsd_configure(big._h, 1)
        assert rc == (0 if ok else _lib.E_UNSUPPORTED), (m_big, rc)
        if not ok:
            assert b"160 KiB" in lib.qbp_last_error() and re_bytes(lib.qbp_last_error()) > 160 * 1024
        else:
            syn = np.zeros((3, m_big), np.uint8)
            syn[1, 5] = syn[2, 400] = syn[2, 17] = 1
            llr = np.abs(np.random.default_rng(1).normal(3, 1, (3, n_big)))
            hard = np.zeros((3, n_big), np.uint8)
            sol, stats = big.lsd(syn, llr, hard, 1)
            want = lo.lsd_decode_batch(Hb, syn, llr, hard, 1)
            assert np.array_equal(sol, want["solution"]) and np.array_equal(stats, want["stats"])


def re_bytes(msg):
    import re
    return int(re.search(rb"needs (\d+) B", msg).group(1))


# ---- 5. the command line ---------------------------------------------------------------------------------------------------
def test_cli_agrees_with_run_sweep(tmp_path):
    table = mc.run_sweep("[[72, 12, 6]]", [0.08], 2000, seed=3, max_iter=8, lsd=1)
    assert table[0, 0] == 2000 and table[0, 6] >= 8 and table[0, 10] == 0
    out = tmp_path / "lsd.json"
    subprocess.check_call([sys.executable, "-m", "qldpc_amd.mc", "--code", "[[72, 12, 6]]", "--p", "0.08", "--trials",
                           "2000", "--seed", "3", "--max-iter", "8", "--lsd", "1", "--out", str(out)], cwd=ROOT)
    rows = json.load(open(out))["points"]
    assert [rows[0][k] for k in _lib.COUNTER_NAMES[:11]] == table[0, :11].tolist()
