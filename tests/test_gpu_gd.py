"""GPU: bp_gd_kernel against the numpy statement of BP guided decimation (tests/gd_oracle.py), bit for bit and through
the C ABI -- the batch build on five matrices and both variants, the max_rounds = 0 identity with qbp_decode_batch,
poisoned outputs and launch geometry, and the records build behind QBP_FLAG_GD against the composition of first-stage
decode, statement and classification.

"Bit for bit" for float64 outputs: equal values, NaN equal to NaN (the irregular matrix has checks of weight 1, whose
min-sum message is infinite and turns its variable's posterior into NaN)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gd_oracle as go
from oracle import oracle
from qldpc_amd import _lib, bp, codes, gd, mc
from test_gpu_relay import CASES, irregular37

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_ROUND, LLR, ALPHA = 8, 25.0, 0.9
VARIANTS = [_lib.SUM_PRODUCT, _lib.MIN_SUM]
VIDS = ["sum_product", "min_sum"]
# the cases of tests/test_gpu_relay.py, and [[72,12,6]] with two all-zero columns appended (isolated variables)
GD_CASES = CASES + [("74", 0.1, 1)]
ROUNDS = ["n", 6]                       # max_rounds = n runs the candidates to exhaustion


def matrix(name):
    if name == "rand37":
        H, L = irregular37()
        return H, L, 4
    if name == "74":
        c = codes.load_code("[[72, 12, 6]]")
        z = np.zeros((c.Hx.shape[0], 2), np.uint8)
        return (np.concatenate([np.asarray(c.Hx, np.uint8), z], axis=1),
                np.concatenate([np.asarray(c.Lx, np.uint8), np.zeros((c.Lx.shape[0], 2), np.uint8)], axis=1), c.distance)
    c = codes.load_code({"steane": "steane", "72": "[[72, 12, 6]]", "144": "[[144, 12, 12]]"}[name])
    return np.asarray(c.Hx), np.asarray(c.Lx), c.distance


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def config(variant, max_rounds, T=T_ROUND):
    return gd.GDConfig(T, max_rounds, LLR, variant, ALPHA, 20.0)


def inputs(name, p, seed):
    H, _, _ = matrix(name)
    n = H.shape[1]
    errors = (np.random.default_rng(seed).random((256, n)) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log((1 - p) / p))
    if name == "74":
        prior[72:] = [50.0, -60.0]      # (the largest |prior| by far: an isolated variable must still not be chosen)
    return H, syn, prior


@pytest.fixture(scope="module")
def references():
    """The statement on every (case, variant, max_rounds), computed once: (H, syndromes, prior, config, result)."""
    out = {}
    for name, p, seed in GD_CASES:
        H, syn, prior = inputs(name, p, seed)
        for variant in VARIANTS:
            for rounds in ROUNDS:
                cfg = config(variant, H.shape[1] if rounds == "n" else rounds)
                out[name, p, variant, rounds] = (H, syn, prior, cfg, go.gd_decode_batch(
                    H, syn, prior, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, variant, ALPHA, 20.0))
    return out


# ---- 1. the batch kernel against the statement -------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", ROUNDS, ids=["to_exhaustion", "six_rounds"])
@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("name,p,seed", GD_CASES)
def test_batch_kernel_equals_statement(references, name, p, seed, variant, rounds):
    """The three classes (solved in round 0, after >= 1 decimation, never) are counted on the statement's output over
    the pooled cases: Steane is all round 0, the irregular matrix shows round 0 and never only."""
    pooled = {k: sum(go.classes(r[4])[k] for r in references.values()) for k in ("round0", "later", "never")}
    H, syn, prior, cfg, want = references[name, p, variant, rounds]
    print(pooled, go.classes(want), int(want["iters"].max()))
    assert all(v >= 8 for v in pooled.values()), pooled
    dec = fresh(H)
    hard, conv, iters, llr, rnds = dec.gd_decode(syn, prior, cfg)
    assert np.array_equal(conv, want["converged"])
    assert np.array_equal(rnds, want["rounds"])
    assert np.array_equal(iters, want["iters"])
    assert np.array_equal(hard, want["hard"])
    assert go.same(llr, want["llr"])
    # null outputs, and a second call on the configured handle
    h2, c2, i2, none, r2 = dec.gd_decode(syn[:100], prior, want_llr=False)
    assert none is None and np.array_equal(h2, hard[:100]) and np.array_equal(i2, iters[:100])
    assert np.array_equal(r2, rnds[:100]) and np.array_equal(c2, conv[:100])
    lib = _lib.load()
    only = np.full(256, -5, np.int32)
    assert lib.qbp_gd_decode_batch(dec._h, syn.ctypes.data, prior.ctypes.data, 256, None, None, None, None,
                                   only.ctypes.data) == 0
    assert np.array_equal(only, want["rounds"])
    assert lib.qbp_gd_decode_batch(dec._h, syn.ctypes.data, prior.ctypes.data, 256, None, None, None, None, None) == 0


# ---- 2. max_rounds = 0: the device's flooding decoders -------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("name", ["72", "rand37"])
def test_without_decimation_is_decode_batch_on_the_device(name, variant):
    H, _, _ = matrix(name)
    n = H.shape[1]
    errors = (np.random.default_rng(5).random((300, n)) < 0.05).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log(0.95 / 0.05))
    dec = fresh(H)
    hard, conv, iters, llr = dec.decode(syn, prior, 30, variant=variant, alpha=0.8, damping=1.0)
    g_hard, g_conv, g_iters, g_llr, rnds = dec.gd_decode(syn, prior, gd.GDConfig(30, 0, LLR, variant, 0.8, 20.0))
    assert 20 < conv.sum() < 300
    assert np.array_equal(g_hard, hard) and np.array_equal(g_conv, conv)
    assert np.array_equal(g_iters, np.where(conv, iters + 1, 30))
    assert go.same(g_llr, llr) and np.all(rnds == 0)


# ---- 3. poisoned outputs, launch geometry, the device entry on a stream of its own ----------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("B", [1, 63, 257])
def test_poisoned_outputs_and_geometry(references, variant, B):
    import torch as t
    H, syn, prior, cfg, want = references["72", 0.1, variant, 6]
    idx = np.arange(B) % 256
    syn_b = np.ascontiguousarray(syn[idx])
    dec = fresh(H)
    dec.gd_configure(cfg)
    dev = t.device("cuda", dec.device)
    stream = t.cuda.Stream(dev)
    syn_t = t.from_numpy(syn_b).to(dev)
    prior_t = t.from_numpy(prior).to(dev)
    for per_cu in (0, 1, 3):
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
        try:
            # room for one more record behind every output: it must keep the poison
            hard_t = t.full((B + 1, 72), 0xAB, dtype=t.uint8, device=dev)
            conv_t = t.full((B + 1,), 0xAB, dtype=t.uint8, device=dev)
            it_t = t.full((B + 1,), -77, dtype=t.int32, device=dev)
            rn_t = t.full((B + 1,), -77, dtype=t.int32, device=dev)
            llr_t = t.full((B + 1, 72), float("nan"), dtype=t.float64, device=dev)
            t.cuda.synchronize(dev)
            with t.cuda.stream(stream):
                dec.gd_decode_device(syn_t.data_ptr(), prior_t.data_ptr(), B, hard_t.data_ptr(), conv_t.data_ptr(),
                                     it_t.data_ptr(), llr_t.data_ptr(), rn_t.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
        finally:
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)
        assert np.array_equal(hard_t[:B].cpu().numpy(), want["hard"][idx])
        assert np.array_equal(conv_t[:B].cpu().numpy().astype(bool), want["converged"][idx])
        assert np.array_equal(it_t[:B].cpu().numpy(), want["iters"][idx])
        assert np.array_equal(rn_t[:B].cpu().numpy(), want["rounds"][idx])
        assert go.same(llr_t[:B].cpu().numpy(), want["llr"][idx])
        assert np.all(hard_t[B].cpu().numpy() == 0xAB) and conv_t[B].item() == 0xAB
        assert it_t[B].item() == -77 and rn_t[B].item() == -77 and bool(t.isnan(llr_t[B]).all())


# ---- 4. QBP_FLAG_GD: the records build -------------------------------------------------------------------------------------
MC_ITERS = 8


def compose(dec, H, L, d, errors, prior, cfg, variant, layered):
    """qbp_decode_batch (first stage), the statement on its failures, oracle.classify_trials' rules."""
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, _ = dec.decode(syn, prior, MC_ITERS, variant=variant, alpha=ALPHA, layered=layered)
    det = hard.copy()
    f = np.flatnonzero(~conv)
    r = go.gd_decode_batch(H, syn[f], prior, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant, cfg.alpha,
                           cfg.clip_llr)
    det[f] = r["hard"]
    cnt = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    cnt[10] = int((~r["converged"]).sum())
    assert cnt[10] == int(((det[f].astype(np.int64) @ H.T % 2) != syn[f]).any(1).sum())
    return cnt, len(f)


@pytest.mark.parametrize("first", ["sum_product", "min_sum", "layered"])
@pytest.mark.parametrize("name,p", [("72", 0.08), ("rand37", 0.06), ("144", 0.06)])
def test_mc_run_errors_equals_the_composition(name, p, first):
    H, L, d = matrix(name)
    n = H.shape[1]
    errors = (np.random.default_rng(17).random((500, n)) < p).astype(np.uint8)
    prior = mc.prior_of(p, n)
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    layered = first == "layered"
    # the second stage's variant is the configuration's own: the other one than the first stage's, both get covered
    cfg = config(_lib.SUM_PRODUCT if first == "min_sum" else _lib.MIN_SUM, 6)
    dec = fresh(H)
    dec.gd_configure(cfg)
    if layered:
        dec.layered_configure(None)
    want, failures = compose(dec, H, L, d, errors, prior, cfg, variant, layered)
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=ALPHA,
              flags=_lib.FLAG_GD | (_lib.FLAG_LAYERED if layered else 0))
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), failures)
    assert failures >= 8 and got[6] == failures and got[0] == 500
    assert np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, **kw), want)       # the record buffers reused
    assert np.array_equal(dec.mc_run_errors(L, d, errors[:200], prior, **kw)
                          + dec.mc_run_errors(L, d, errors[200:], prior, **kw), want)


def test_sampled_entries_and_the_split_of_the_range():
    H, L, d = matrix("72")
    prior = mc.prior_of(0.08, 72)
    cfg = config(_lib.MIN_SUM, 6)
    dec = fresh(H)
    dec.gd_configure(cfg)
    kw = dict(seed=21, max_iter=MC_ITERS, flags=_lib.FLAG_GD)
    whole = dec.mc_run(L, d, 0.08, prior, 0, 1000, **kw)
    assert whole[0] == 1000 and whole[6] >= 8
    parts = dec.mc_run(L, d, 0.08, prior, 0, 1, **kw) + dec.mc_run(L, d, 0.08, prior, 1, 377, **kw) \
        + dec.mc_run(L, d, 0.08, prior, 377, 1000, **kw)
    assert np.array_equal(parts, whole)
    # qbp_mc_run on the errors qbp_mc_sample_errors returns = qbp_mc_run_errors on them = the composition
    errors = dec.mc_sample_errors(0.08, 0, 1000, seed=21)
    stored = dec.mc_run_errors(L, d, errors, prior, max_iter=MC_ITERS, flags=_lib.FLAG_GD)
    assert np.array_equal(stored, whole)
    want, failures = compose(dec, H, L, d, errors, prior, cfg, _lib.SUM_PRODUCT, False)
    assert np.array_equal(whole, want) and whole[10] == want[10]
    other = fresh(H)
    other.gd_configure(cfg)
    assert np.array_equal(other.mc_run_probs(L, d, np.full(72, 0.08), prior, 0, 1000, **kw), whole)
    bp_only = dec.mc_run(L, d, 0.08, prior, 0, 1000, seed=21, max_iter=MC_ITERS)
    assert np.array_equal(bp_only[[0, 6, 7]], whole[[0, 6, 7]])      # the first stage's bookkeeping is untouched
    # fixed weight
    kw = dict(max_iter=MC_ITERS, flags=_lib.FLAG_GD)
    got = dec.mc_run_weight(L, d, 9, prior, 0, 500, seed=4, **kw)
    werr = dec.mc_sample_errors_weight(9, 0, 500, seed=4)
    assert got[6] >= 8 and np.array_equal(got, dec.mc_run_errors(L, d, werr, prior, **kw))
    assert np.array_equal(got, dec.mc_run_weight(L, d, 9, prior, 0, 123, seed=4, **kw)
                          + dec.mc_run_weight(L, d, 9, prior, 123, 500, seed=4, **kw))
    assert np.array_equal(got, compose(dec, H, L, d, werr, prior, cfg, _lib.SUM_PRODUCT, False)[0])


# ---- 5. QBP_E_INVALID and QBP_E_UNSUPPORTED -----------------------------------------------------------------------------------
def test_invalid_and_unsupported_cases():
    from qldpc_amd import relay
    H, L, d = matrix("72")
    Lx = np.ascontiguousarray(L, np.uint8)
    n = 72
    prior = mc.prior_of(0.05, n)
    lib = _lib.load()
    dec = fresh(H)
    syn = np.zeros((4, 36), np.uint8)
    fill = np.full(12, 7, np.int64)

    def run(flags, h=dec):
        counters = fill.copy()
        rc = lib.qbp_mc_run(h._h, Lx.ctypes.data, Lx.shape[0], d, 0.05, 1, 0, 0, 200, prior.ctypes.data, MC_ITERS, 0, 1.0,
                            1.0, 20.0, flags, counters.ctypes.data)
        assert rc == 0 or np.array_equal(counters, fill)
        return rc

    # nothing configured yet
    hard = np.full((4, n), 9, np.uint8)
    assert lib.qbp_gd_decode_batch(dec._h, syn.ctypes.data, prior.ctypes.data, 4, hard.ctypes.data, None, None, None,
                                   None) == -1
    assert b"qbp_gd_configure" in lib.qbp_last_error() and np.all(hard == 9)
    assert lib.qbp_gd_decode_batch_device(dec._h, 8, 8, 4, None, None, None, None, None, None) == -1
    assert run(_lib.FLAG_GD) == -1 and b"qbp_gd_configure" in lib.qbp_last_error()

    def configure(T=8, rounds=6, llr=25.0, variant=2, alpha=1.0, clip=20.0):
        return lib.qbp_gd_configure(dec._h, T, rounds, llr, variant, alpha, clip)

    for bad in (dict(T=0), dict(T=-3), dict(rounds=-1), dict(llr=0.0), dict(llr=-25.0), dict(llr=np.inf), dict(llr=np.nan),
                dict(variant=_lib.DAMPED_SP), dict(variant=3), dict(variant=-1), dict(alpha=np.nan), dict(alpha=np.inf),
                dict(clip=np.inf), dict(clip=np.nan)):
        assert configure(**bad) == -1, bad
    assert run(_lib.FLAG_GD) == -1                          # (a refused configuration configures nothing)
    assert configure() == 0
    assert run(_lib.FLAG_GD) == 0
    bad_prior = prior.copy()
    bad_prior[3] = np.inf
    assert lib.qbp_gd_decode_batch(dec._h, syn.ctypes.data, bad_prior.ctypes.data, 4, hard.ctypes.data, None, None, None,
                                   None) == -1
    assert b"prior[3]" in lib.qbp_last_error() and np.all(hard == 9)
    # one second stage per call
    dec.relay_configure(relay.RelayConfig(np.zeros((1, n)), [3]))
    for flags in (_lib.FLAG_GD | _lib.FLAG_OSD0, _lib.FLAG_GD | _lib.osd_flags("cs", 3),
                  _lib.FLAG_GD | _lib.FLAG_OSD_E | (2 << 16), _lib.FLAG_GD | _lib.FLAG_OSD_LARGE,
                  _lib.FLAG_GD | _lib.FLAG_RELAY):
        assert run(flags) == -1
        with pytest.raises(_lib.QbpError) as e:
            dec.mc_run_weight(L, d, 3, prior, 0, 100, flags=flags)
        assert e.value.code == -1
    counters = fill.copy()                                  # the record limit of QBP_FLAG_OSD0
    assert lib.qbp_mc_run(dec._h, Lx.ctypes.data, Lx.shape[0], d, 0.05, 1, 0, 0, _lib.MC_OSD_MAX_TRIALS + 1,
                          prior.ctypes.data, MC_ITERS, 0, 1.0, 1.0, 20.0, _lib.FLAG_GD, counters.ctypes.data) == -1
    assert b"at most" in lib.qbp_last_error() and np.array_equal(counters, fill)
    # entries without such a stage
    probs = np.full(n, 0.05)
    for fn in (lambda: dec.mc_run_budgets(L, d, probs, prior, (4, 8), 0, 100, flags=_lib.FLAG_GD),
               lambda: dec.mc_run_spectrum(L, d, probs, prior, 0, 100, max_iter=8, flags=_lib.FLAG_GD),
               lambda: dec.mc_run_errors_spectrum(L, d, np.zeros((10, n), np.uint8), prior, max_iter=8,
                                                  flags=_lib.FLAG_GD),
               lambda: dec.decode_shots(L, np.zeros((10, 5), np.uint8), prior, max_iter=8, flags=_lib.FLAG_GD)):
        with pytest.raises(_lib.QbpError) as e:
            fn()
        assert e.value.code == _lib.E_UNSUPPORTED
    # a matrix whose state does not fit the LDS: 2592 x 7776, CSR only, nothing is decoded
    m_big, n_big = 2592, 7776
    rows = np.repeat(np.arange(m_big), 9)
    cols = (np.arange(m_big * 9) * 7 + rows) % n_big
    Hb = np.zeros((m_big, n_big), np.uint8)
    Hb[rows, cols] = 1
    Hb[np.arange(n_big) % m_big, np.arange(n_big)] = 1      # (no empty column)
    big = fresh(Hb)
    for variant in VARIANTS:
        with pytest.raises(_lib.QbpError) as e:
            big.gd_configure(config(variant, 6))
        assert e.value.code == _lib.E_UNSUPPORTED
    assert b"160 KiB" in lib.qbp_last_error()


# ---- 6. end to end: mc.run_sweep and the command line ---------------------------------------------------------------------------
def test_run_sweep_and_cli_agree(tmp_path):
    cfg = dict(iters_per_round=8, max_rounds=6, decim_llr=25.0, variant=_lib.MIN_SUM, alpha=1.0, clip_llr=20.0)
    table = mc.run_sweep("[[72, 12, 6]]", [0.08], 3000, seed=3, max_iter=8, gd=cfg)
    assert table[0, 0] == 3000 and table[0, 6] >= 8
    bp_only = mc.run_sweep("[[72, 12, 6]]", [0.08], 3000, seed=3, max_iter=8)
    assert np.array_equal(table[0, [0, 6, 7]], bp_only[0, [0, 6, 7]]) and table[0, 10] < table[0, 6]
    out = tmp_path / "gd.json"
    subprocess.check_call([sys.executable, "-m", "qldpc_amd.mc", "--code", "[[72, 12, 6]]", "--p", "0.08", "--trials",
                           "3000", "--seed", "3", "--max-iter", "8", "--gd", "8", "6", "--gd-llr", "25", "--out",
                           str(out)], cwd=ROOT)
    rows = json.load(open(out))["points"]
    assert [rows[0][k] for k in _lib.COUNTER_NAMES[:11]] == table[0, :11].tolist()
