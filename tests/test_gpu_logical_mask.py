"""GPU: logical operators on bits 12 .. 63 of the logical mask, through every kernel that folds it.

A trial is a logical error when lm, the XOR of lx_cols[v] over the residual's support, is non-zero; bit l of lx_cols[v]
is Lx[l][v] (McInputs::prepare_lx of qbp.hip) and k may be 64.  Every kernel family folds lm across lanes in its own
way (64-bit LDS atomicXor, __shfl_xor ladders, a 64-bit slot inside a word array).  The placements of
tests/logical_mask_util.py move the rows of a base L to high bits; classification looks at lm != 0 alone, so

* `top`, `straddle` and `spread` must return what the base L returns, digit for digit -- counters, budget rows,
  spectrum tables and iteration histogram;
* `single(r, b)` and `k33` must return what L[r : r + 1] (k = 1, bit 0) returns;
* qbp_decode_shots must return the base predictions with their bits moved, and the same counters.

All runs of a family go through ONE handle, in an order where consecutive calls keep k = 64 and differ in one row,
with k = 12 followed by k = 13 on the same first 12 rows and k = 0 between two k = 64 calls: a stale lx_cols upload
(the byte-compare cache of prepare_lx) would show as well.  A kernel that lost bits 32 .. 63 would fail every one of
these equalities but those of `single(r, 31)`, the control on the last bit a 32-bit fold keeps
(tests/test_logical_mask_cpu.py shows that on the CPU oracle).

Inputs: p = 0.06, max_iter = 8, 1500 trials, seed 3 (logical_mask_util).  On the CPU oracle they give, BP only on
[[72,12,6]], [1] = 475, [6] = 380, [8] = 368, with OSD-0 [1] = 405, [8] = 298; fixed weight 5: 510 / 387 / 360; the
4-round phenomenological matrix: 1449 / 1486 / 1447; the irregular matrix: 476 / 477 / 472, with OSD-0 275 / 477 / 271.
The window decoder's numpy statement (tests/window_oracle.py on the CPU oracle, (W, F) = (3, 1), OSD-0) gives 1448 /
1499 / 1448 on the 6-round matrix, and 712 and 714 for the first two rows alone.
Every base run asserts the floors [1] >= 8, [6] >= 8 and [8] >= 8 ([8]: the trials BP did not converge on -- the records
handed to the second stage -- that end as logical errors), so no equality below is vacuous.  The second stages other
than OSD-0 have no CPU figure here; any decoder leaves a few per cent of logical errors on a distance-6 code at a mean
error weight of 4.3, and the floors are asserted all the same."""
import numpy as np
import pytest

import logical_mask_util as lm
from oracle import oracle
from qldpc_amd import _lib, bp, dem, mc, shots, window
from test_gpu_gd import config as gd_config
from test_gpu_osd_order_large import _forced
from test_gpu_relay import fresh_configured as relay_configured
from test_window_plan import matrix as window_matrix

pytestmark = pytest.mark.gpu

P, MAX_ITER, T, SEED = lm.P, lm.MAX_ITER, lm.TRIALS, lm.SEED
KW = dict(seed=SEED, max_iter=MAX_ITER)
BUDGETS = (2, 4, 8)
WEIGHT = 5


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def check_family(run, L, what, move=None, k0=True, k13=False):
    """`run(L') -> tuple of arrays`, the counters first: every placement of L through it, in the order of the module
    docstring, against the runs of the rows the placement keeps.  `move(outputs, bits)`: what the outputs of a run
    become when its rows go to `bits` (shots: the predictions); None: nothing changes.  Returns the outputs by name."""
    L = np.ascontiguousarray(L, np.uint8)
    n = L.shape[1]
    move = move or (lambda outs, bits: outs)
    out = {"base": run(L)}
    cnt = np.asarray(out["base"][0]).reshape(-1, _lib.NUM_COUNTERS)
    print(what, "base", cnt.tolist())
    assert (cnt[:, 0] == T).all(), (what, cnt)
    assert (cnt[:, 1] >= 8).all() and (cnt[:, 6] >= 8).all() and (cnt[:, 8] >= 8).all(), (what, cnt)
    if k13:
        out["k13"] = run(lm.extra_row(L))                  # k = 12, then k = 13 on the same first 12 rows
    maps = {}
    for name, Lp, m in lm.placements(L):
        out[name], maps[name] = run(Lp), m
        if name == "top":
            top = Lp
    if k0:
        out["k0"] = run(np.zeros((0, n), np.uint8))        # between two calls with k = 64
        out["top again"] = run(top)
    ones = {r: run(np.ascontiguousarray(L[r:r + 1])) for r in lm.SINGLE_ROWS}

    bad = []                                               # (every placement that differs, not the first alone)
    for name, m in maps.items():
        on = np.flatnonzero(m >= 0)
        ref = out["base"] if len(on) == L.shape[0] else ones[int(on[0])]
        if not same(out[name], move(ref, m[on])):
            bad.append((name, np.asarray(out[name][0]).tolist(), np.asarray(ref[0]).tolist()))
        elif len(on) == 1 and np.array_equal(out[name][0], out["base"][0]):
            bad.append((name, "the counters of the base run"))
    assert not bad, (what, [b[0] for b in bad], bad)
    for b in lm.SINGLE_BITS:
        assert not np.array_equal(out[f"single(0,{b})"][0], out[f"single(1,{b})"][0]), (what, b)
    if k0:
        none = np.asarray(out["k0"][0]).reshape(-1, _lib.NUM_COUNTERS)
        assert not none[:, lm.L_ONLY].any(), (what, none)
        assert np.array_equal(none[:, lm.L_FREE], cnt[:, lm.L_FREE]), (what, none)
        assert same(out["top again"], out["base"]), what
    if k13:
        more = np.asarray(out["k13"][0]).reshape(-1, _lib.NUM_COUNTERS)
        assert (more[:, 1] - cnt[:, 1] >= 8).all(), (what, more, cnt)        # (the CPU oracle: 489 against 475)
        assert same(out["k13"], run(np.ascontiguousarray(lm.extra_row(L)[::-1]))), what
    return out


def check_anchors(out, H, L, d, prior, what):
    """qbp_mc_run, BP only, against oracle.mc_counters on the same L': `top`, `single(0, 63)` and k = 0."""
    top = next(Lp for name, Lp, _ in lm.placements(L) if name == "top")
    for name, Lp in (("top", top), ("single(0,63)", lm.single(L, 0, 63)[1]), ("k0", np.zeros((0, L.shape[1]), np.uint8))):
        want = oracle.mc_counters(H, Lp, d, P, prior, 0, T, seed=SEED, max_iter=MAX_ITER)
        assert np.array_equal(out[name][0], want), (what, name, out[name][0], want)
    assert not out["k0"][0][list(lm.L_ONLY)].any()


# ---- 1. the on-chip kernel, <6, 3> ---------------------------------------------------------------------------------------
def test_on_chip_kernel_every_entry():
    H, L, d = lm.code72()
    n = H.shape[1]
    prior, probs = lm.prior_of(n), np.full(n, P)
    errors = oracle.mc_errors(n, P, 1, SEED, 0, T)
    dec = fresh(H)
    entries = {
        "mc_run": lambda Lp: (dec.mc_run(Lp, d, P, prior, 0, T, **KW),),
        "mc_run_probs": lambda Lp: (dec.mc_run_probs(Lp, d, probs, prior, 0, T, **KW),),
        "mc_run_errors": lambda Lp: (dec.mc_run_errors(Lp, d, errors, prior, max_iter=MAX_ITER),),
        "mc_run_budgets": lambda Lp: (dec.mc_run_budgets(Lp, d, probs, prior, BUDGETS, 0, T, seed=SEED),),
        "mc_run_spectrum": lambda Lp: dec.mc_run_spectrum(Lp, d, probs, prior, 0, T, **KW),
        "mc_run_weight": lambda Lp: (dec.mc_run_weight(Lp, d, WEIGHT, prior, 0, T, **KW),),
        "mc_run, forced": lambda Lp: (dec.mc_run(Lp, d, P, prior, 0, T, flags=_lib.FLAG_FORCE_FULL, **KW),),
    }
    outs = {}
    for what, run in entries.items():
        outs[what] = check_family(run, L, "on-chip " + what, k13=what == "mc_run")
        assert dec.info("last_kernel") == 1, what
    check_anchors(outs["mc_run"], H, L, d, prior, "on-chip")
    # the entries agree with each other where they state the same run
    for what in ("mc_run_probs", "mc_run_errors", "mc_run, forced"):
        assert np.array_equal(outs[what]["base"][0], outs["mc_run"]["base"][0]), what
    assert np.array_equal(outs["mc_run_budgets"]["base"][0][-1], outs["mc_run"]["base"][0])
    assert np.array_equal(outs["mc_run_spectrum"]["base"][0], outs["mc_run"]["base"][0])
    assert outs["mc_run_spectrum"]["base"][1].sum() > 0 and outs["mc_run_spectrum"]["base"][2].sum() == T


# ---- 2. the on-chip kernel, <8, 4> ---------------------------------------------------------------------------------------
def test_on_chip_kernel_wide_instantiation():
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 4, P, P)
    assert H.shape == (144, 432) and H.sum(axis=1).max() == 8
    prior = mc.dem_prior(probs)
    dec = fresh(H)
    check_family(lambda Lp: (dec.mc_run_probs(Lp, 6, probs, prior, 0, T, **KW),), L, "on-chip <8,4> mc_run_probs")
    assert dec.info("last_kernel") == 1


# ---- 3. the general-H kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["irregular", "72"])
def test_general_kernel(name):
    H, L, d = lm.irregular() if name == "irregular" else lm.code72()
    n = H.shape[1]
    prior, probs = lm.prior_of(n), np.full(n, P)
    dec = fresh(H)
    if name == "72":
        dec.set_option(_lib.OPT_KERNEL, _lib.KERNEL_GENERAL)
    out = check_family(lambda Lp: (dec.mc_run(Lp, d, P, prior, 0, T, **KW),), L, f"general-H {name} mc_run",
                       k13=name == "72")
    assert dec.info("last_kernel") == 2
    check_family(lambda Lp: (dec.mc_run_probs(Lp, d, probs, prior, 0, T, **KW),), L, f"general-H {name} mc_run_probs")
    assert dec.info("last_kernel") == 2
    if name == "72":
        check_anchors(out, H, L, d, prior, "general-H")


# ---- 4. OSD-0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [0, 1, 2, 3])
def test_osd0_kernels(big):
    H, L, d = lm.code72()
    prior = lm.prior_of(72)
    dec = fresh(H)
    dec.set_option(_lib.OPT_OSD_BIG, big)
    out = check_family(lambda Lp: (dec.mc_run(Lp, d, P, prior, 0, T, flags=_lib.FLAG_OSD0, **KW),), L, f"OSD-0 kernel {big}")
    want = oracle.mc_counters(H, L, d, P, prior, 0, T, seed=SEED, max_iter=MAX_ITER, osd=True)
    assert np.array_equal(out["base"][0][:len(want)], want)


def test_osd0_spectrum_build():
    H, L, d = lm.code72()
    prior, probs = lm.prior_of(72), np.full(72, P)
    dec = fresh(H)
    out = check_family(lambda Lp: dec.mc_run_spectrum(Lp, d, probs, prior, 0, T, flags=_lib.FLAG_OSD0, **KW), L,
                       "OSD-0 spectrum")
    _, spectrum, hist = out["base"]
    assert spectrum[1].sum() > 0 and spectrum[3].sum() >= 8 and hist.sum() == T


# ---- 5. order-w OSD -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["osd_order_kernel", "osd_order_blocked_kernel"])
def test_osd_order_kernels(kernel):
    H, L, d = lm.code72()
    prior = lm.prior_of(72)
    blocked = kernel == "osd_order_blocked_kernel"
    dec = _forced(H, 1) if blocked else fresh(H)
    flags = _lib.osd_flags("cs", 3, large=blocked)
    check_family(lambda Lp: (dec.mc_run(Lp, d, P, prior, 0, T, flags=flags, **KW),), L, "CS-3 " + kernel)


# ---- 6. the second stages, each after a flooding first stage ------------------------------------------------------------------
def second_stage(stage):
    H, _, _ = lm.code72()
    if stage == "relay":
        return relay_configured(H), _lib.FLAG_RELAY
    dec = fresh(H)
    if stage == "lsd":
        dec.lsd_configure(1)
        return dec, _lib.FLAG_LSD
    if stage == "gd":
        dec.gd_configure(gd_config(_lib.MIN_SUM, 6))
        return dec, _lib.FLAG_GD
    dec.layered_configure(None)
    return dec, _lib.FLAG_LAYERED | (_lib.FLAG_OSD0 if stage == "layered+osd0" else 0)


@pytest.mark.parametrize("stage", ["lsd", "relay", "gd", "layered", "layered+osd0"])
def test_second_stages(stage):
    H, L, d = lm.code72()
    prior = lm.prior_of(72)
    dec, flags = second_stage(stage)
    check_family(lambda Lp: (dec.mc_run(Lp, d, P, prior, 0, T, flags=flags, **KW),), L, stage)


# ---- 7. the sliding-window decoder ------------------------------------------------------------------------------------------------
def test_window_classify_kernel():
    H, cr = window_matrix("72")
    _, Lx, d = lm.code72()
    n = H.shape[1]
    L = np.concatenate([np.tile(Lx, 6), np.zeros((12, n - 6 * 72), np.uint8)], axis=1)    # [Lx ... Lx | 0]
    prior, probs = lm.prior_of(n), np.full(n, P)
    errors = oracle.mc_errors(n, P, 1, SEED, 0, T)
    wdec = window.decoder_for(H, cr, 3, 1)
    kw = dict(max_iter=MAX_ITER, flags=_lib.FLAG_OSD0)
    check_family(lambda Lp: (wdec.mc_run_errors(Lp, d, errors, prior, **kw),), L, "window mc_run_errors")
    check_family(lambda Lp: (wdec.mc_run_probs(Lp, d, probs, prior, 0, T, seed=SEED, **kw),), L, "window mc_run_probs")
    wdec.close()


# ---- 8. recorded shots -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _lib.FLAG_OSD0], ids=["bp", "osd0"])
@pytest.mark.parametrize("name", ["72", "irregular"])
def test_decode_shots(name, flags):
    H, L, _ = lm.code72() if name == "72" else lm.irregular()
    n = H.shape[1]
    prior = lm.prior_of(n)
    errors = oracle.mc_errors(n, P, 1, SEED, 0, T).astype(np.int64)
    det = shots.pack_bits(errors @ H.T.astype(np.int64) % 2)
    dec = fresh(H)

    def run(Lp):
        actual = shots.masks_of(errors @ Lp.T.astype(np.int64) % 2)
        return dec.decode_shots(Lp, det, prior, actual, max_iter=MAX_ITER, flags=flags)

    def move(outs, bits):
        return outs[0], lm.move_bits(outs[1], bits), outs[2]

    out = check_family(run, L, f"shots {name} {flags}", move=move, k0=False)
    assert dec.info("last_kernel") == (1 if name == "72" else 2)
    assert (out["single(0,63)"][1] >> np.uint64(63)).sum() >= 8 and out["top"][1].max() >= np.uint64(1) << np.uint64(52)
    # the recorded observables move the same way
    base_actual = shots.masks_of(errors @ L.T.astype(np.int64) % 2)
    for pname, Lp, m in lm.placements(L):
        assert np.array_equal(shots.masks_of(errors @ Lp.T.astype(np.int64) % 2), lm.move_bits(base_actual, m)), pname


# ---- k out of range ------------------------------------------------------------------------------------------------------------------
def test_k_out_of_range_is_refused_by_the_window_and_weight_entries():
    """k = 65 and k = -1: QBP_E_INVALID, the counters untouched -- host and device forms of qbp_window_mc_run_probs,
    qbp_window_mc_run_errors and qbp_mc_run_weight (the other entries: tests/test_gpu_shots.py and, through the shared
    check of the Monte-Carlo entries, tests/test_gpu_mc_entries.py)."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", bp.DEVICE)
    stream = torch.cuda.current_stream(dev).cuda_stream
    H, cr = window_matrix("steane")
    n = H.shape[1]
    wdec = window.decoder_for(H, cr, 3, 1)
    H72, L72, d = lm.code72()
    dec = fresh(H72)
    POISON = -7777
    for k in (65, -1):
        Lw, Lc = np.ones((65, n), np.uint8), np.ones((65, 72), np.uint8)
        pw, pc = lm.prior_of(n), lm.prior_of(72)
        probs = np.full(n, P)
        errors = np.zeros((4, n), np.uint8)
        cnt = np.full(_lib.NUM_COUNTERS, POISON, np.int64)
        d_cnt = torch.full((_lib.NUM_COUNTERS,), POISON, dtype=torch.int64, device=dev)
        d_pw, d_pc = torch.from_numpy(pw).to(dev), torch.from_numpy(pc).to(dev)
        tail = (MAX_ITER, 0, 1.0, 1.0, 20.0, 0)
        calls = {
            "window probs": lambda: lib.qbp_window_mc_run_probs(wdec._h, Lw.ctypes.data, k, 3, probs.ctypes.data, 1, SEED, 0,
                                                                100, pw.ctypes.data, *tail, cnt.ctypes.data),
            "window probs, device": lambda: lib.qbp_window_mc_run_probs_device(
                wdec._h, Lw.ctypes.data, k, 3, probs.ctypes.data, 1, SEED, 0, 100, d_pw.data_ptr(), *tail, d_cnt.data_ptr(),
                stream),
            "window errors": lambda: lib.qbp_window_mc_run_errors(wdec._h, Lw.ctypes.data, k, 3, errors.ctypes.data, 4,
                                                                  pw.ctypes.data, *tail, cnt.ctypes.data),
            "weight": lambda: lib.qbp_mc_run_weight(dec._h, Lc.ctypes.data, k, d, WEIGHT, SEED, 0, 100, pc.ctypes.data,
                                                    *tail, cnt.ctypes.data),
            "weight, device": lambda: lib.qbp_mc_run_weight_device(dec._h, Lc.ctypes.data, k, d, WEIGHT, SEED, 0, 100,
                                                                   d_pc.data_ptr(), *tail, d_cnt.data_ptr(), stream),
        }
        for what, call in calls.items():
            assert call() == _lib.E_INVALID, (k, what)
            assert b"logical operators" in lib.qbp_last_error(), (k, what, lib.qbp_last_error())
            torch.cuda.synchronize(dev)
            assert np.all(cnt == POISON) and bool((d_cnt == POISON).all()), (k, what)
    # the handles are as they were: k = 64 goes through
    L64 = lm.single(L72, 0, 63)[1]
    assert dec.mc_run_weight(L64, d, WEIGHT, lm.prior_of(72), 0, 100, **KW)[0] == 100
    assert wdec.mc_run_probs(np.ones((64, n), np.uint8), 3, np.full(n, P), lm.prior_of(n), 0, 100, **KW)[0] == 100
    wdec.close()
