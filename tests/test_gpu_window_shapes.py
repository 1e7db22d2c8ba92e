"""GPU: the sliding-window decoder (qbp_window_*) beyond one pass of its glue kernels' grid-stride loops, and on the
options of its call surface that tests/test_gpu_window.py leaves alone.

The reference is always the numpy statement tests/window_oracle.py composed from separate ordinary Decoders on the H_k
(``Parts`` of tests/test_gpu_window.py); records are independent, so the statement on a subset of the rows is that subset
of the statement.  Monte-Carlo counters are compared with window_shapes_util.classify of the statement's outputs, never
of the window decoder's own.  Every comparison is exact (NaN equal to NaN for llr).

A. window_grid() gives a launch at most 2048 blocks of 256 lanes: 524288 items a pass, 8192 records for the two
   wavefront-per-record kernels.  tests/test_gpu_window.py decodes 257 records, so every loop there ends in its first
   trip.  Here 60000 records of the 18 x 60 steane matrix make window_gather_kernel, both window_commit_kernel forms,
   window_syndrome_kernel and window_classify_kernel come round again in every window, and 524288 + 4099 records
   window_fail_list_kernel; tests/test_window_shapes_cpu.py states the arithmetic from the plan alone.
   One loop stays single-pass in the suite: window_gather_prior_kernel strides from a sum of |U_k| above 524288 on,
   sub-matrices of several hundred thousand variables.  Its index is an int and the plan bounds that sum at 2^28.
B. QBP_DAMPED_SP, QBP_FLAG_FORCE_FULL, OSD method E, QBP_FLAG_OSD_LARGE, window classes on the general-H kernel,
   qbp_window_set_option forwarding, qbp_window_mc_run_probs_device, and one decoder whose batch grows between calls."""
import time

import numpy as np
import pytest

import window_oracle as wo
import window_shapes_util as ws
from qldpc_amd import _lib, bp
from test_gpu_window import ALPHA, CLIP, DAMPING, MAX_ITER, Parts, big, device_call, same, wdec  # noqa: F401 (big: a fixture)
from test_window_plan import P_OF, matrix
from window_shapes_util import GRID_LANES, GRID_WAVES, SIZES

pytestmark = pytest.mark.gpu

OSD0 = ("cs", 0, False)
ALL_VARIANTS = {"sum_product": _lib.SUM_PRODUCT, "damped_sp": _lib.DAMPED_SP, "min_sum": _lib.MIN_SUM}


def flags_of(osd):
    return 0 if osd is None else _lib.osd_flags(*osd)


def tag(osd):
    return "none" if osd is None else "osd0" if osd[1] == 0 else f"{osd[0]}{osd[1]}{'L' if osd[2] else ''}"


class PartsW(Parts):
    """``Parts`` with the second stage spelled (method, order, large), or None."""

    def __init__(self, variant, osd=None, max_iter=MAX_ITER):
        super().__init__(variant, "none" if osd is None else "osd", max_iter)
        self.second = osd

    def osd(self, Hk, syn, llr, hard):
        method, order, large = self.second
        d = self.dec(Hk)
        return d.osd0(syn, llr, hard) if order == 0 else d.osd(syn, llr, hard, method, order, large=large)


def run(d, syn, prior, variant, osd, extra=0, **kw):
    return d.decode(syn, prior, MAX_ITER, variant, ALPHA, DAMPING, CLIP, flags_of(osd) | extra, **kw)


def run_fresh(H, cr, W, F, syn, prior, variant, osd):
    """One call on a decoder of its own, closed afterwards."""
    d = wdec(H, cr, W, F)
    try:
        return run(d, syn, prior, variant, osd)
    finally:
        d.close()


GEOMETRY = ("last_kernel", "one_barrier", "threads", "lds_bytes", "grid")


def geometry(d, *index):
    """The launch geometry a handle's last BP launch left: of a class of a window decoder, or of an ordinary Decoder."""
    return tuple(d.info(key, *index) for key in GEOMETRY)


@pytest.fixture(scope="module")
def long_batch():
    """A1 and B10: the 60000 steane records and the min-sum statement on them for both sizes, with OSD-0 and without.
    Computed once for the module, never written to, released with it."""
    H, cr, _, syn, prior = ws.inputs("steane", ws.STRIDE_B, ws.STRIDE_SEED)
    want = {(W, F, osd): PartsW(_lib.MIN_SUM, osd).statement(H, cr, W, F, syn, prior)
            for W, F in SIZES for osd in (None, OSD0)}
    return H, cr, syn, prior, want


def test_the_constants_are_those_of_the_window_tests():
    assert (MAX_ITER, ALPHA, DAMPING, CLIP) == (ws.MAX_ITER, ws.ALPHA, ws.DAMPING, ws.CLIP)


# ---- A1. decode beyond one grid pass -------------------------------------------------------------------------------------
@pytest.mark.parametrize("osd", [None, OSD0], ids=tag)
@pytest.mark.parametrize("W,F", SIZES)
def test_decode_beyond_one_grid_pass(long_batch, W, F, osd):
    """B = 60000 records of steane (18 x 60, six rounds).  (3, 1): four windows of 9 checks, 540000 gather lanes and
    60000 x 17 (60000 x 40 in the last window) commit items; (4, 2): two windows of 12 checks, 720000 gather lanes,
    60000 x 30 and 60000 x 53 commit items -- every window of both passes 524288, and 60000 records pass the 8192 of
    window_commit_kernel<true>, so B needs no raising for (4, 2)."""
    B = ws.STRIDE_B
    H, cr, syn, prior, statements = long_batch
    later = ws.assert_every_loop_strides(B, H, cr, W, F)
    assert GRID_WAVES < later < B - 8
    want = statements[W, F, osd]
    # the records a later pass owns are of every kind: dropping or duplicating a pass changes what is compared
    for first in (GRID_WAVES, later):
        ws.assert_kinds([a[first:] for a in want], osd, f"({W}, {F}) {tag(osd)} rows {first} .. {B}")
    d = wdec(H, cr, W, F)
    got = run(d, syn, prior, _lib.MIN_SUM, osd)
    same([a[later:] for a in got], [a[later:] for a in want], ("beyond the first pass", W, F, tag(osd)))
    same(got, want, (W, F, tag(osd), B))
    d.close()


# ---- A2, A3. Monte-Carlo beyond one grid pass ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc_case():
    """A2 and A3: (H, cr, L, probs, prior, errors, {osd: (want, head)}) -- T = 60000 trials of the probs sampler, the
    classification of the statement on them, and of its first 8192 trials alone.  Once for the module."""
    H, cr = matrix("steane")
    p = P_OF["steane"]
    L, probs = ws.mc_inputs()
    prior = np.full(H.shape[1], np.log((1 - p) / p))
    plain = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    errors = plain.mc_sample_errors_probs(probs, ws.MC_BEGIN, ws.MC_T, draws=2, seed=ws.MC_SEED)
    plain.close()
    counts, g = {}, GRID_WAVES
    for osd in (None, OSD0):
        x, conv, iters, _, fails = PartsW(_lib.MIN_SUM, osd).statement(H, cr, 3, 1, ws.syndromes_of(H, errors), prior)
        want, valid = ws.classify(H, L, ws.MC_DISTANCE, errors, x, iters, fails)
        assert np.array_equal(valid, conv)
        counts[osd] = want, ws.classify(H, L, ws.MC_DISTANCE, errors[:g], x[:g], iters[:g], fails[:g])[0]
    return H, cr, L, probs, prior, errors, counts


def mc_args(osd):
    return dict(max_iter=MAX_ITER, variant=_lib.MIN_SUM, alpha=ALPHA, damping=DAMPING, clip_llr=CLIP, flags=flags_of(osd))


@pytest.mark.parametrize("osd", [None, OSD0], ids=tag)
def test_mc_beyond_one_grid_pass(mc_case, osd):
    """T = 60000 trials in ONE chunk (the default holds 2^20): window_classify_kernel makes an eighth trip (one trial per
    wavefront, 8192 a pass), window_syndrome_kernel a third (T m = 1080000 lanes), and every kernel of the decode strides
    as in A1.  Fifteen chunks of 4099 trials, none of which strides, must count the same."""
    H, cr, L, probs, prior, errors, counts = mc_case
    want, head = counts[osd]
    T, n, m = ws.MC_T, H.shape[1], H.shape[0]
    assert T <= (1 << 28) // n and T <= 1 << 20                       # one chunk
    assert 7 * GRID_WAVES < T and T * m > GRID_LANES
    ws.assert_every_loop_strides(T, H, cr, 3, 1)
    print(f"classify {T} trials against {GRID_WAVES}, syndromes {T} x {m} = {T * m} lanes against {GRID_LANES}")
    print("want", want.tolist(), "beyond the first pass", (want - head).tolist())
    assert want[0] == T and all((want - head)[i] >= 5 for i in (1, 6, 9) + (() if osd else (10,))), (want, head)
    d = wdec(H, cr, 3, 1)
    begin, end, args = ws.MC_BEGIN, ws.MC_BEGIN + T, mc_args(osd)
    stored = lambda: d.mc_run_errors(L, ws.MC_DISTANCE, errors, prior, **args)
    drawn = lambda a=begin, b=end, **kw: d.mc_run_probs(L, ws.MC_DISTANCE, probs, prior, a, b, draws=2, seed=ws.MC_SEED,
                                                        **args, **kw)
    got = stored()
    assert np.array_equal(got, want), (got, want)
    got = drawn()
    assert np.array_equal(got, want), (got, want)
    cut = begin + 30001
    split = drawn(begin, cut)
    drawn(cut, end, counters=split)
    assert np.array_equal(split, want), (split, want)
    try:
        d.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 4099)
        assert 14 * 4099 < T <= 15 * 4099 and 4099 <= GRID_WAVES and 4099 * 40 <= GRID_LANES
        assert np.array_equal(stored(), want)
        assert np.array_equal(drawn(), want)
    finally:
        d.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)
    assert np.array_equal(stored(), want)
    assert np.array_equal(drawn(), want)
    d.close()


@pytest.mark.parametrize("osd", [None, OSD0], ids=tag)
def test_mc_device_entry_on_a_side_stream(mc_case, osd):
    """qbp_window_mc_run_probs_device: device prior and counters, a side stream, the T of the test above.  The
    counters are ADDED to (prefilled with 1000 ..), and the int64 on either side of them stays as it was."""
    import torch
    H, cr, L, probs, prior, _, counts = mc_case
    want = counts[osd][0]
    dev = torch.device("cuda", bp.DEVICE)
    d = wdec(H, cr, 3, 1)
    d_prior = torch.from_numpy(prior).to(dev)
    prefill = np.arange(12, dtype=np.int64) + 1000
    buf = torch.full((14,), -7777, dtype=torch.int64, device=dev)
    buf[1:13] = torch.from_numpy(prefill).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for calls in (1, 2):
        d.mc_run_probs_device(L, ws.MC_DISTANCE, probs, d_prior.data_ptr(), ws.MC_BEGIN, ws.MC_BEGIN + ws.MC_T,
                              buf[1:].data_ptr(), draws=2, seed=ws.MC_SEED, stream=side.cuda_stream, **mc_args(osd))
        side.synchronize()
        host = buf.cpu().numpy()
        assert host[0] == -7777 and host[13] == -7777
        assert np.array_equal(host[1:13], prefill + calls * want), (calls, host, want)
    d.close()


# ---- A4. the failure list beyond one grid pass ------------------------------------------------------------------------------
def test_failure_list_beyond_one_grid_pass():
    """B = 524288 + 4099 records in one decode call, steane (3, 1), OSD-0, no llr: window_fail_list_kernel takes one
    record per lane, so its 4099 last records belong to a second trip.  The order of the list depends on the order the
    lanes arrive in and no output may: the statement is compared on every row from 524288 - 4099 on and on every 64th
    below (8128 + 8198 rows).  Measured on an MI355X: 0.4 s for the whole test, so no row below 524288 was thinned."""
    t0 = time.perf_counter()
    B = ws.LIST_B
    H, cr, _, syn, prior = ws.inputs("steane", B, ws.LIST_SEED)
    assert B > GRID_LANES
    print(f"fail list {B} records against {GRID_LANES} lanes")
    d = wdec(H, cr, 3, 1)
    t1 = time.perf_counter()
    x, conv, iters, llr, fails = run(d, syn, prior, _lib.MIN_SUM, OSD0, want_llr=False)
    t2 = time.perf_counter()
    assert llr is None
    rows = ws.list_rows()
    want = PartsW(_lib.MIN_SUM, OSD0).statement(H, cr, 3, 1, syn[rows], prior)
    beyond = rows >= GRID_LANES
    plain = PartsW(_lib.MIN_SUM, None).statement(H, cr, 3, 1, syn[rows[beyond]], prior)
    second = want[4][beyond] > 0
    changed = second & (want[0][beyond] != plain[0]).any(axis=1)
    print(f"rows beyond {GRID_LANES}: {int(second.sum())} with a second stage, {int(changed.sum())} of them changed by it; "
          f"all compared rows: second stage {int((want[4] > 0).sum())} of {rows.size}")
    assert second.sum() >= 8 and changed.sum() >= 1          # an unlisted failure would show
    for got, w, name in zip((x, conv, iters, fails), (want[0], want[1], want[2], want[4]),
                            ("correction", "converged", "iters", "window_fails")):
        bad = np.flatnonzero((got[rows] != w).reshape(rows.size, -1).any(axis=1))
        assert bad.size == 0, (name, rows[bad][:8], bad.size)
    d.close()
    print(f"wall time: the decode call {t2 - t1:.2f} s, the whole test {time.perf_counter() - t0:.2f} s")


# ---- B5. QBP_DAMPED_SP -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("osd", [None, OSD0], ids=tag)
@pytest.mark.parametrize("name", ["72", "irregular"])
def test_damped_sum_product(name, osd):
    H, cr, _, syn, prior = ws.inputs(name, 257, 5)
    parts = PartsW(_lib.DAMPED_SP, osd)
    for W, F in SIZES:
        want = parts.statement(H, cr, W, F, syn, prior)
        print(f"{name} damped_sp {tag(osd)} ({W}, {F}): kinds", ws.kinds(want))
        assert (want[4] > 0).sum() >= 8 and (want[4] == 0).sum() >= 8
        same(run_fresh(H, cr, W, F, syn, prior, _lib.DAMPED_SP, osd), want, (name, tag(osd), W, F))


# ---- B6. QBP_FLAG_FORCE_FULL --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", list(ALL_VARIANTS))
@pytest.mark.parametrize("name", ["72", "steane"])
def test_force_full_changes_no_output(name, vname):
    """A forced launch runs all max_iter iterations and keeps the outputs of the first converged one: every output
    equals the unforced call's and the statement's, with and without OSD-0.
    The outputs alone do not show that the bit reached a sub-handle; the launch geometry does.  A forced on-chip launch
    has no first-step table in LDS (and other slots per workgroup), so after the forced window call every class reports
    the geometry an ordinary Decoder on its H_k reports after its own forced decode of as many records, and not the
    geometry of the unforced call.  The steane windows have rows of at most 6 and columns of at most 3 entries, the
    narrow build of the kernel: there a forced launch, and no other, is the one-barrier kernel.  The windows of "72"
    have rows of 8 entries, the wide build, which has no one-barrier form.  (4, 3) adds a second class."""
    H, cr, _, syn, prior = ws.inputs(name, 257, 5)
    variant = ALL_VARIANTS[vname]
    FORCE = _lib.FLAG_FORCE_FULL
    for W, F in SIZES + ((4, 3),):
        d = wdec(H, cr, W, F)
        P = wo.plan(H, cr, W, F)
        wins = list(wo.windows(H, P))
        classes = range(d.info("classes"))
        assert len(classes) == (2 if (W, F) == (4, 3) else 1) == int(P["cls"].max()) + 1
        # the ordinary decoder of every class, on the first window of the class: unforced, then forced
        plain = {}
        for c in classes:
            C, U, _, Hk = wins[int(np.flatnonzero(P["cls"] == c)[0])]
            dec = _lib.Decoder(*bp.csr_from_H(Hk), bp.DEVICE)
            for extra in (0, FORCE):
                dec.decode(np.ascontiguousarray(syn[:, C]), np.ascontiguousarray(prior[U]), MAX_ITER, variant, ALPHA, DAMPING,
                           CLIP, extra)
                plain[c, extra] = geometry(dec)
            dec.close()
        for osd in (None, OSD0):
            want = PartsW(variant, osd).statement(H, cr, W, F, syn, prior)
            assert (want[4] > 0).sum() >= 8 and (want[4] == 0).sum() >= 8
            unforced = run(d, syn, prior, variant, osd)
            seen = {(c, 0): geometry(d, c) for c in classes}
            forced = run(d, syn, prior, variant, osd, FORCE)
            seen.update({(c, FORCE): geometry(d, c) for c in classes})
            for c in classes:
                print(f"{name} {vname} {tag(osd)} ({W}, {F}) class {c} {GEOMETRY}: unforced {seen[c, 0]}, forced "
                      f"{seen[c, FORCE]}")
                assert seen[c, FORCE] == plain[c, FORCE] and seen[c, 0] == plain[c, 0], (c, seen, plain)
                assert seen[c, FORCE] != seen[c, 0] and seen[c, FORCE][0] == 1
                assert seen[c, FORCE][3] != seen[c, 0][3]                                # lds_bytes: the first-step table
                assert (seen[c, 0][1], seen[c, FORCE][1]) == ((0, 1) if name == "steane" else (0, 0))     # one_barrier
            same(forced, unforced, ("forced against unforced", name, vname, tag(osd), W, F))
            same(forced, want, ("forced against the statement", name, vname, tag(osd), W, F))
        d.close()


# ---- B7. OSD method E and QBP_FLAG_OSD_LARGE ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72", "irregular"])
def test_osd_method_e(name):
    osd = ("e", 4, False)
    H, cr, _, syn, prior = ws.inputs(name, 257, 5)
    for vname in ("min_sum", "sum_product"):
        parts = PartsW(ALL_VARIANTS[vname], osd)
        for W, F in SIZES:
            want = parts.statement(H, cr, W, F, syn, prior)
            print(f"{name} {vname} e4 ({W}, {F}): kinds", ws.kinds(want))
            assert (want[4] > 0).sum() >= 8
            same(run_fresh(H, cr, W, F, syn, prior, ALL_VARIANTS[vname], osd), want, (name, vname, "e4", W, F))


BIG_P = 0.012


def test_osd_large_on_the_864_row_windows(big):  # noqa: F811
    """The call tests/test_gpu_window.py shows refused without the flag: order-w OSD (cs, order 2) on the 864 x 2592
    windows, against the ordinary decoder's qbp_osd_batch with the same flags on H_k."""
    H, _, _, cr, d = big
    osd = ("cs", 2, True)
    errors = (np.random.default_rng(3).random((64, 7776)) < BIG_P).astype(np.uint8)
    syn = ws.syndromes_of(H, errors)
    prior = np.full(7776, np.log((1 - BIG_P) / BIG_P))
    want = PartsW(_lib.SUM_PRODUCT, osd).statement(H, cr, 6, 3, syn, prior)
    print("864 x 2592 windows, cs2 large: window_fails", np.bincount(want[4]).tolist(), "kinds", ws.kinds(want))
    assert (want[4] > 0).sum() >= 8
    same(run(d, syn, prior, _lib.SUM_PRODUCT, osd), want, "2592 x 7776, QBP_FLAG_OSD_LARGE")


# ---- B8. window classes on the general-H kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("make,kinds", [(ws.heavy_everywhere, [2]), (ws.heavy_last_round, [1, 2])],
                         ids=["every window", "the last window"])
def test_window_classes_on_the_general_kernel(make, kinds):
    """Rows of weight 9 and more do not fit the on-chip kernel (at most 8 entries a row): in every window, or only in
    the windows that hold the last round -- a decoder whose classes run different kernels."""
    H, cr, _, syn, prior = ws.heavy_inputs(make)
    for W, F in SIZES:
        d = wdec(H, cr, W, F)
        got_kinds = [d.info("kernel_kind", c) for c in range(d.info("classes"))]
        print(f"{make.__name__} ({W}, {F}): windows {d.info('windows')}, kernel kind per class {got_kinds}")
        assert got_kinds == kinds
        for vname in ("min_sum", "sum_product"):
            for osd in (None, OSD0):
                want = PartsW(ALL_VARIANTS[vname], osd).statement(H, cr, W, F, syn, prior)
                print(f"  {vname} {tag(osd)}: kinds", ws.kinds(want))
                assert (want[4] > 0).sum() >= 8 and (want[4] == 0).sum() >= 8
                same(run(d, syn, prior, ALL_VARIANTS[vname], osd), want, (make.__name__, vname, tag(osd), W, F))
                assert [d.info("last_kernel", c) for c in range(len(kinds))] == kinds
        d.close()


# ---- B9. qbp_window_set_option forwards -------------------------------------------------------------------------------------------
def test_set_option_reaches_every_sub_handle():
    """(4, 3) beside the two usual sizes: two window classes (a shorter last window), so "every" is more than one."""
    H, cr, _, syn, prior = ws.inputs("72", 257, 5)
    lib = _lib.load()
    for W, F in SIZES + ((4, 3),):
        d = wdec(H, cr, W, F)
        classes = range(d.info("classes"))
        assert len(classes) == (2 if (W, F) == (4, 3) else 1)
        want = {osd: PartsW(_lib.MIN_SUM, osd).statement(H, cr, W, F, syn, prior) for osd in (None, OSD0)}   # on defaults

        def check(what, kind):
            for osd in (None, OSD0):
                same(run(d, syn, prior, _lib.MIN_SUM, osd), want[osd], (what, W, F, tag(osd)))
            seen = [(d.info("kernel_kind", c), d.info("last_kernel", c), d.info("threads", c)) for c in classes]
            print(f"72 ({W}, {F}) {what}: (kernel_kind, last_kernel, threads) per class {seen}")
            assert all(s[:2] == (kind, kind) for s in seen), (what, seen)
            return [s[2] for s in seen]
        auto = check("defaults", 1)
        d.set_option(_lib.OPT_KERNEL, _lib.KERNEL_GENERAL)
        check("OPT_KERNEL = 2", 2)
        d.set_option(_lib.OPT_KERNEL, _lib.KERNEL_AUTO)
        assert check("OPT_KERNEL = 0", 1) == auto
        d.set_option(_lib.OPT_SLOTS_PER_BLOCK, 1)
        one = check("OPT_SLOTS_PER_BLOCK = 1", 1)
        # one record per workgroup: its m_k threads rounded up to wavefronts (the default packs at least as many)
        assert one == [-(-d.info("m", c) // 64) * 64 for c in classes] and all(a >= b for a, b in zip(auto, one))
        d.set_option(_lib.OPT_SLOTS_PER_BLOCK, 0)
        # what a sub-handle refuses comes back through the window call, and changes nothing
        for option, value in ((_lib.OPT_KERNEL, 7), (_lib.OPT_SLOTS_PER_BLOCK, 1025), (_lib.OPT_GENERAL_THREADS, -1),
                              (9999, 1)):
            assert lib.qbp_window_set_option(d._h, option, value) == _lib.E_INVALID, (option, value)
            with pytest.raises(_lib.QbpError) as e:
                d.set_option(option, value)
            assert e.value.code == _lib.E_INVALID
        assert check("after the refusals", 1) == auto
        d.close()


# ---- B10. one decoder, growing batches ----------------------------------------------------------------------------------------------
STEPS = [(1, 5), (257, 5), (ws.STRIDE_B, ws.STRIDE_SEED), (257, 6)]         # (records, seed of the inputs)


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("first", [OSD0, None], ids=["osd0 throughout", "osd0 from the third call"])
def test_one_decoder_growing_batches(long_batch, first, entry):
    """The workspaces of a qbp_window are reserved per call for that call's B: 1, 257, 60000 records, then 257 others,
    on ONE decoder -- and, in the second sequence, OSD-0 only from the call on that also grows them, so d_sol and
    d_fail_list are first reserved on a used object.  Every result equals a fresh decoder's and the statement."""
    import torch
    H, cr, long_syn, prior, long_want = long_batch
    d = wdec(H, cr, 3, 1)
    stream = torch.cuda.Stream(torch.device("cuda", bp.DEVICE)) if entry == "device" else None
    for step, (batch, seed) in enumerate(STEPS):
        osd = first if step < 2 else OSD0
        if batch == ws.STRIDE_B:
            syn, want = long_syn, long_want[3, 1, osd]
        else:
            syn = ws.inputs("steane", batch, seed)[3]
            want = PartsW(_lib.MIN_SUM, osd).statement(H, cr, 3, 1, syn, prior)
        fresh = run_fresh(H, cr, 3, 1, syn, prior, _lib.MIN_SUM, osd)
        same(fresh, want, ("a fresh decoder", tag(osd), batch))
        if entry == "host":
            got = run(d, syn, prior, _lib.MIN_SUM, osd)
        else:
            got, _ = device_call(d, syn, prior, flags_of(osd), stream)      # (poisoned, one element of slack either side)
            got[1] = got[1].astype(bool)
        print(f"{entry} step {step}: B = {batch}, {tag(osd)}, kinds {ws.kinds(got)}")
        same(got, fresh, (entry, "the grown decoder", step, tag(osd), batch))
    d.close()
