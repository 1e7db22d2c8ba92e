"""GPU: lsd_large_kernel (QBP_OPT_LSD_MEM; the rows of the active checks in a global workspace) against the numpy
statement of localized statistics decoding (tests/lsd_oracle.py) and against lsd_kernel, bit for bit: forced on the
small matrices, past each limit of the LDS kernel (bytes: 612 x 1836, 864 x 2592, 1008 x 8991; rows: 2049 x 384),
a workspace slice that serves a heavy record and then light ones, independence of the batch size, the grid, the stream
and an earlier configuration into poisoned buffers, the records build behind QBP_FLAG_LSD, and the refusals."""
import functools
import os
import sys

import numpy as np
import pytest

import geometry_util as gu
import lsd_oracle as lo
import lsd_util as lu
import record_kernel_util as ru
import test_gpu_lsd as tl
import test_lsd_large_cpu as tc
from oracle import oracle
from qldpc_amd import _lib, bp, codes, lsd, mc
from test_gpu_lsd_sizes import SOL_POISON, STAT_POISON, bp_records, make_special

pytestmark = pytest.mark.gpu

G = (0, 1, 3)
MEM_LDS, MEM_LARGE, MEM_AUTO = tc.MEM_LDS, tc.MEM_LARGE, tc.MEM_AUTO
# matrix, p of the BP(50) inputs, records (tests/test_gpu_lsd.py's cases but [[288,12,18]])
SMALL = [("steane", 0.2, 48), ("72", 0.08, 64), ("74", 0.08, 48), ("rand37", 0.08, 48), ("rows70", 0.003, 64),
         ("144", 0.07, 48)]


def fresh(H, mem=None):
    dec = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    if mem is not None:
        dec.set_option(_lib.OPT_LSD_MEM, mem)
    return dec


def device_lsd(dec, inputs, stream=0, stats=True, solution=True):
    """One qbp_lsd_batch_device into poisoned outputs with a spare record behind each, which must keep the poison."""
    t = gu.torch()
    syn_t, llr_t, hard_t = (gu.to_device(np.ascontiguousarray(a)) for a in inputs)
    B, n = len(inputs[0]), inputs[1].shape[1]
    sol_t = t.full((B + 1, n), SOL_POISON, dtype=t.uint8, device="cuda")
    st_t = t.full((B + 1, 4), STAT_POISON, dtype=t.int32, device="cuda")
    t.cuda.synchronize()
    dec.lsd_device(syn_t.data_ptr(), llr_t.data_ptr(), hard_t.data_ptr(), B, sol_t.data_ptr() if solution else 0,
                   st_t.data_ptr() if stats else 0, stream=stream or gu.stream_ptr())
    t.cuda.synchronize()
    assert bool((sol_t[B] == SOL_POISON).all()) and bool((st_t[B] == STAT_POISON).all()), "written beyond record B"
    return sol_t[:B].cpu().numpy(), st_t[:B].cpu().numpy()


def large_info(H, B, num_cu, blocks=0):
    m, n = H.shape
    return dict(threads=tc.THREADS, grid=tc.lsd_large_grid(m, n, B, num_cu, blocks), lds_bytes=tc.lsd_large_lds_bytes(m, n))


def assert_equal(got, want, what, rows=slice(None)):
    sol, stats = got
    assert np.array_equal(stats, want["stats"][rows]), (what, np.flatnonzero((stats != want["stats"][rows]).any(1))[:8])
    assert np.array_equal(sol, want["solution"][rows]), (what, np.flatnonzero((sol != want["solution"][rows]).any(1))[:8])


# =========================================================================================================================
# 1. the forced large build on the small cases
# =========================================================================================================================
@functools.lru_cache(maxsize=None)
def small_inputs(name):
    """BP(50) outputs with the four special records of tests/test_gpu_lsd.py (ties and a NaN, a zero residual, two
    syndromes with a flipped bit), and the failures first."""
    p, B = next((p, B) for n_, p, B in SMALL if n_ == name)
    H = lu.matrix(name)
    syn, llr, hard, conv = lu.bp_outputs(H, p, 3, B, 50)
    f = np.flatnonzero(~conv)
    assert len(f) >= 4, (name, len(f))
    order = np.concatenate([f, np.flatnonzero(conv)])
    return (H,) + make_special(H, syn[order], llr[order], hard[order])


@functools.lru_cache(maxsize=None)
def small_ref(name, g):
    H, syn, llr, hard = small_inputs(name)
    return lo.lsd_decode_batch(H, syn, llr, hard, g)


@pytest.mark.parametrize("g", G)
@pytest.mark.parametrize("name", [c[0] for c in SMALL])
def test_forced_large_build_equals_statement_and_lds_kernel(name, g):
    H, syn, llr, hard = small_inputs(name)
    want = small_ref(name, g)
    print(name, g, lo.presence(want))
    dec = fresh(H, MEM_LARGE)
    dec.lsd_configure(g, large="force")
    got = device_lsd(dec, (syn, llr, hard))
    assert ru.info(dec) == large_info(H, len(syn), dec.info("num_cu"))
    assert_equal(got, want, (name, g))
    # the LDS kernel on the same handle, then the host entry and the Python front under "force"
    dec.lsd_configure(g, large=False)
    lds = device_lsd(dec, (syn, llr, hard))
    assert dec.info("threads") == 64 and np.array_equal(lds[0], got[0]) and np.array_equal(lds[1], got[1])
    sol, stats = dec.lsd(syn, llr, hard, g, large="force")
    assert dec.info("threads") == tc.THREADS and np.array_equal(sol, got[0]) and np.array_equal(stats, got[1])
    res = lsd.performLSDBatch(H, syn[:6], llr[:6], hard[:6], g, large="force")
    assert np.array_equal(res[0], want["solution"][:6]) and np.array_equal(res[1], want["stats"][:6])
    assert np.array_equal(lsd.performLSD(H, syn[2], llr[2], hard[2], g, large=True), want["solution"][2])


def test_small_inputs_cover_the_situations():
    """From the statement's stats: a record solved in one round, one that merges two clusters, one with valid = 0."""
    one_round = merged = invalid = 0
    for name, _, _ in SMALL:
        for g in G:
            w = small_ref(name, g)
            one_round += int(((w["stats"][:, 0] == 1) & (w["stats"][:, 3] == 1)).sum())
            merged += int(w["merged"].sum())
            invalid += int((w["stats"][:, 3] == 0).sum())
    print(one_round, merged, invalid)
    assert one_round >= 1 and merged >= 1 and invalid >= 1


# =========================================================================================================================
# 2. past each limit of the LDS kernel
# =========================================================================================================================
def failures_of(c, iters, count):
    """The first `count` records of a case the CPU oracle's BP(iters) fails on -> (syn, llr, hard)."""
    llr, hard, conv = bp_records(c.H, c.syn, c.prior, iters)
    f = np.flatnonzero(~conv)[:count]
    assert len(f) == count, (len(f), count)
    return c.syn[f], llr[f], hard[f]


# The statement takes more than five seconds on these two (one record of 612 x 1836 runs 720 rounds at g = 1): its
# records (BP outputs: make_inputs) and the statement's outputs on them are stored by tests/golden/make_lsd_large_refs.py
GOLDEN_TAGS = ("ph72x17", "rows2049")
GOLDEN_KEYS = ("solution", "stats", "merged", "skipped")
GOLDEN_PATH = os.path.join(tl.ROOT, "tests", "golden", "lsd_large_refs.npz")


@functools.lru_cache(maxsize=None)
def ph17():
    return ru.phenomenological(17, 0.01, 117, 96)


@functools.lru_cache(maxsize=None)
def beyond_inputs(tag):
    """(H, syn, llr, hard) of a case; the records of the two stored cases are the stored ones."""
    made = make_inputs(tag) if tag not in GOLDEN_TAGS else (make_inputs(tag, matrix_only=True),)
    if tag in GOLDEN_TAGS:
        with np.load(GOLDEN_PATH) as z:
            made += tuple(z[f"{tag}_{k}"] for k in ("syn", "llr", "hard"))
    return made


def make_inputs(tag, matrix_only=False):
    if matrix_only:
        return ph17().H if tag == "ph72x17" else lu.rows2048(True)
    if tag == "ph72x17":                                     # 612 x 1836: one round beyond the LDS kernel
        c = ph17()
        return (c.H,) + make_special(c.H, *failures_of(c, 8, 6))
    if tag == "rows2049":                                    # 2049 x 384: beyond the row masks, not the bytes
        import test_gpu_lsd_sizes as ts
        H = lu.rows2048(True)
        _, syn, llr, hard = ts.rows_inputs()
        syn = np.concatenate([syn[:4], np.zeros((4, 1), np.uint8)], axis=1)
        syn[2, 2048] = 1                                     # (the extra row seeds a cluster of its own)
        return H, syn, llr[:4], hard[:4]
    if tag == "ph144x12":                                    # 864 x 2592
        from qldpc_amd import dem
        H, L, probs = dem.phenomenological("[[144, 12, 12]]", 12, 0.01, 0.01)
        rng = np.random.default_rng(12)
        H = ru._dense(H)
        c = ru.Case(tag, H, L, probs, ru.noisy_prior(0.01, H.shape[1], rng), ru.draw([probs], 16, rng))
        return (H,) + failures_of(c, 8, 4)
    assert tag == "dem1008"                                  # 1008 x 8991, the synthetic model of tools/bench_dem.py
    sys.path.insert(0, os.path.join(tl.ROOT, "tools"))
    try:
        import bench_dem
    finally:
        sys.path.pop(0)
    H, L, probs = bench_dem.synthetic_dem()
    H = ru._dense(H)
    rng = np.random.default_rng(1008)
    c = ru.Case(tag, H, L, probs, mc.dem_prior(probs), ru.draw([np.minimum(0.5, probs * 8.0)], 32, rng))
    return (H,) + failures_of(c, 8, 4)


SHAPES = {"ph72x17": (612, 1836), "rows2049": (2049, 384), "ph144x12": (864, 2592), "dem1008": (1008, 8991)}


@functools.lru_cache(maxsize=None)
def beyond_ref(tag, g):
    if tag not in GOLDEN_TAGS:
        return lo.lsd_decode_batch(*beyond_inputs(tag), g)
    with np.load(GOLDEN_PATH) as z:
        return {k: z[f"{tag}_g{g}_{k}"] for k in GOLDEN_KEYS}


@pytest.mark.parametrize("tag,gs", [("ph72x17", (1, 0)), ("rows2049", (1, 0)), ("ph144x12", (1,)), ("dem1008", (1,))])
def test_beyond_the_lds_kernel(tag, gs):
    H, syn, llr, hard = beyond_inputs(tag)
    assert H.shape == SHAPES[tag] and tc.lds_kernel_refuses(*H.shape)
    lib = _lib.load()
    dec = fresh(H)
    # option 0: today's refusal, and a launch on that handle touches no output
    assert lib.qbp_lsd_configure(dec._h, 1) == _lib.E_UNSUPPORTED
    assert tl.re_bytes(lib.qbp_last_error()) == lu.lsd_lds_bytes(*H.shape) and b"2048 rows" in lib.qbp_last_error()
    for g in gs:
        want = beyond_ref(tag, g)
        print(tag, g, lo.presence(want), want["stats"][:, :2].tolist())
        for mem in (MEM_LARGE, MEM_AUTO):
            dec.set_option(_lib.OPT_LSD_MEM, mem)
            dec.lsd_configure(g, large={MEM_LARGE: "force", MEM_AUTO: True}[mem])
            got = device_lsd(dec, (syn, llr, hard))
            assert ru.info(dec) == large_info(H, len(syn), dec.info("num_cu")), ru.info(dec)
            assert_equal(got, want, (tag, g, mem))
    # back to option 0 after a configuration: every call checks again
    dec.set_option(_lib.OPT_LSD_MEM, MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        device_lsd(dec, (syn, llr, hard))
    assert e.value.code == _lib.E_UNSUPPORTED


def test_auto_keeps_the_lds_kernel_where_it_fits():
    H, syn, llr, hard = small_inputs("72")
    dec = fresh(H)
    dec.lsd_configure(1, large=True)
    got = device_lsd(dec, (syn, llr, hard))
    assert dec.info("threads") == 64 and dec.info("lds_bytes") == lu.lsd_lds16(*H.shape)
    assert_equal(got, small_ref("72", 1), "auto on 36 x 72")


# =========================================================================================================================
# 3. a slice of the workspace serves one record after another
# =========================================================================================================================
@pytest.mark.parametrize("reverse", [False, True])
def test_workspace_reuse_heavy_then_light(reverse):
    """One workgroup per CU and more records than workgroups: slice b serves records b, b + grid, b + 2 grid.  The
    first grid records are heavy (g = 0 would be heavier still, but g is the call's: the records with the most active
    checks under the statement), the others light ones, among them zero residuals; then the same records in reverse
    order, light before heavy.  Whatever a slice held from its last record, every record equals the statement."""
    H, syn, llr, hard = small_inputs("144")
    for g in (0, 1):
        want = small_ref("144", g)
        dec = fresh(H, MEM_LARGE)
        dec.lsd_configure(g, large="force")
        num_cu = dec.info("num_cu")
        by_weight = np.argsort(-want["stats"][:, 1], kind="stable")
        B = 2 * num_cu + 19
        idx = np.concatenate([np.resize(by_weight[:8], num_cu), np.resize(by_weight[8:], B - num_cu)])
        heavy, light = want["stats"][idx[:num_cu], 1], want["stats"][idx[num_cu:], 1]
        assert heavy.min() >= light.max() and heavy.mean() > 2 * light.mean() and light.min() == 0
        if reverse:
            idx = idx[::-1]
        with gu.options(dec, blocks=1):
            got = device_lsd(dec, (syn[idx], llr[idx], hard[idx]))
        assert ru.info(dec) == large_info(H, B, num_cu, 1) and dec.info("grid") == num_cu < B
        assert_equal(got, want, ("reuse", g, reverse), idx)


# =========================================================================================================================
# 4. independence of B, the grid, the stream and an earlier configuration; null outputs
# =========================================================================================================================
@pytest.mark.parametrize("B", [1, 65, 700])
def test_poisoned_outputs_geometry_stream_and_reuse(B):
    t = gu.torch()
    H, syn, llr, hard = small_inputs("72")
    idx = (np.arange(B) * 7 + 3) % len(syn)
    dec = fresh(H, MEM_LARGE)
    stream = t.cuda.Stream()
    for g, per_cu in ((3, 0), (1, 0), (1, 1), (0, 2), (1, 7)):               # (g = 1 follows g = 3 on the same handle)
        want = small_ref("72", g)
        dec.lsd_configure(g, large="force")
        with gu.options(dec, blocks=per_cu):
            with t.cuda.stream(stream):
                got = device_lsd(dec, (syn[idx], llr[idx], hard[idx]), stream=stream.cuda_stream)
        assert ru.info(dec) == large_info(H, B, dec.info("num_cu"), per_cu)
        assert_equal(got, want, (B, g, per_cu), idx)
    # stats and solution may each be NULL
    want = small_ref("72", 1)
    sol, st = device_lsd(dec, (syn[idx], llr[idx], hard[idx]), stats=False)
    assert np.array_equal(sol, want["solution"][idx]) and bool((st == STAT_POISON).all())
    lib = _lib.load()
    syn_t, llr_t, hard_t = (gu.to_device(np.ascontiguousarray(a[idx])) for a in (syn, llr, hard))
    st_t = t.full((B, 4), STAT_POISON, dtype=t.int32, device="cuda")
    t.cuda.synchronize()
    # (the batch entries ask for a solution; the records build runs without one: section 5)
    assert lib.qbp_lsd_batch_device(dec._h, syn_t.data_ptr(), llr_t.data_ptr(), hard_t.data_ptr(), B, None,
                                    st_t.data_ptr(), None) == _lib.E_INVALID
    t.cuda.synchronize()
    assert bool((st_t == STAT_POISON).all())


# =========================================================================================================================
# 5. QBP_FLAG_LSD: the records build
# =========================================================================================================================
@pytest.mark.parametrize("first", ["sum_product", "min_sum", "layered"])
@pytest.mark.parametrize("g", [1, 0])
def test_mc_counters_equal_the_composition_and_the_lds_build(first, g):
    c = codes.load_code(lu.NAMES["72"])
    H, L, d = np.asarray(c.Hx, np.uint8), np.asarray(c.Lx, np.uint8), c.distance
    errors = (np.random.default_rng(17).random((400, 72)) < 0.08).astype(np.uint8)
    prior = mc.prior_of(0.08, 72)
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    layered = first == "layered"
    dec = fresh(H)
    dec.lsd_configure(g, large="force")
    if layered:
        dec.layered_configure(None)
    want, failures = tl.compose(dec, H, L, d, errors, prior, g, variant, layered)
    kw = dict(max_iter=tl.MC_ITERS, variant=variant, alpha=tl.ALPHA,
              flags=_lib.FLAG_LSD | (_lib.FLAG_LAYERED if layered else 0))
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    assert ru.info(dec) == large_info(H, 400, dec.info("num_cu"))
    assert failures >= 8 and got[6] == failures and np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, d, errors[:150], prior, **kw)
                          + dec.mc_run_errors(L, d, errors[150:], prior, **kw), want)
    dec.lsd_configure(g, large=False)
    assert np.array_equal(dec.mc_run_errors(L, d, errors, prior, **kw), want) and dec.info("threads") == 64
    if first == "sum_product" and g == 1:
        # the sampled entries: the split of the range, the chunk size, and mc.run_sweep
        dec.lsd_configure(1, large="force")
        kw = dict(seed=21, max_iter=tl.MC_ITERS, flags=_lib.FLAG_LSD)
        whole = dec.mc_run(L, d, 0.08, prior, 0, 1000, **kw)
        assert dec.info("threads") == tc.THREADS and whole[6] >= 8
        assert np.array_equal(dec.mc_run(L, d, 0.08, prior, 0, 377, **kw) + dec.mc_run(L, d, 0.08, prior, 377, 1000, **kw),
                              whole)
        sampled = dec.mc_sample_errors(0.08, 0, 1000, seed=21)
        assert np.array_equal(whole, tl.compose(dec, H, L, d, sampled, prior, 1, _lib.SUM_PRODUCT, False)[0])
        wkw = dict(max_iter=tl.MC_ITERS, flags=_lib.FLAG_LSD)
        by_weight = dec.mc_run_weight(L, d, 9, prior, 0, 500, seed=4, **wkw)
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 64)
        try:
            assert np.array_equal(by_weight, dec.mc_run_weight(L, d, 9, prior, 0, 500, seed=4, **wkw))
        finally:
            dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)
        werr = dec.mc_sample_errors_weight(9, 0, 500, seed=4)
        assert np.array_equal(by_weight, tl.compose(dec, H, L, d, werr, prior, 1, _lib.SUM_PRODUCT, False)[0])
        table = mc.run_sweep(lu.NAMES["72"], [0.08], 1000, seed=21, max_iter=tl.MC_ITERS, lsd=1, lsd_large="force")
        assert np.array_equal(table[0], whole)


@pytest.mark.parametrize("first", ["flooding", "layered_large"])
def test_mc_beyond_the_lds_kernel(first):
    """612 x 1836 through mc_run_errors and mc_run_probs, after flooding BP and after the layered large build (which
    converges on every error of the case at rate 0.01: its errors are 40 at rate 0.02)."""
    c = ph17()
    H, L, errors, prior = c.H, np.ascontiguousarray(c.L, np.uint8), c.errors, c.prior
    layered = first == "layered_large"
    if layered:
        errors = ru.draw([np.full(c.n, 0.02)], 40, np.random.default_rng(171))
    dec = fresh(H)
    dec.lsd_configure(1, large=True)
    if layered:
        dec.set_option(_lib.OPT_LAYERED_MEM, MEM_LARGE)
        dec.layered_configure(None)
    want, failures = tl.compose(dec, H, L, 0, errors, prior, 1, _lib.SUM_PRODUCT, layered)
    kw = dict(max_iter=tl.MC_ITERS, alpha=tl.ALPHA, flags=_lib.FLAG_LSD | (_lib.FLAG_LAYERED if layered else 0))
    got = dec.mc_run_errors(L, 0, errors, prior, **kw)
    print(first, dict(zip(_lib.COUNTER_NAMES, got.tolist())), failures, ru.info(dec))
    assert ru.info(dec) == large_info(H, len(errors), dec.info("num_cu"))
    assert failures >= 4 and got[6] == failures and np.array_equal(got, want)
    assert np.array_equal(dec.mc_run_errors(L, 0, errors[:17], prior, **kw)
                          + dec.mc_run_errors(L, 0, errors[17:], prior, **kw), want)
    # mc_run_probs: the sampler's own errors, whole and split, against the composition on them
    pkw = dict(seed=5, max_iter=tl.MC_ITERS, alpha=tl.ALPHA, flags=kw["flags"])
    probs = np.full(c.n, 0.02 if layered else 0.01)
    whole = dec.mc_run_probs(L, 0, probs, prior, 0, 128, **pkw)
    assert np.array_equal(dec.mc_run_probs(L, 0, probs, prior, 0, 47, **pkw)
                          + dec.mc_run_probs(L, 0, probs, prior, 47, 128, **pkw), whole)
    sampled = dec.mc_sample_errors_probs(probs, 0, 128, seed=5)
    assert np.array_equal(whole, tl.compose(dec, H, L, 0, sampled, prior, 1, _lib.SUM_PRODUCT, layered)[0]) and whole[6] >= 2
    # option 0 on the same handle: the call is refused before any GPU work
    dec.set_option(_lib.OPT_LSD_MEM, MEM_LDS)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_errors(L, 0, errors, prior, **kw)
    assert e.value.code == _lib.E_UNSUPPORTED


# =========================================================================================================================
# 6. refusals, host only
# =========================================================================================================================
def test_option_values_out_of_range():
    lib = _lib.load()
    dec = fresh(small_inputs("72")[0])
    for bad in (3, -1):
        assert lib.qbp_set_option(dec._h, _lib.OPT_LSD_MEM, bad) == _lib.E_INVALID
        assert b"localized statistics decoding memory mode" in lib.qbp_last_error()
    for ok in (MEM_LDS, MEM_LARGE, MEM_AUTO):
        dec.set_option(_lib.OPT_LSD_MEM, ok)


@pytest.mark.parametrize("shape", [(1, 65536), (8000, 64)], ids=["n65536", "tables"])
def test_matrices_beyond_the_large_build(shape):
    """n = 65536, and a matrix whose cluster tables pass 160 KiB: refused under every value of the option, with the
    byte count of the build the value allows."""
    lib = _lib.load()
    Hb = np.zeros(shape, np.uint8)
    Hb[np.arange(shape[0]), np.arange(shape[0]) % shape[1]] = 1
    Hb[0, shape[1] - 1] = 1
    big = fresh(Hb)
    for mem in (MEM_LARGE, MEM_AUTO, MEM_LDS):
        big.set_option(_lib.OPT_LSD_MEM, mem)
        assert lib.qbp_lsd_configure(big._h, 1) == _lib.E_UNSUPPORTED
        msg = lib.qbp_last_error()
        need = tc.lsd_large_lds_bytes(*Hb.shape) if mem != MEM_LDS else lu.lsd_lds_bytes(*Hb.shape)
        assert b"160 KiB" in msg and tl.re_bytes(msg) == need > tc.LDS_LIMIT, msg
        sol = np.full((1, Hb.shape[1]), 9, np.uint8)
        args = (np.zeros((1, Hb.shape[0]), np.uint8), np.ones((1, Hb.shape[1])), np.zeros((1, Hb.shape[1]), np.uint8))
        assert lib.qbp_lsd_batch(big._h, *(a.ctypes.data for a in args), 1, sol.ctypes.data, None) == _lib.E_INVALID
        assert np.all(sol == 9)


def test_a_valid_call_after_a_refused_one():
    """A handle configured under option 1 whose option then asks for what the matrix does not allow: refused with the
    outputs untouched, and a following valid call on the same handle works."""
    lib = _lib.load()
    H, syn, llr, hard = beyond_inputs("ph72x17")
    want = beyond_ref("ph72x17", 1)
    args = tuple(np.ascontiguousarray(a[:3]) for a in (syn, llr, hard))
    dec2 = fresh(H, MEM_LARGE)
    dec2.lsd_configure(1, large="force")
    dec2.set_option(_lib.OPT_LSD_MEM, MEM_LDS)
    sol = np.full((3, H.shape[1]), 9, np.uint8)
    st = np.full((3, 4), -5, np.int32)
    assert lib.qbp_lsd_batch(dec2._h, *(a.ctypes.data for a in args), 3, sol.ctypes.data, st.ctypes.data) == _lib.E_UNSUPPORTED
    assert b"needs 166292 B" in lib.qbp_last_error() and np.all(sol == 9) and np.all(st == -5)
    with pytest.raises(_lib.QbpError):
        device_lsd(dec2, args)
    dec2.set_option(_lib.OPT_LSD_MEM, MEM_AUTO)
    assert_equal(dec2.lsd(*args), want, "after a refusal", slice(0, 3))
