"""bp_relay_kernel, bp_gd_kernel and bp_layered_kernel beyond one pass per workgroup: on matrices where a thread owns
more than one work item of the strided loops (class-blocked check and variable steps, long rows and columns, the
syndrome ballot, the BPGD arg-max, a layered level wider than the workgroup), with more records than workgroups (the
shared work counter), with dynamic LDS between 64 and 160 KiB, and on a detector error model with per-column priors --
against the numpy statements (tests/relay_oracle.py, tests/gd_oracle.py, tests/layered_oracle.py), bit for bit, NaN
equal to NaN, into poisoned buffers.

The CPU tests (unmarked) assert that every matrix reaches the path it is named for; the GPU tests assert the launch
geometry the library reports (threads, grid, lds_bytes) against the restatement in record_kernel_util and print it."""
import contextlib
import functools

import numpy as np
import pytest

import gd_oracle as go
import geometry_util as gu
import layered_oracle as lo
import record_kernel_util as ru
import relay_oracle as ro
import test_gpu_gd as tg
import test_gpu_relay as tr
from oracle import oracle
from qldpc_amd import _lib, bp, dem, mc

gpu = pytest.mark.gpu
LAYERED = _lib.FLAG_LAYERED
LAYERED_ITERS = 30
LAYERED_VARIANTS = [(_lib.SUM_PRODUCT, 1.0), (_lib.MIN_SUM, 0.8)]
VIDS = ["sum_product", "min_sum"]
GD_ITER_LIMIT = 1 << 30                     # (Outputs.fetch: any iteration count >= 0 is a written one)


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


# =========================================================================================================================
# 0. CPU: each case reaches what it claims
# =========================================================================================================================
def test_np_lds_bytes_is_the_size_of_the_table_image():
    assert ru.np_lds_bytes() == 8 * (16 * 18 + 16 * 2 + 32 + 32) == 3072


def test_thread_counts_of_the_matrices_named_in_the_kernels():
    """gd_threads / relay_threads on the two figures their comments give: [[144,12,12]] 192, [[288,12,18]] 320."""
    from qldpc_amd import codes
    for name, want in (("[[144, 12, 12]]", 192), ("[[288, 12, 18]]", 320)):
        sh = ru.Shape(np.asarray(codes.load_code(name).Hx))
        assert ru.gd_threads(sh) == want and ru.relay_threads(sh) == want


def test_ph72x6_two_gd_passes_and_the_widest_relay_workgroup():
    c = ru.case("ph72x6")
    sh = c.shape
    assert (sh.m, sh.n, sh.E) == (216, 648, 1692) and (sh.check_items, sh.var_items) == (256, 704)
    assert sh.long_rows == sh.long_cols == sh.empty_cols == 0
    assert ru.gd_threads(sh) == 384 and ru.passes(sh.var_items, 384) == 2 and ru.passes(sh.check_items, 384) == 1
    assert ru.relay_threads(sh) == 704 and ru.passes(sh.var_items, 704) == 1
    assert ru.passes(sh.n, 384) == 2                    # the arg-max and the output loops: two variables per thread
    widths = ru.level_widths(c.H, lo.order_of(c.H, "default"))
    assert len(widths) == 4 and max(widths) == 54
    # (four slots of this matrix pass the 80 KiB that keep two workgroups on a CU: three)
    assert ru.layered_slots(sh, 54, ru.BATCH, True) == 3 and ru.passes(3 * sh.m, ru.LAYERED_THREADS) == 3
    assert ru.gd_lds_bytes(sh.m, sh.n, sh.E, True) < ru.LDS_DEFAULT


def test_ph72x12_three_gd_passes_two_relay_passes_and_m_beyond_the_layered_workgroup():
    c = ru.case("ph72x12")
    sh = c.shape
    assert (sh.m, sh.n, sh.E) == (432, 1296, 3420) and (sh.check_items, sh.var_items) == (512, 1408)
    assert ru.gd_threads(sh) == 512 and ru.passes(sh.var_items, 512) == 3
    assert sh.var_items % 512 != 0                      # a ragged last pass
    assert ru.relay_threads(sh) == 704 and ru.passes(sh.var_items, 704) == 2
    assert ru.passes(sh.m, 512) == 1 and sh.m > 256     # the syndrome ballot: lane 0 of a wavefront writes two words
    widths = ru.level_widths(c.H, lo.order_of(c.H, "default"))
    assert len(widths) == 4 and max(widths) == 108
    # 256 / 108 = 2 slots, but two pass the 80 KiB that keep two workgroups on a CU: the automatic choice is one, and
    # QBP_OPT_LAYERED_SLOTS = 2 (88 KiB, above the 64 KiB a kernel gets without the attribute) is run as well
    assert ru.layered_slots(sh, 108, ru.BATCH, True) == 1 and ru.layered_slots(sh, 108, ru.BATCH, True, 2) == 2
    assert sh.m > ru.LAYERED_THREADS and ru.passes(2 * sh.m, ru.LAYERED_THREADS) == 4
    assert ru.LDS_DEFAULT < ru.layered_lds_bytes(sh.m, sh.n, sh.E, 2, True) < ru.LDS_LIMIT
    assert ru.relay_lds_bytes(sh.m, sh.n, sh.E) < ru.LDS_DEFAULT


def test_dem_synth_long_rows_long_columns_empty_columns_and_column_priors_in_two_gd_passes():
    c = ru.case("dem_synth")
    sh = c.shape
    assert (sh.m, sh.n) == (144, 595)
    assert sh.row_w.max() > 8 and sh.long_rows >= 64 and sh.long_edges > 512      # long-row loops: two passes as well
    assert set(np.unique(sh.col_w[sh.col_w > 4])) == {5, 6} and sh.long_cols >= 64
    assert sh.empty_cols == 3
    assert ru.gd_threads(sh) == 320 and ru.passes(sh.var_items, 320) == 2
    assert ru.relay_threads(sh) == 640 and ru.passes(sh.long_edges, 640) >= 2
    assert len(np.unique(c.prior)) > 150                # the model's own probabilities: 160 hyperedges, each its own


def test_disjoint300_one_level_beyond_the_layered_workgroup_with_a_long_row_in_the_ragged_pass():
    c = ru.case("disjoint300")
    sh = c.shape
    assert (sh.m, sh.n, sh.E) == (300, 912, 912) and sh.long_rows == 2 and set(sh.col_w) == {1}
    for kind in ("default", "random"):
        order = lo.order_of(c.H, kind)
        levels = lo.levels_of(c.H, order)
        assert [len(g) for g in levels] == [300]
        if kind == "default":
            assert (sh.row_w[levels[0][ru.LAYERED_THREADS:]] > 8).sum() == 2      # both long rows among items 256 .. 299
    assert ru.layered_slots(sh, 300, ru.BATCH, True) == 1
    assert ru.gd_threads(sh) == 512 and ru.passes(sh.var_items, 512) == 2 and ru.relay_threads(sh) == 960


@pytest.mark.parametrize("kind", list(ru.NEAR_LIMIT))
def test_near_limit_rounds_fit_and_one_more_does_not(kind):
    lds_of = ru.NEAR_LIMIT[kind]
    T = ru.largest_rounds(lds_of)
    assert T == {"relay": 33, "gd_min_sum": 40, "gd_sum_product": 39, "layered": 39}[kind]
    assert ru.LDS_DEFAULT < lds_of(ru.ph_shape(T)) <= ru.LDS_LIMIT < lds_of(ru.ph_shape(T + 1))
    H = dem.phenomenological("[[72, 12, 6]]", 2, 0.01)[0]
    sh = ru.Shape(H.toarray())
    assert (sh.m, sh.n, sh.E) == (ru.ph_shape(2).m, ru.ph_shape(2).n, ru.ph_shape(2).E)


# =========================================================================================================================
# the statements, computed once
# =========================================================================================================================
def relay_config(n):
    return tr.config(n, 1)


@functools.lru_cache(maxsize=None)
def relay_ref(tag):
    c = ru.case(tag)
    cfg = relay_config(c.n)
    return ro.relay_decode_batch(c.H, c.syn, c.prior, cfg.gammas, cfg.leg_iters, tr.STOP, tr.ALPHA)


@functools.lru_cache(maxsize=None)
def gd_ref(tag, variant, rounds):
    """rounds 6: the batch of case(tag); "n": its records that both variants solve within 40 decimations (a record the
    statement never solves walks n rounds of 8 iterations in numpy)."""
    c = ru.case(tag) if rounds == 6 else ru.easy(tag)
    cfg = tg.config(variant, c.n if rounds == "n" else rounds)
    return c, cfg, go.gd_decode_batch(c.H, c.syn, c.prior, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, variant,
                                      tg.ALPHA, 20.0)


@functools.lru_cache(maxsize=None)
def layered_ref(tag, kind, variant, alpha):
    c = ru.case(tag)
    return lo.layered_decode_batch(c.H, c.syn, c.prior, LAYERED_ITERS, variant, alpha, 20.0, lo.order_of(c.H, kind),
                                   "level")


# =========================================================================================================================
# 2. batch builds against the statements
# =========================================================================================================================
@gpu
@pytest.mark.parametrize("tag", ru.TAGS)
def test_relay_batch_equals_statement(tag):
    c, want = ru.case(tag), relay_ref(tag)
    B, sh = ru.BATCH, c.shape
    dec = fresh(c.H)
    dec.relay_configure(relay_config(c.n))
    out = ru.RecordOutputs(B, c.n, ("legs", "solutions"))
    ru.relay_launch(dec, gu.to_device(c.syn), gu.to_device(c.prior), B, out, gu.stream_ptr())
    got = out.fetch_all(B, tr.LEGS * tr.ITERS + 1, f"relay {tag}")
    ru.assert_same(got, ru.relay_want(want), f"relay {tag}")
    info = ru.info(dec)
    print(tag, "relay", info, ro.classes(want))
    assert info == dict(threads=ru.relay_threads(sh), grid=ru.relay_grid(sh, B, dec.info("num_cu")),
                        lds_bytes=ru.relay_lds_bytes(sh.m, sh.n, sh.E))


@gpu
@pytest.mark.parametrize("rounds", [6, "n"], ids=["six_rounds", "to_exhaustion"])
@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
@pytest.mark.parametrize("tag", ru.TAGS)
def test_gd_batch_equals_statement(tag, variant, rounds):
    c, cfg, want = gd_ref(tag, variant, rounds)
    B, sh = ru.BATCH, c.shape
    dec = fresh(c.H)
    dec.gd_configure(cfg)
    out = ru.RecordOutputs(B, c.n, ("rounds",))
    ru.gd_launch(dec, gu.to_device(c.syn), gu.to_device(c.prior), B, out, gu.stream_ptr())
    what = f"gd {tag} variant {variant} max_rounds {rounds}"
    got = out.fetch_all(B, GD_ITER_LIMIT, what)
    ru.assert_same(got, ru.gd_want(want), what)
    info = ru.info(dec)
    print(what, info, go.classes(want), "most rounds", int(want["rounds"].max()))
    sp = variant == _lib.SUM_PRODUCT
    assert info == dict(threads=ru.gd_threads(sh), grid=ru.gd_grid(sh, B, dec.info("num_cu"), sp),
                        lds_bytes=ru.gd_lds_bytes(sh.m, sh.n, sh.E, sp))


@contextlib.contextmanager
def layered_slots_option(dec, slots):
    dec.set_option(_lib.OPT_LAYERED_SLOTS, slots)
    try:
        yield
    finally:
        dec.set_option(_lib.OPT_LAYERED_SLOTS, 0)


@gpu
@pytest.mark.parametrize("kind", ["default", "random"])
@pytest.mark.parametrize("tag", ru.TAGS)
def test_layered_batch_equals_statement(tag, kind):
    c = ru.case(tag)
    B, sh = ru.BATCH, c.shape
    order = lo.order_of(c.H, kind)
    width = max(ru.level_widths(c.H, order))
    dec = fresh(c.H)
    dec.layered_configure(order)
    syn_t, prior_t = gu.to_device(c.syn), gu.to_device(c.prior)
    out = gu.Outputs(B, c.n)
    for variant, alpha in LAYERED_VARIANTS:
        want = layered_ref(tag, kind, variant, alpha)
        tables = variant == _lib.SUM_PRODUCT
        for slots in (0, 2):
            what = f"layered {tag} {kind} variant {variant} slots {slots}"
            with layered_slots_option(dec, slots):
                got = gu.decode(dec, syn_t, prior_t, B, out, what, max_iter=LAYERED_ITERS, variant=variant, alpha=alpha,
                                flags=LAYERED)
            gu.assert_same(got, want, what)
            S = ru.layered_slots(sh, width, B, tables, slots)
            info = ru.info(dec)
            print(what, info, "S", S, "widest level", width, "converged", int(want[1].sum()))
            assert info == dict(threads=ru.LAYERED_THREADS, grid=ru.layered_grid(sh, S, B, dec.info("num_cu"), tables),
                                lds_bytes=ru.layered_lds_bytes(sh.m, sh.n, sh.E, S, tables))


@gpu
def test_statement_classes_are_present():
    """Per decoder, pooled over the four matrices: >= 8 records in each class of the statement's own output."""
    pooled = {k: sum(ro.classes(relay_ref(t))[k] for t in ru.TAGS) for k in ("leg0", "later", "replaced", "never")}
    print("relay", pooled, {t: ro.classes(relay_ref(t)) for t in ru.TAGS})
    assert all(v >= 8 for v in pooled.values()), pooled
    for variant, vid in zip(tg.VARIANTS, VIDS):
        refs = {(t, r): gd_ref(t, variant, r)[2] for t in ru.TAGS for r in (6, "n")}
        pooled = {k: sum(go.classes(r)[k] for r in refs.values()) for k in ("round0", "later", "never")}
        print("gd", vid, pooled, {k: go.classes(r) for k, r in refs.items()})
        assert all(v >= 8 for v in pooled.values()), pooled
        deep = sum(int((r["rounds"] > 6).sum()) for (t, rounds), r in refs.items() if rounds == "n")
        assert deep >= 8, deep                          # max_rounds = n goes beyond what max_rounds = 6 reaches
    for (variant, alpha), vid in zip(LAYERED_VARIANTS, VIDS):
        refs = [layered_ref(t, k, variant, alpha) for t in ru.TAGS for k in ("default", "random")]
        conv = np.concatenate([r[1] for r in refs])
        iters = np.concatenate([r[2] for r in refs])
        counts = dict(converged=int(conv.sum()), not_converged=int((~conv).sum()), late=int((conv & (iters > 2)).sum()))
        print("layered", vid, counts)
        assert all(v >= 8 for v in counts.values()), counts


# ---- dynamic LDS between 64 and 160 KiB, and the refusal one round further -------------------------------------------------
NEAR_B, NEAR_P = 8, 0.01


def near_limit_decoder(kind, c):
    """(configure, launch, statement) of one kind on the case c."""
    if kind == "relay":
        cfg = relay_config(c.n)
        extra = ("legs", "solutions")
        configure = lambda dec: dec.relay_configure(cfg)
        launch = lambda dec, s, p, B, out: ru.relay_launch(dec, s, p, B, out, gu.stream_ptr())
        statement = lambda: ru.relay_want(ro.relay_decode_batch(c.H, c.syn, c.prior, cfg.gammas, cfg.leg_iters, tr.STOP,
                                                                 tr.ALPHA))
    elif kind.startswith("gd"):
        variant = _lib.MIN_SUM if kind == "gd_min_sum" else _lib.SUM_PRODUCT
        cfg = tg.config(variant, 6)
        extra = ("rounds",)
        configure = lambda dec: dec.gd_configure(cfg)
        launch = lambda dec, s, p, B, out: ru.gd_launch(dec, s, p, B, out, gu.stream_ptr())
        statement = lambda: ru.gd_want(go.gd_decode_batch(c.H, c.syn, c.prior, cfg.iters_per_round, cfg.max_rounds,
                                                           cfg.decim_llr, variant, tg.ALPHA, 20.0))
    else:
        extra = ()
        order = lo.order_of(c.H, "ascending")       # (the statement's default order takes H H^T: slow at 1400 checks)
        configure = lambda dec: dec.layered_configure(order)
        launch = lambda dec, s, p, B, out: gu.launch(dec, s, p, B, out, max_iter=LAYERED_ITERS,
                                                     variant=_lib.SUM_PRODUCT, flags=LAYERED)
        statement = lambda: lo.layered_decode_batch(c.H, c.syn, c.prior, LAYERED_ITERS, lo.SUM_PRODUCT, 1.0, 20.0,
                                                    order, "level")
    return extra, configure, launch, statement


@gpu
@pytest.mark.parametrize("kind", list(ru.NEAR_LIMIT))
def test_near_limit_decodes_and_one_round_more_is_unsupported(kind):
    lds_of = ru.NEAR_LIMIT[kind]
    T = ru.largest_rounds(lds_of)
    c = ru.phenomenological(T, NEAR_P, 100 + T, NEAR_B)
    extra, configure, launch, statement = near_limit_decoder(kind, c)
    want = statement()
    dec = fresh(c.H)
    configure(dec)
    syn_t, prior_t = gu.to_device(c.syn), gu.to_device(c.prior)
    out = ru.RecordOutputs(NEAR_B, c.n, extra)
    launch(dec, syn_t, prior_t, NEAR_B, out)
    ru.assert_same(out.fetch_all(NEAR_B, GD_ITER_LIMIT, f"{kind} T = {T}"), want, f"{kind} T = {T}")
    info = ru.info(dec)
    print(kind, "T", T, c.H.shape, info, "converged", int(np.sum(want[1])))
    assert info["lds_bytes"] == lds_of(c.shape) and ru.LDS_DEFAULT < info["lds_bytes"] <= ru.LDS_LIMIT
    assert info["grid"] == NEAR_B
    # a second, smaller launch on the same handle, after the attribute was raised
    small = ru.RecordOutputs(3, c.n, extra)
    launch(dec, syn_t, prior_t, 3, small)
    ru.assert_same(small.fetch_all(3, GD_ITER_LIMIT, f"{kind} T = {T}, B = 3"), tuple(x[:3] for x in want),
                   f"{kind} T = {T}, B = 3")
    # one round more: refused, and no output is touched
    big = ru.phenomenological(T + 1, NEAR_P, 100 + T, NEAR_B)
    assert lds_of(big.shape) > ru.LDS_LIMIT
    dec2 = fresh(big.H)
    with pytest.raises(_lib.QbpError) as e:
        near_limit_decoder(kind, big)[1](dec2)
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in _lib.load().qbp_last_error()
    out2 = ru.RecordOutputs(NEAR_B, big.n, extra)
    with pytest.raises(_lib.QbpError) as e:
        near_limit_decoder(kind, big)[2](dec2, gu.to_device(big.syn), gu.to_device(big.prior), NEAR_B, out2)
    assert e.value.code in (_lib.E_UNSUPPORTED, _lib.E_INVALID)         # (nothing is configured on this handle)
    assert out2.untouched()


# =========================================================================================================================
# 3. the work counter of the per-record kernels: more records than workgroups
# =========================================================================================================================
def spread(B, base, seed):
    """B rows of a base set of statement records, through a fixed permutation."""
    return np.random.default_rng(seed).permutation(B) % base


def on_own_stream(fn):
    """Run fn() with a non-default torch stream current; returns after the stream has drained."""
    t = gu.torch()
    stream = t.cuda.Stream()
    t.cuda.synchronize()
    with t.cuda.stream(stream):
        assert gu.stream_ptr() == stream.cuda_stream and stream.cuda_stream != 0
        fn(stream.cuda_stream)
    stream.synchronize()


@functools.lru_cache(maxsize=None)
def relay_small_ref(name, p, seed):
    """The records of tests/test_gpu_relay.py's `references` fixture."""
    H, _, _ = tr.matrix(name)
    n = H.shape[1]
    errors = (np.random.default_rng(seed).random((256, n)) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log((1 - p) / p))
    cfg = tr.config(n, seed)
    return H, syn, prior, cfg, ro.relay_decode_batch(H, syn, prior, cfg.gammas, cfg.leg_iters, tr.STOP, tr.ALPHA)


@gpu
@pytest.mark.parametrize("name,p,seed", [("72", 0.1, 1), ("rand37", 0.05, 1)])
def test_relay_work_counter(name, p, seed):
    H, syn, prior, cfg, ref = relay_small_ref(name, p, seed)
    sh, n = ru.Shape(H), H.shape[1]
    dec = fresh(H)
    dec.relay_configure(cfg)
    B = 2 * ru.relay_grid(sh, 1 << 30, dec.info("num_cu")) + 37
    idx = spread(B, 256, 5)
    syn_t, prior_t = gu.to_device(syn[idx]), gu.to_device(prior)
    out = ru.RecordOutputs(B, n, ("legs", "solutions"))
    on_own_stream(lambda s: ru.relay_launch(dec, syn_t, prior_t, B, out, s))
    grid = dec.info("grid")
    print(name, "relay", ru.info(dec), "B", B, ro.classes(ref))
    assert B == 2 * grid + 37 and B > grid
    got = out.fetch_all(B, tr.LEGS * tr.ITERS + 1, f"relay {name} B {B}")
    ru.assert_same(got, ru.relay_want(ref, idx), f"relay {name} B {B}")


@gpu
@pytest.mark.parametrize("blocks", [0, 1], ids=["auto", "one_per_cu"])
@pytest.mark.parametrize("variant", tg.VARIANTS, ids=VIDS)
@pytest.mark.parametrize("name,p,seed", [("72", 0.1, 1), ("rand37", 0.05, 1)])
def test_gd_work_counter(name, p, seed, variant, blocks):
    H, syn, prior = tg.inputs(name, p, seed)
    cfg = tg.config(variant, 6)
    ref = gd_small_ref(name, p, seed, variant)
    sh, n = ru.Shape(H), H.shape[1]
    dec = fresh(H)
    dec.gd_configure(cfg)
    sp = variant == _lib.SUM_PRODUCT
    B = 2 * ru.gd_grid(sh, 1 << 30, dec.info("num_cu"), sp, blocks) + 37
    idx = spread(B, 256, 6)
    syn_t, prior_t = gu.to_device(syn[idx]), gu.to_device(prior)
    out = ru.RecordOutputs(B, n, ("rounds",))
    with gu.options(dec, blocks=blocks):
        on_own_stream(lambda s: ru.gd_launch(dec, syn_t, prior_t, B, out, s))
    grid = dec.info("grid")
    print(name, "gd", variant, "blocks", blocks, ru.info(dec), "B", B, go.classes(ref))
    assert B == 2 * grid + 37 and B > grid
    what = f"gd {name} variant {variant} blocks {blocks} B {B}"
    ru.assert_same(out.fetch_all(B, GD_ITER_LIMIT, what), ru.gd_want(ref, idx), what)


@functools.lru_cache(maxsize=None)
def gd_small_ref(name, p, seed, variant):
    """The six-round records of tests/test_gpu_gd.py's `references` fixture."""
    H, syn, prior = tg.inputs(name, p, seed)
    cfg = tg.config(variant, 6)
    return go.gd_decode_batch(H, syn, prior, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, variant, tg.ALPHA, 20.0)


@gpu
@pytest.mark.parametrize("slots", [1, 0])
def test_layered_work_counter_on_a_level_wider_than_the_workgroup(slots):
    c = ru.case("disjoint300")
    sh = c.shape
    dec = fresh(c.H)
    dec.layered_configure(None)
    prior_t = gu.to_device(c.prior)
    num_cu = dec.info("num_cu")
    for variant, alpha in LAYERED_VARIANTS:
        want = layered_ref("disjoint300", "default", variant, alpha)
        tables = variant == _lib.SUM_PRODUCT
        S = ru.layered_slots(sh, 300, 1 << 30, tables, slots)
        assert S == 1
        for B in (37, 2 * ru.layered_grid(sh, S, 1 << 30, num_cu, tables) * S + 5):
            idx = spread(B, ru.BATCH, 7)
            syn_t = gu.to_device(c.syn[idx])
            out = gu.Outputs(B, c.n)
            with_slots = lambda s: gu.launch(dec, syn_t, prior_t, B, out, max_iter=LAYERED_ITERS, variant=variant,
                                             alpha=alpha, flags=LAYERED)
            with layered_slots_option(dec, slots):
                on_own_stream(with_slots)
            what = f"layered disjoint300 variant {variant} slots {slots} B {B}"
            got = out.fetch(B, LAYERED_ITERS, what)
            grid = dec.info("grid")
            print(what, ru.info(dec))
            assert grid == ru.layered_grid(sh, S, B, num_cu, tables)
            assert B == 37 or (B == 2 * grid * S + 5 and B > grid * S)
            gu.assert_same(got, tuple(x[idx] for x in want), what)


# =========================================================================================================================
# 4. records builds on the larger matrices
# =========================================================================================================================
MC_ITERS = tg.MC_ITERS
assert tr.MC_ITERS == MC_ITERS
MC_TRIALS = {"ph72x6": 224, "dem_synth": 256}
MC_RATE = {"ph72x6": 0.03, "dem_synth": 5.0}


@functools.lru_cache(maxsize=None)
def mc_case(tag, trials=None, rate=None):
    """(H, L, distance, errors, prior) of a records build: stored errors, the per-column prior of case(tag)."""
    c = ru.case(tag)
    rate = MC_RATE[tag] if rate is None else rate
    probs = np.minimum(0.5, c.probs * rate) if tag == "dem_synth" else np.full(c.n, rate)
    errors = ru.draw([probs], trials or MC_TRIALS[tag], np.random.default_rng(17))
    return c.H, np.ascontiguousarray(c.L, np.uint8), 6 if tag == "ph72x6" else 0, errors, c.prior


def first_stage(first):
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    return variant, first == "layered"


def compose_layered(dec, H, L, d, errors, prior, variant, second):
    """The layered first stage on the device (batch entry), `second(syn, llr, hard) -> (hard, converged)` on its
    failures, oracle.classify_trials' rules: tests/test_gpu_relay.py's compose with FLAG_LAYERED in the first stage."""
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, llr = dec.decode(syn, prior, MC_ITERS, variant=variant, alpha=tr.ALPHA, layered=True)
    det = hard.copy()
    f = np.flatnonzero(~conv)
    det[f], solved = second(syn[f], llr[f], hard[f])
    cnt = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
    cnt[10] = int((~solved).sum())
    assert cnt[10] == int(((det[f].astype(np.int64) @ H.T % 2) != syn[f]).any(1).sum())
    return cnt, len(f)


# (OSD-0 behind the flooding first stages is tests/test_gpu_dem.py's)
STAGES = [(f, s) for f in ("sum_product", "min_sum", "layered") for s in ("relay", "gd")] + [("layered", "osd0")]


@gpu
@pytest.mark.parametrize("first,second", STAGES)
@pytest.mark.parametrize("tag", list(MC_TRIALS))
def test_mc_run_errors_equals_the_composition(tag, first, second):
    H, L, d, errors, prior = mc_case(tag)
    n = H.shape[1]
    variant, layered = first_stage(first)
    dec = fresh(H)
    if layered:
        dec.layered_configure(None)
    if second == "relay":
        cfg = tr.config(n, 4)
        dec.relay_configure(cfg)
        flag = _lib.FLAG_RELAY
        if layered:
            def stage(syn, llr, hard):
                r = ro.relay_decode_batch(H, syn, prior, cfg.gammas, cfg.leg_iters, cfg.stop_after, cfg.alpha, cfg.clip_llr)
                return r["hard"], r["converged"]
            want, failures = compose_layered(dec, H, L, d, errors, prior, variant, stage)
        else:
            want, failures = tr.compose(dec, H, L, d, errors, prior, cfg, variant)
    elif second == "gd":
        cfg = tg.config(_lib.SUM_PRODUCT if first == "min_sum" else _lib.MIN_SUM, 6)
        dec.gd_configure(cfg)
        flag = _lib.FLAG_GD
        want, failures = tg.compose(dec, H, L, d, errors, prior, cfg, variant, layered)
    else:
        flag = _lib.FLAG_OSD0

        def stage(syn, llr, hard):
            sol = np.stack([oracle.osd0(H, syn[i], llr[i], hard[i]) for i in range(len(syn))]) if len(syn) else hard
            return sol, ~((sol.astype(np.int64) @ H.T % 2) != syn).any(1)
        want, failures = compose_layered(dec, H, L, d, errors, prior, variant, stage)
    kw = dict(max_iter=MC_ITERS, variant=variant, alpha=tr.ALPHA, flags=flag | (LAYERED if layered else 0))
    got = dec.mc_run_errors(L, d, errors, prior, **kw)
    print(tag, first, second, dict(zip(_lib.COUNTER_NAMES, got.tolist())), "failures", failures, ru.info(dec))
    assert failures >= 64 and got[6] == failures and got[0] == len(errors)
    assert np.array_equal(got, want)


@gpu
def test_gd_records_beyond_the_grid():
    """More failure records than workgroups of the second stage: one workgroup per CU, and a rate at which most of the
    trials reach it."""
    H, L, d, errors, prior = mc_case("ph72x6", 420, 0.05)
    cfg = tg.config(_lib.MIN_SUM, 6)
    dec = fresh(H)
    dec.gd_configure(cfg)
    want, failures = tg.compose(dec, H, L, d, errors, prior, cfg, _lib.SUM_PRODUCT, False)
    with gu.options(dec, blocks=1):
        got = dec.mc_run_errors(L, d, errors, prior, max_iter=MC_ITERS, variant=_lib.SUM_PRODUCT, alpha=tg.ALPHA,
                                flags=_lib.FLAG_GD)
    info = ru.info(dec)
    print(dict(zip(_lib.COUNTER_NAMES, got.tolist())), "failures", failures, info)
    assert info["threads"] == ru.gd_threads(ru.Shape(H)) and info["grid"] == min(len(errors), dec.info("num_cu"))
    assert failures > info["grid"]
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("second", ["relay", "gd"])
def test_run_dem_takes_the_second_stage(second):
    c = ru.case("dem_synth")
    probs = np.minimum(0.5, c.probs * 5.0)
    trials = 2000
    if second == "relay":
        cfg = tr.config(c.n, 4)
        kw, flag = dict(relay=cfg), _lib.FLAG_RELAY
    else:
        cfg = tg.config(_lib.MIN_SUM, 6)
        kw, flag = dict(gd=cfg), _lib.FLAG_GD
    got = mc.run_dem(c.H, c.L, probs, trials, prior=c.prior, seed=9, max_iter=MC_ITERS, **kw)
    dec = fresh(c.H)
    (dec.relay_configure if second == "relay" else dec.gd_configure)(cfg)
    direct = dec.mc_run_probs(c.L, 0, probs, c.prior, 0, trials, seed=9, max_iter=MC_ITERS, flags=flag)
    print(second, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
    assert got[0] == trials and got[6] >= 64
    assert np.array_equal(got, direct)
