"""lsd_kernel on large, tall and near-limit matrices: dynamic LDS above 64 KiB (up to the 160 KiB limit and the refusal
one round further), the 32-bit per-lane row masks up to bit 31 (2048 rows, and the refusal of 2049), per-column priors,
long rows and columns and empty columns of a detector error model, the bitonic sort without padding and with almost
nothing but padding, many clusters alive at once in different 64-row passes, more records than workgroups when the LDS
leaves one workgroup per CU, and the records build behind QBP_FLAG_LSD -- against the numpy statement
(tests/lsd_oracle.py), bit for bit, into poisoned buffers.

The CPU tests (unmarked) assert, on the statement's output alone, that every case reaches the path it is named for; the
GPU tests assert the launch geometry the library reports (threads, grid, lds_bytes) against the restatement in lsd_util
and print it with the presence counts."""
import functools

import numpy as np
import pytest

import geometry_util as gu
import lsd_oracle as lo
import lsd_util as lu
import record_kernel_util as ru
import test_gpu_lsd as tl
from oracle import oracle
from qldpc_amd import _lib, bp
from test_gpu_record_kernel_sizes import mc_case, on_own_stream, spread

gpu = pytest.mark.gpu
TAGS = ("ph72x6", "ph72x12", "dem_synth")
FAMILIES = ("dense", "sparse")
G = (0, 1, 3)
RECORDS = 16                                # per tag and family
SOL_POISON, STAT_POISON = 0xAB, -77


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def bp_records(H, syn, prior, iters):
    """Sum-product BP(iters) of the CPU oracle -> (llr, hard, converged)."""
    hard, conv, _, llr = oracle.decode_batch(H, syn, prior, iters)
    return np.ascontiguousarray(llr, np.float64), np.ascontiguousarray(hard, np.uint8), np.asarray(conv, bool)


def make_special(H, syn, llr, hard):
    """Records 0 .. 3 as tests/test_gpu_lsd.py's `inputs` makes them: exact ties and a NaN in the llr, an all-zero
    residual, and two syndromes with one bit flipped (row 0, row m - 1)."""
    syn, llr = syn.copy(), llr.copy()
    llr[0] = np.round(llr[0])
    llr[0, 1] = np.nan
    syn[1] = hard[1].astype(np.int64) @ H.T % 2
    syn[2, 0] ^= 1
    syn[3, H.shape[0] - 1] ^= 1
    return syn, llr, hard


def show(res):
    """lsd_oracle.presence plus the classes of this file: records that end with >= 3 and >= 4 clusters, and with
    clusters whose lowest checks lie in >= 3 different 64-row blocks."""
    out = lo.presence(res)
    s = res["stats"]
    out.update(three_clusters=int((s[:, 2] >= 3).sum()), four_clusters=int((s[:, 2] >= 4).sum()),
               three_blocks=sum(len(set((np.asarray(x) // 64).tolist())) >= 3 for x in res["cluster_lows"]),
               most_rounds=int(s[:, 0].max()), most_active=int(s[:, 1].max()))
    return out


def device_lsd(dec, syn_t, llr_t, hard_t, B, n, stream=0):
    """One qbp_lsd_batch_device into poisoned outputs with one spare record behind each -> (solution, stats); the spare
    records must keep the poison."""
    t = gu.torch()
    sol_t = t.full((B + 1, n), SOL_POISON, dtype=t.uint8, device="cuda")
    st_t = t.full((B + 1, 4), STAT_POISON, dtype=t.int32, device="cuda")
    t.cuda.synchronize()
    dec.lsd_device(syn_t.data_ptr(), llr_t.data_ptr(), hard_t.data_ptr(), B, sol_t.data_ptr(), st_t.data_ptr(),
                   stream=stream or gu.stream_ptr())
    t.cuda.synchronize()
    assert bool((sol_t[B] == SOL_POISON).all()) and bool((st_t[B] == STAT_POISON).all()), "written beyond record B"
    assert dec.info("threads") == 64
    return sol_t[:B].cpu().numpy(), st_t[:B].cpu().numpy()


def check(dec, H, inputs, g, want, what, blocks=0):
    """Configure g, launch the whole batch, compare with the statement and with the restated geometry."""
    m, n = H.shape
    syn, llr, hard = inputs
    B = len(syn)
    dec.lsd_configure(g)
    sol, stats = device_lsd(dec, *(gu.to_device(a) for a in (syn, llr, hard)), B, n)
    info = ru.info(dec)
    print(what, "g", g, info, show(want))
    assert info == dict(threads=64, grid=lu.lsd_grid(m, n, B, dec.info("num_cu"), blocks), lds_bytes=lu.lsd_lds16(m, n))
    assert np.array_equal(stats, want["stats"]), (what, g, np.flatnonzero((stats != want["stats"]).any(1))[:8])
    assert np.array_equal(sol, want["solution"]), (what, g, np.flatnonzero((sol != want["solution"]).any(1))[:8])
    return info


# =========================================================================================================================
# 0. the launch arithmetic restated
# =========================================================================================================================
def test_lds_bytes_of_the_cases():
    for (m, n), want in (((216, 648), 27336), ((432, 1296), 89216), ((144, 595), 18412), ((2048, 384), 143888),
                         ((2049, 384), 143961)):
        assert lu.lsd_lds_bytes(m, n) == want
    for tag, shape in zip(TAGS, ((216, 648), (432, 1296), (144, 595))):
        assert ru.case(tag).H.shape == shape
    assert lu.rows2048().shape == (2048, 384) and lu.rows2048(True).shape == (2049, 384)
    # workgroups per CU: osd0_kernel's 32 on a small matrix, what the LDS holds on the larger ones, one above 80 KiB
    assert lu.lsd_grid(36, 72, 1 << 30, 256) == 256 * 32
    assert [lu.lsd_grid(*ru.case(tag).H.shape, 1 << 30, 256) for tag in TAGS] == [256 * 5, 256, 256 * 8]
    assert lu.lsd_grid(2048, 384, 1 << 30, 256) == 256 and lu.lsd_grid(216, 648, 1 << 30, 256, 1) == 256
    assert lu.lsd_grid(216, 648, 7, 256) == 7
    assert lu.lsd_lds_bytes(432, 1296) > ru.LDS_DEFAULT and lu.lsd_lds_bytes(216, 648) < ru.LDS_DEFAULT


def lsd_lds_of(sh):
    return lu.lsd_lds_bytes(sh.m, sh.n)


def test_near_limit_sixteen_rounds_fit_and_seventeen_do_not():
    assert ru.largest_rounds(lsd_lds_of) == 16
    assert lsd_lds_of(ru.ph_shape(16)) == 147536 and (ru.ph_shape(16).m, ru.ph_shape(16).n) == (576, 1728)
    assert lsd_lds_of(ru.ph_shape(17)) == 166292 > lu.LDS_LIMIT
    assert ru.LDS_DEFAULT < 147536 <= lu.LDS_LIMIT == ru.LDS_LIMIT


# =========================================================================================================================
# 1. the batch kernel against the statement on the large cases
# =========================================================================================================================
@functools.lru_cache(maxsize=None)
def large_inputs(tag, family):
    """RECORDS failures of the CPU oracle's sum-product BP with the case's own per-column prior -- dense: BP(8) on
    ru.case(tag); sparse: BP(1) on the first 160 rows of ru.pool(tag) -- the first four made special."""
    c = ru.case(tag) if family == "dense" else ru.pool(tag).subset(np.arange(160))
    llr, hard, conv = bp_records(c.H, c.syn, c.prior, 8 if family == "dense" else 1)
    f = np.flatnonzero(~conv)[:RECORDS]
    assert len(f) == RECORDS, (tag, family, len(f))
    return make_special(c.H, c.syn[f], llr[f], hard[f])


@functools.lru_cache(maxsize=None)
def large_ref(tag, family, g):
    return lo.lsd_decode_batch(ru.case(tag).H, *large_inputs(tag, family), g)


def test_large_cases_show_every_situation():
    """Pooled over the three matrices, both families and the three step sizes, on the statement's output."""
    pooled = {}
    for tag in TAGS:
        for family in FAMILIES:
            for g in G:
                one = show(large_ref(tag, family, g))
                print(tag, family, g, one)
                for k, v in one.items():
                    pooled[k] = pooled.get(k, 0) + v
    print(pooled)
    for k in ("merged", "skipped", "three_rounds", "four_clusters"):
        assert pooled[k] >= 8, (k, pooled)
    assert pooled["three_blocks"] >= 4 and pooled["trivial"] >= 1, pooled


def test_dem_synth_activates_heavy_columns_and_never_an_empty_one():
    H = ru.case("dem_synth").H
    col_w = H.sum(0)
    assert (col_w == 0).sum() == 3 and col_w.max() >= 5 and H.sum(1).max() > 8
    heavy = 0
    for family in FAMILIES:
        for g in G:
            active = large_ref("dem_synth", family, g)["active"]
            assert not active[:, col_w == 0].any()
            heavy += int(active[:, col_w >= 5].sum())
    print("activations of columns of weight >= 5:", heavy)
    assert heavy >= 1
    assert len(np.unique(ru.case("dem_synth").prior)) > 150


@gpu
@pytest.mark.parametrize("g", G)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("tag", TAGS)
def test_large_batch_equals_statement(tag, family, g):
    H = ru.case(tag).H
    check(fresh(H), H, large_inputs(tag, family), g, large_ref(tag, family, g), f"{tag} {family}")


# =========================================================================================================================
# 2. near the 160 KiB limit
# =========================================================================================================================
NEAR_T, NEAR_B = 16, 8


@functools.lru_cache(maxsize=None)
def near_inputs():
    """The 8 records of ru.phenomenological(16, 0.01, ., 8): what BP(8) leaves where it fails, what BP(1) leaves on
    the others (where it fails as well)."""
    c = ru.phenomenological(NEAR_T, 0.01, 100 + NEAR_T, NEAR_B)
    llr, hard, conv = bp_records(c.H, c.syn, c.prior, 8)
    llr1, hard1, conv1 = bp_records(c.H, c.syn, c.prior, 1)
    assert not (conv & conv1).any(), "a record neither BP(8) nor BP(1) fails on"
    llr[conv], hard[conv] = llr1[conv], hard1[conv]
    return c.H, c.syn, llr, hard, int((~conv).sum())


@functools.lru_cache(maxsize=None)
def near_ref(g):
    H, syn, llr, hard, _ = near_inputs()
    return lo.lsd_decode_batch(H, syn, llr, hard, g)


def test_near_limit_records_do_real_work():
    H, syn, llr, hard, from_bp8 = near_inputs()
    assert H.shape == (576, 1728) and len(syn) == NEAR_B
    one, zero = show(near_ref(1)), show(near_ref(0))
    print("BP(8) failures", from_bp8, one, zero)
    for counts in (one, zero):          # (the only other matrix above 64 KiB in the suite sees neither of these)
        assert counts["trivial"] == 0 and counts["merged"] >= 1 and counts["skipped"] >= 1 and counts["two_clusters"] >= 1
    assert one["three_rounds"] >= 1


@gpu
def test_near_limit_decodes_and_one_round_more_is_unsupported():
    H, syn, llr, hard, _ = near_inputs()
    m, n = H.shape
    dec = fresh(H)
    for g in (1, 0):
        info = check(dec, H, (syn, llr, hard), g, near_ref(g), f"ph72x{NEAR_T}")
        assert info["grid"] == NEAR_B and ru.LDS_DEFAULT < info["lds_bytes"] <= lu.LDS_LIMIT
    # a second, smaller launch on the same handle, after the attribute was raised
    want = near_ref(0)
    sol, stats = device_lsd(dec, *(gu.to_device(a[:3]) for a in (syn, llr, hard)), 3, n)
    assert dec.info("grid") == 3
    assert np.array_equal(sol, want["solution"][:3]) and np.array_equal(stats, want["stats"][:3])
    # one round more: refused, and a launch on that handle touches no output
    big = ru.phenomenological(NEAR_T + 1, 0.01, 100 + NEAR_T, 2)
    assert lu.lsd_lds_bytes(*big.H.shape) > lu.LDS_LIMIT
    dec2 = fresh(big.H)
    with pytest.raises(_lib.QbpError) as e:
        dec2.lsd_configure(1)
    assert e.value.code == _lib.E_UNSUPPORTED and b"160 KiB" in _lib.load().qbp_last_error()
    t = gu.torch()
    syn_t, llr_t, hard_t = (gu.to_device(a) for a in (big.syn, np.ones((2, big.n)), np.zeros((2, big.n), np.uint8)))
    sol_t = t.full((2, big.n), SOL_POISON, dtype=t.uint8, device="cuda")
    st_t = t.full((2, 4), STAT_POISON, dtype=t.int32, device="cuda")
    with pytest.raises(_lib.QbpError) as e:
        dec2.lsd_device(syn_t.data_ptr(), llr_t.data_ptr(), hard_t.data_ptr(), 2, sol_t.data_ptr(), st_t.data_ptr())
    assert e.value.code in (_lib.E_UNSUPPORTED, _lib.E_INVALID)
    t.cuda.synchronize()
    assert bool((sol_t == SOL_POISON).all()) and bool((st_t == STAT_POISON).all())


# =========================================================================================================================
# 3. the row masks up to bit 31
# =========================================================================================================================
ROWS_B = 16


@functools.lru_cache(maxsize=None)
def rows_inputs():
    """BP converges on everything for so redundant a matrix, so no BP outputs: errors of weight 4 .. 12 with a bit in
    the lower block (columns 0 .. 31), in the upper block (352 .. 383) and between, `hard` 0 or sparse, and a noisy llr:
    a noisy prior times a random factor that tends to be smaller on the columns of the error (overlapping ranges: some
    clusters find their error at once, others grow first; with a factor blind to the error the clusters between the
    blocks grow column by column over all 320 columns, hundreds of rounds of the numpy statement on 2048 rows).  The
    last two records have a syndrome bit flipped in row 2047 and in row 0 (outside the column space)."""
    H = lu.rows2048()
    m, n = H.shape
    rng = np.random.default_rng(31)
    errors = np.zeros((ROWS_B, n), np.uint8)
    for b in range(ROWS_B):
        w = int(rng.integers(4, 13))
        errors[b, rng.integers(0, 32)] = errors[b, 352 + rng.integers(0, 32)] = 1
        errors[b, 32 + rng.choice(320, w - 2, replace=False)] = 1
    syn = gu.syndromes_of(H, errors)
    factor = np.where(errors == 1, rng.uniform(0.05, 0.6, (ROWS_B, n)), rng.uniform(0.4, 1.6, (ROWS_B, n)))
    llr = ru.noisy_prior(0.02, n, rng) * factor
    hard = np.zeros((ROWS_B, n), np.uint8)
    hard[1::2] = rng.random((ROWS_B // 2, n)) < 0.01
    syn[ROWS_B - 2, m - 1] ^= 1
    syn[ROWS_B - 1, 0] ^= 1
    return H, syn, np.ascontiguousarray(llr), hard


@functools.lru_cache(maxsize=None)
def rows_ref(g):
    return lo.lsd_decode_batch(*rows_inputs(), g)


def test_rows2048_reaches_bit_31_of_the_row_masks():
    H, syn, llr, hard = rows_inputs()
    assert H.shape == (lu.MAX_ROWS, 384) and not H[:1984, 352:].any() and not H[64:, :32].any()
    residual = (syn + hard.astype(np.int64) @ H.T) % 2
    assert sum(int(r[1984:].any()) for r in residual) >= 8            # seeds in the last 64-row pass
    for g in (0, 1):
        want = rows_ref(g)
        one = show(want)
        print(g, one)
        assert sum(len(p) > 0 and p.max() >= 1984 for p in want["pivot_rows"]) >= 8
        assert sum(len(p) > 0 and p.min() < 64 for p in want["pivot_rows"]) >= 8
        assert one["invalid"] >= 2 and want["stats"][ROWS_B - 2, 3] == 0 and want["stats"][ROWS_B - 1, 3] == 0
        assert one["three_clusters"] >= 8


@gpu
@pytest.mark.parametrize("g", [0, 1])
def test_rows2048_equals_statement(g):
    H, syn, llr, hard = rows_inputs()
    check(fresh(H), H, (syn, llr, hard), g, rows_ref(g), "rows2048")


@gpu
def test_2049_rows_are_unsupported_by_the_row_limit_alone():
    H = lu.rows2048(extra_row=True)
    assert H.shape == (lu.MAX_ROWS + 1, 384) and lu.lsd_lds_bytes(*H.shape) == 143961 < lu.LDS_LIMIT
    lib = _lib.load()
    dec = fresh(H)
    assert lib.qbp_lsd_configure(dec._h, 1) == _lib.E_UNSUPPORTED
    assert b"2048 rows" in lib.qbp_last_error() and tl.re_bytes(lib.qbp_last_error()) == 143961
    with pytest.raises(_lib.QbpError):
        dec.lsd(np.zeros((1, 2049), np.uint8), np.ones((1, 384)), np.zeros((1, 384), np.uint8), want_stats=False)


# =========================================================================================================================
# 4. the bitonic sort without padding, and with 255 padding keys
# =========================================================================================================================
SORT_B, SORT_P = 32, 0.04


@functools.lru_cache(maxsize=None)
def sort_inputs(n):
    """32 BP(50) outputs; in every record half the llr entries repeat the magnitude of another with the opposite sign,
    and +inf, -inf and two NaNs sit at record-dependent places: the column index decides the order."""
    H = lu.sort_edge(n)
    syn, llr, hard, conv = lu.bp_outputs(H, SORT_P, 3, SORT_B, 50)
    rng = np.random.default_rng(n)
    llr = llr.copy()
    for b in range(SORT_B):
        perm = rng.permutation(n)
        half = n // 4
        llr[b, perm[:half]] = -llr[b, perm[half:2 * half]]
        llr[b, perm[2 * half]], llr[b, perm[2 * half + 1]] = np.inf, -np.inf
        llr[b, perm[2 * half + 2]] = llr[b, perm[2 * half + 3]] = np.nan
    return H, syn, llr, hard, int((~conv).sum())


@functools.lru_cache(maxsize=None)
def sort_ref(n, g):
    return lo.lsd_decode_batch(*sort_inputs(n)[:4], g)


@pytest.mark.parametrize("n", [256, 257])
def test_sort_edge_inputs(n):
    H, syn, llr, hard, failures = sort_inputs(n)
    NP = 1 << (n - 1).bit_length()
    assert H.shape == (100, n) and NP == (256 if n == 256 else 512) and NP - n == (0 if n == 256 else 255)
    assert 8 <= failures <= 24, failures
    keys = lo.order_keys(llr)
    assert all(len(np.unique(k)) <= n - n // 4 - 1 for k in keys)      # ties: a quarter of the keys twice, two NaNs
    assert np.isinf(llr).sum(1).tolist() == [2] * SORT_B and np.isnan(llr).sum(1).tolist() == [2] * SORT_B
    for g in (0, 1):
        one = show(sort_ref(n, g))
        print(n, g, "failures", failures, one)
        assert one["merged"] >= 8 and one["skipped"] >= 1 and (g == 0 or one["three_rounds"] >= 8)


@gpu
@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("n", [256, 257])
def test_sort_edge_equals_statement(n, g):
    H, syn, llr, hard, _ = sort_inputs(n)
    check(fresh(H), H, (syn, llr, hard), g, sort_ref(n, g), f"sort_edge {n}")


# =========================================================================================================================
# 5. more records than workgroups, one workgroup per CU
# =========================================================================================================================
def both_families(tag, g):
    ins = [large_inputs(tag, f) for f in FAMILIES]
    refs = [large_ref(tag, f, g) for f in FAMILIES]
    return tuple(np.concatenate([x[i] for x in ins]) for i in range(3)), \
        {k: np.concatenate([r[k] for r in refs]) for k in ("solution", "stats")}


@gpu
@pytest.mark.parametrize("tag,blocks", [("ph72x12", 0), ("ph72x6", 1)], ids=["lds_limited", "one_per_cu"])
def test_item_striding_with_one_workgroup_per_cu(tag, blocks):
    H = ru.case(tag).H
    m, n = H.shape
    (syn, llr, hard), want = both_families(tag, 1)
    dec = fresh(H)
    dec.lsd_configure(1)
    grid_full = lu.lsd_grid(m, n, 1 << 30, dec.info("num_cu"), blocks)
    assert grid_full == dec.info("num_cu")
    B = 2 * grid_full + 37
    idx = spread(B, len(syn), 5)
    syn_t, llr_t, hard_t = (gu.to_device(a[idx]) for a in (syn, llr, hard))
    got = []
    with gu.options(dec, blocks=blocks):
        on_own_stream(lambda s: got.extend(device_lsd(dec, syn_t, llr_t, hard_t, B, n, stream=s)))
    info = ru.info(dec)
    print(tag, "blocks", blocks, info, "B", B)
    assert info == dict(threads=64, grid=grid_full, lds_bytes=lu.lsd_lds16(m, n)) and B > info["grid"]
    assert np.array_equal(got[1], want["stats"][idx]), np.flatnonzero((got[1] != want["stats"][idx]).any(1))[:8]
    assert np.array_equal(got[0], want["solution"][idx])


# =========================================================================================================================
# 6. the records build on the larger matrices
# =========================================================================================================================
def mc_check(tag, first, g, blocks=0, trials=None, rate=None):
    H, L, d, errors, prior = mc_case(tag, trials, rate)
    variant = _lib.MIN_SUM if first == "min_sum" else _lib.SUM_PRODUCT
    dec = fresh(H)
    dec.lsd_configure(g)
    want, failures = tl.compose(dec, H, L, d, errors, prior, g, variant, False)
    with gu.options(dec, blocks=blocks):
        got = dec.mc_run_errors(L, d, errors, prior, max_iter=tl.MC_ITERS, variant=variant, alpha=tl.ALPHA,
                                flags=_lib.FLAG_LSD)
    info = ru.info(dec)
    print(tag, first, "g", g, "blocks", blocks, dict(zip(_lib.COUNTER_NAMES, got.tolist())), "failures", failures, info)
    assert info == dict(threads=64, grid=lu.lsd_grid(*H.shape, len(errors), dec.info("num_cu"), blocks),
                        lds_bytes=lu.lsd_lds16(*H.shape))
    assert failures >= 64 and got[6] == failures and got[0] == len(errors)
    assert np.array_equal(got, want)
    return failures, info


@gpu
@pytest.mark.parametrize("first,g", [("sum_product", 1), ("min_sum", 1), ("sum_product", 0)])
@pytest.mark.parametrize("tag", ["ph72x6", "dem_synth"])
def test_mc_run_errors_equals_the_composition(tag, first, g):
    mc_check(tag, first, g)


@gpu
def test_lsd_records_beyond_the_grid():
    """More failure records than workgroups: one workgroup per CU, and twice the trials of the case above."""
    failures, info = mc_check("ph72x6", "sum_product", 1, blocks=1, trials=448, rate=0.03)
    assert failures > info["grid"]
