"""GPU: the BP kernels across launch geometries, into poisoned output buffers (tests/geometry_util.py).

The other test files pin the arithmetic of the kernels at whatever geometry "auto" picks for their batch on the card
they run on.  Here the arithmetic is taken as given and the machinery around it is varied: slots per workgroup,
workgroups per CU, workgroup width, memory mode, batch sizes at which the shared work counter is unused, used once,
and used through every chunk size down to a ragged tail.  Every comparison is bit for bit.  The reference is the CPU
oracle: a batch is decoded once at the default geometry and compared with oracle.decode_batch (all of it when it is
small, else a fixed random subset of at least 1500 syndromes plus every non-converged one); every other geometry is
compared with that result.  All decodes go through qbp_decode_batch_device with torch tensors, whose outputs are
poisoned before each launch."""
import numpy as np
import pytest

import geometry_util as gu
from budget_oracle import ladder_counters
from oracle import oracle
from qldpc_amd import _lib, bp, codes, mc, shots
from spectrum_oracle import check_identities, spectrum_counters

gpu = pytest.mark.gpu

SP = dict(variant=_lib.SUM_PRODUCT)
DAMPED = dict(variant=_lib.DAMPED_SP, alpha=0.9, damping=0.8, clip_llr=20.0)
MINSUM = dict(variant=_lib.MIN_SUM, alpha=0.8, damping=0.7, clip_llr=25.0)
FUSED = ("[[72, 12, 6]]", "[[144, 12, 12]]", "[[288, 12, 18]]", "steane", "irregular", "st72x2")
P_EASY, P_HARD = 0.02, 0.07

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- matrices -----------------------------------------------------------------------------------------------------
def space_time(H, T):
    """spaceTime.py:4-18, as tests/test_gpu_parity.py::test_large_spacetime_matrix_vs_oracle builds it."""
    m = H.shape[0]
    Hs = np.kron(np.eye(T, dtype=np.int64), H)
    Ht = (np.eye(m * T, dtype=np.int64) + np.eye(m * T, k=-m, dtype=np.int64)) % 2
    return np.hstack([Hs, Ht])


def matrix(name):
    def make():
        if name == "irregular":          # the padded (6, 3)-class matrix of test_first_check_step_table_changes_nothing
            rng = np.random.default_rng(5)
            H = (rng.random((40, 90)) < 0.05).astype(np.int64)
            H[:, 0] = 0
            H[3] = 0
            H[3, :2] = 1
            H = H[(H.sum(1) <= 6)]
            return H[:, H.sum(0) <= 3]
        if name == "st72x2":             # (8, 4) class: 72 x 216
            return space_time(codes.load_code("[[72, 12, 6]]").Hx, 2)
        if name == "st144x12":           # 864 x 2592
            return space_time(codes.load_code("[[144, 12, 12]]").Hx, 12)
        if name == "long_row":           # general-H only: a row of weight 22 (the long-row path), an empty column
            rng = np.random.default_rng(12)
            H = (rng.random((24, 60)) < 0.12).astype(np.int64)
            H[0] = 0
            H[0, 3:25] = 1
            H[:, 40] = 0
            assert H[0].sum() == 22 and not H[:, 40].any()
            return H
        return np.ascontiguousarray(codes.load_code(name).Hx).astype(np.int64)
    return cached(("H", name), make)


def decoder(name):
    """A Decoder of this module's own (options set here never reach the decoders other test files share)."""
    return cached(("dec", name), lambda: _lib.Decoder(*bp.csr_from_H(matrix(name))))


# ---- reference batches ----------------------------------------------------------------------------------------------
class Batch:
    """`rows` syndromes of one matrix at error rate p: device copies, one poisoned output set, and the result of the
    default geometry, checked against the oracle (per decode mode, on first use)."""

    def __init__(self, name, p, rows, seed):
        self.name, self.p, self.rows = name, p, rows
        self.H = matrix(name)
        self.m, self.n = self.H.shape
        rng = np.random.default_rng([seed, rows])
        self.syn = gu.syndromes_of(self.H, rng.random((rows, self.n)) < p)
        self.prior = np.full(self.n, np.log((1 - p) / p))
        self.syn_t, self.prior_t = gu.to_device(self.syn), gu.to_device(self.prior)
        self.out = gu.Outputs(rows, self.n)
        self.refs = {}

    def decode(self, dec, B, what, max_iter=50, flags=0, nulls=(), **kw):
        return gu.decode(dec, self.syn_t, self.prior_t, B, self.out, what, max_iter=max_iter, flags=flags,
                         nulls=nulls, **kw)

    def reference(self, dec, max_iter=50, **kw):
        key = (max_iter,) + tuple(sorted(kw.items()))
        if key not in self.refs:
            what = f"{self.name} p={self.p} default geometry {kw}"
            ref = self.decode(dec, self.rows, what, max_iter=max_iter, **kw)
            conv = ref[1]
            if self.rows <= 4000:
                sub = np.arange(self.rows)
            else:
                pick = np.random.default_rng(self.rows).choice(self.rows, 2000, replace=False)
                sub = np.union1d(pick, np.flatnonzero(~conv))
            o = oracle.decode_batch(self.H, self.syn[sub], self.prior, max_iter, threads=8, **kw)
            gu.assert_same(tuple(x[sub] for x in ref), (o[0], o[1], o[2], o[3]), what + " vs oracle")
            print(f"REF {what}: B={self.rows} grid={dec.info('grid')} threads={dec.info('threads')} oracle on "
                  f"{len(sub)}, {int((~conv).sum())} not converged, mean iteration {ref[2].mean():.2f}")
            self.refs[key] = ref
        return self.refs[key]

    def drop_mode_references(self):
        """Keep the plain sum-product reference only (the others are as large and used by one test each)."""
        self.refs = {k: v for k, v in self.refs.items() if k == (50,)}


def fused_rows(name, num_cu):
    m = matrix(name).shape[0]
    need = [gu.ragged_batch(m, num_cu, deep=True)]
    for S in gu.slot_values(m) + [gu.FUSED_MAX_THREADS // m]:
        for blocks in (0, 1, 4):
            need.append(gu.several_rounds_batch(S, blocks, m, num_cu))
    return max(need)


def easy_batch(name):
    dec = decoder(name)
    return cached(("easy", name), lambda: Batch(name, P_EASY, fused_rows(name, dec.info("num_cu")), 1))


def hard_batch(name):
    dec = decoder(name)
    return cached(("hard", name), lambda: Batch(name, P_HARD, 12 * dec.info("num_cu") + 7, 2))


def run_fused(name, batch, S, blocks, B, full_wg=0, two_barriers=0, max_iter=50, flags=0, **kw):
    """One on-chip launch of the first B syndromes of `batch` at geometry (S, blocks): poisoned outputs, the geometry
    the library reports checked against the options, the result compared with the default geometry's."""
    dec = decoder(name)
    assert 1 <= B <= batch.rows, (name, S, blocks, B, batch.rows)
    ref = batch.reference(dec, max_iter=max_iter, **kw)            # (forced iterations change no output)
    num_cu, m = dec.info("num_cu"), batch.m
    forced = bool(flags & _lib.FLAG_FORCE_FULL)
    what = f"{name} p={batch.p} S={S} blocks={blocks} full_wg={full_wg} B={B} flags={flags} max_iter={max_iter} {kw}"
    with gu.options(dec, slots=S, blocks=blocks, full_wg=full_wg, two_barriers=two_barriers):
        got = batch.decode(dec, B, what, max_iter=max_iter, flags=flags, **kw)
        grid, threads = dec.info("grid"), dec.info("threads")
        assert dec.info("last_kernel") == 1
        if forced:
            assert dec.info("one_barrier") == (0 if two_barriers or name == "st72x2" else 1), what
    S_eff = gu.expected_slots(m, B, num_cu, S, forced, full_wg)
    print(f"GEOM {name} p={batch.p} S={S}->{S_eff} blocks={blocks} full_wg={full_wg} B={B} grid={grid} "
          f"threads={threads} flags={flags} max_iter={max_iter} variant={kw.get('variant', 0)}")
    assert threads == gu.threads_of(S_eff, m), (what, "threads", threads, "slots", S_eff)
    want_wgs = -(-B // S_eff)
    if blocks:
        assert grid == min(want_wgs, num_cu * blocks), (what, "grid", grid)
    else:
        assert grid == want_wgs or (grid % num_cu == 0 and grid <= num_cu * gu.auto_blocks_bound(S_eff, m)), (what, grid)
    gu.assert_same(got, tuple(x[:B] for x in ref), what + f" grid={grid} threads={threads}")
    return grid, S_eff


# ---- CPU: the batch sizes reach what they are meant to reach ----------------------------------------------------------
@pytest.mark.parametrize("m,f", [(3, 4), (28, 4), (36, 4), (72, 2), (144, 1)])
def test_batch_size_formulas_reach_every_chunk_size(m, f):
    """work_chunk's thresholds, restated in geometry_util: with one slot per workgroup and one workgroup per CU the
    batch of 17 f syndromes per slot hands out chunks of 8 f, 8, 4, 2 and 1 and ends on a ragged tail.  The first
    fetch of every slot is judged at 9 syndromes per slot handed out, where 17 f - 9 per slot are too few for the
    small-code chunk 8 f (only the slots that come back first get one), so a second batch of 33 f per slot is run as
    well, whose first fetch is 8 f for every slot.  Every index is handed out exactly once in both."""
    num_cu = 256
    assert gu.chunk_factor(m) == f
    for deep in (False, True):
        B = gu.ragged_batch(m, num_cu, deep)
        sizes, seen = gu.simulate_chunks(B, num_cu, m)
        assert (seen == 1).all()
        assert {8 * f, 8, 4, 2, 1} <= set(sizes)
        assert (B - num_cu) % 8 and sum(sizes) > B - num_cu          # the last chunks reach beyond B
        assert sizes[0] == (8 * f if deep else 8 if f > 1 else 4)
    # cheap syndromes (the running-cost rule asks for 8): no later chunk below 8, still every index once
    sizes, seen = gu.simulate_chunks(gu.ragged_batch(m, num_cu), num_cu, m, by_cost=8)
    assert min(sizes[num_cu:]) == 8 and (seen == 1).all()
    # the slot counts of the tests: S * m <= 1024, one of them off the 64-lane grid
    S = gu.slot_values(m)
    assert len(set(S)) == 4 and max(S) * m <= 1024 < (max(S) + 1) * m and (S[3] * m) % 64


# ---- A. on-chip kernel ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", FUSED)
def test_fused_geometry_product(name):
    """Plain sum-product with early exit: slots {auto, 1, 2, max, off the 64-lane grid} x workgroups per CU
    {auto, 1, 4} x QBP_OPT_EARLY_EXIT_FULL_WG {0, 1} (which only the automatic slot count looks at).  S = 1 with one
    workgroup per CU runs the ragged batches of 17 f and 33 f syndromes per slot, the others a little more than four
    rounds of the grid."""
    dec = decoder(name)
    assert dec.info("kernel_kind") == 1
    num_cu, m = dec.info("num_cu"), matrix(name).shape[0]
    batch = easy_batch(name)
    seen_auto = set()
    for S in [0] + gu.slot_values(m):
        for blocks in (0, 1, 4):
            for full_wg in (0, 1):
                S_big = S or gu.auto_slots(m, batch.rows, num_cu, False, full_wg)
                sizes = [gu.several_rounds_batch(S_big, blocks, m, num_cu)]
                if S == 1 and blocks == 1:
                    sizes = [gu.ragged_batch(m, num_cu), gu.ragged_batch(m, num_cu, deep=True)]
                for B in sizes:
                    grid, S_eff = run_fused(name, batch, S, blocks, B, full_wg=full_wg)
                    if blocks:
                        assert grid == num_cu * blocks and B > 4 * grid * S_eff
                    if S == 0:
                        seen_auto.add(S_eff)
    assert len(seen_auto) == (2 if 512 // m >= 1 and 1024 // m >= 2 else 1)     # full_wg took effect


@gpu
@pytest.mark.parametrize("name", FUSED)
def test_fused_degenerate_batch_sizes(name):
    """B = 1, B = S - 1 (the library shrinks the only workgroup to the batch: idle lanes, no idle slot), B = S + 1 (all
    but one slot of the second workgroup idle), B = grid * S exactly (the work counter is never read and its memset
    skipped), B = grid * S + 1 (one slot reads it once)."""
    dec = decoder(name)
    num_cu, m = dec.info("num_cu"), matrix(name).shape[0]
    batch = easy_batch(name)
    one, two, smax, odd = gu.slot_values(m)
    for S, blocks in ((smax, 1), (odd, 4), (two, 1), (one, 4)):
        full = num_cu * blocks * S
        for B in sorted({1, max(S - 1, 1), S + 1, full, full + 1}):
            grid, S_eff = run_fused(name, batch, S, blocks, B)
            if B >= full:
                assert grid * S_eff == full


@gpu
@pytest.mark.parametrize("name", FUSED)
def test_fused_other_modes(name):
    """Forced iterations (one-barrier and two-barrier kernels), the two damped variants and max_iter = 1, each at
    S = 1 / one workgroup per CU (ragged batch), at an off-grid S with four workgroups per CU, and at the largest S
    with the automatic count."""
    dec = decoder(name)
    num_cu, m = dec.info("num_cu"), matrix(name).shape[0]
    batch = easy_batch(name)
    one, two, smax, odd = gu.slot_values(m)
    geoms = ((one, 1, gu.ragged_batch(m, num_cu)), (odd, 4, gu.several_rounds_batch(odd, 4, m, num_cu)),
             (smax, 0, gu.several_rounds_batch(smax, 0, m, num_cu)))
    modes = (dict(flags=_lib.FLAG_FORCE_FULL), dict(flags=_lib.FLAG_FORCE_FULL, two_barriers=1),
             dict(flags=_lib.FLAG_FORCE_FULL, max_iter=7, **DAMPED), DAMPED, MINSUM, dict(max_iter=1),
             dict(max_iter=1, flags=_lib.FLAG_FORCE_FULL))
    try:
        for mode in modes:
            for S, blocks, B in geoms:
                run_fused(name, batch, S, blocks, B, **mode)
    finally:
        batch.drop_mode_references()


@gpu
@pytest.mark.parametrize("name", FUSED)
def test_fused_many_iterations(name):
    """p = 0.07: many syndromes run to max_iter beside ones that stop at once -- the cost-based chunk rule, and slots
    of one workgroup that finish far apart."""
    dec = decoder(name)
    m = matrix(name).shape[0]
    batch = hard_batch(name)
    ref = batch.reference(dec)
    if name.startswith("[["):
        assert (~ref[1]).sum() > batch.rows // 20 and (ref[1] & (ref[2] == 0)).sum() > 0
    one, two, smax, odd = gu.slot_values(m)
    for S, blocks in ((one, 1), (two, 1), (odd, 1), (smax, 1), (0, 0), (0, 1)):
        for mode in ({}, dict(flags=_lib.FLAG_FORCE_FULL), MINSUM):
            run_fused(name, batch, S, blocks, batch.rows, **mode)


@gpu
def test_geometry_options_out_of_range_are_refused_on_the_host():
    """qbp_set_option answers QBP_E_INVALID before any GPU work, and the refused value does not stick."""
    name = "[[144, 12, 12]]"
    dec = decoder(name)
    m = matrix(name).shape[0]
    batch = hard_batch(name)
    for opt, value in (("slots", 1024 // m + 1), ("slots", -1), ("blocks", 33), ("blocks", -1), ("threads", 1025),
                       ("threads", -1), ("mem", 3), ("kernel", 4)):
        with pytest.raises(_lib.QbpError) as e:
            dec.set_option(gu.OPTS[opt], value)
        assert e.value.code == -1, (opt, value)
    run_fused(name, batch, 0, 0, batch.rows)


# ---- B. Monte-Carlo builds ----------------------------------------------------------------------------------------------
MC_T, MC_SEED, MC_BEGIN, MC_ITER = 30000, 11, 5, 50
MC_SPLIT = 11111                       # a range is also run as [0, MC_SPLIT) + [MC_SPLIT, MC_T): the last launch of run()
MC_BUDGETS = (2, 5, MC_ITER)
MC_CODES = ("[[72, 12, 6]]", "[[144, 12, 12]]")


def mc_geometries(m):
    return ((0, 0), (1, 1), (gu.FUSED_MAX_THREADS // m, 4))          # the first one is the reference: auto


def mc_setup(name):
    code = codes.load_code(name)
    return code, decoder(name), mc.prior_of(P_EASY, code.n), np.full(code.n, P_EASY)


def counters_tensor(rows=1, start=0):
    t = gu.torch()
    return t.full((rows, _lib.NUM_COUNTERS), start, dtype=t.int64, device="cuda")


def across_geometries(dec, m, run):
    """run() at every geometry; all results equal the first (automatic) one, which is returned."""
    results = []
    for S, blocks in mc_geometries(m):
        with gu.options(dec, slots=S, blocks=blocks):
            results.append(run())
            assert dec.info("last_kernel") == 1
            print(f"MC-GEOM S={S} blocks={blocks} grid={dec.info('grid')} threads={dec.info('threads')}")
            if S:
                assert dec.info("threads") == gu.threads_of(S, m)
                assert dec.info("grid") == min(-(-(MC_T - MC_SPLIT) // S), dec.info("num_cu") * blocks)
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert np.array_equal(a, b), (a, b)
    return results[0]


@gpu
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
@pytest.mark.parametrize("name", MC_CODES)
def test_mc_run_across_geometries(name, osd):
    code, dec, prior, _ = mc_setup(name)
    flags = _lib.FLAG_OSD0 if osd else 0
    prior_t = gu.to_device(prior)
    a, b, mid = MC_BEGIN, MC_BEGIN + MC_T, MC_BEGIN + MC_SPLIT

    def run():
        whole = dec.mc_run(code.Lx, code.distance, P_EASY, prior, a, b, seed=MC_SEED, max_iter=MC_ITER, flags=flags)
        assert whole[0] == MC_T
        cnt = counters_tensor()
        for lo, hi in ((a, mid), (mid, b)):          # two calls ADD to the same device counters
            dec.mc_run_device(code.Lx, code.distance, P_EASY, prior_t.data_ptr(), lo, hi, cnt.data_ptr(), seed=MC_SEED,
                              max_iter=MC_ITER, flags=flags, stream=gu.stream_ptr())
        gu.torch().cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy()[0], whole)
        return (whole,)

    got = across_geometries(dec, code.Hx.shape[0], run)[0]
    want = oracle.mc_counters(code.Hx, code.Lx, code.distance, P_EASY, prior, a, b, seed=MC_SEED, max_iter=MC_ITER,
                              osd=osd)
    assert np.array_equal(got, want), (got, want)
    assert got[6] > 0


@gpu
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
@pytest.mark.parametrize("name", MC_CODES)
def test_mc_run_probs_across_geometries(name, osd):
    code, dec, prior, probs = mc_setup(name)
    flags = _lib.FLAG_OSD0 if osd else 0
    prior_t = gu.to_device(prior)
    a, b, mid = MC_BEGIN, MC_BEGIN + MC_T, MC_BEGIN + MC_SPLIT

    def run():
        whole = dec.mc_run_probs(code.Lx, code.distance, probs, prior, a, b, seed=MC_SEED, max_iter=MC_ITER, flags=flags)
        assert whole[0] == MC_T
        cnt = counters_tensor()
        for lo, hi in ((a, mid), (mid, b)):
            dec.mc_run_probs_device(code.Lx, code.distance, probs, prior_t.data_ptr(), lo, hi, cnt.data_ptr(),
                                    seed=MC_SEED, max_iter=MC_ITER, flags=flags, stream=gu.stream_ptr())
        gu.torch().cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy()[0], whole)
        return (whole,)

    got = across_geometries(dec, code.Hx.shape[0], run)[0]
    # (probs filled with p draws the bits of qbp_mc_run(p): include/qbp.h)
    want = oracle.mc_counters(code.Hx, code.Lx, code.distance, P_EASY, prior, a, b, seed=MC_SEED, max_iter=MC_ITER,
                              osd=osd)
    assert np.array_equal(got, want), (got, want)


@gpu
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
@pytest.mark.parametrize("name", MC_CODES)
def test_mc_run_budgets_across_geometries(name, osd):
    code, dec, prior, probs = mc_setup(name)
    flags = _lib.FLAG_OSD0 if osd else 0
    prior_t = gu.to_device(prior)
    a, b, mid = MC_BEGIN, MC_BEGIN + MC_T, MC_BEGIN + MC_SPLIT

    def run():
        whole = dec.mc_run_budgets(code.Lx, code.distance, probs, prior, MC_BUDGETS, a, b, seed=MC_SEED, flags=flags)
        assert (whole[:, 0] == MC_T).all()
        cnt = counters_tensor(len(MC_BUDGETS))
        for lo, hi in ((a, mid), (mid, b)):
            dec.mc_run_budgets_device(code.Lx, code.distance, probs, prior_t.data_ptr(), MC_BUDGETS, lo, hi,
                                      cnt.data_ptr(), seed=MC_SEED, flags=flags, stream=gu.stream_ptr())
        gu.torch().cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), whole)
        return (whole,)

    got = across_geometries(dec, code.Hx.shape[0], run)[0]
    want = ladder_counters(code.Hx, code.Lx, code.distance, P_EASY, prior, a, b, MC_BUDGETS, seed=MC_SEED, osd=osd)
    assert np.array_equal(got, want), (got, want)
    assert got[0, 6] > got[-1, 6] > 0


@gpu
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
@pytest.mark.parametrize("name", MC_CODES)
def test_mc_run_spectrum_across_geometries(name, osd):
    code, dec, prior, probs = mc_setup(name)
    flags = _lib.FLAG_OSD0 if osd else 0
    a, b, mid = MC_BEGIN, MC_BEGIN + MC_T, MC_BEGIN + MC_SPLIT
    kw = dict(seed=MC_SEED, max_iter=MC_ITER, flags=flags)

    def run():
        cnt, spec, hist = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, a, b, **kw)
        assert cnt[0] == MC_T and hist.sum() == MC_T
        check_identities(cnt, spec, hist, MC_ITER, osd)
        # two calls ADD to the same tables
        c1, spec2, hist2 = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, a, mid, **kw)
        c2, spec2, hist2 = dec.mc_run_spectrum(code.Lx, code.distance, probs, prior, mid, b, spectrum=spec2,
                                               iter_hist=hist2, **kw)
        assert np.array_equal(c1 + c2, cnt) and np.array_equal(spec2, spec) and np.array_equal(hist2, hist)
        return cnt, spec, hist

    got = across_geometries(dec, code.Hx.shape[0], run)
    want = spectrum_counters(code.Hx, code.Lx, code.distance, P_EASY, prior, a, b, seed=MC_SEED, max_iter=MC_ITER,
                             osd=osd)
    for x, y in zip(got, want):
        assert np.array_equal(x, y), (x, y)
    assert got[1].sum() > 0


def shots_oracle(code, errors, prior, osd):
    """(counters, predictions, converged) of qbp_decode_shots from the oracle alone (include/qbp.h)."""
    H = np.asarray(code.Hx).astype(np.int64)
    syn = gu.syndromes_of(H, errors)
    hard, conv, iters, llr = oracle.decode_batch(H, syn, prior, MC_ITER, threads=8)
    x = hard.copy()
    cnt = np.zeros(_lib.NUM_COUNTERS, np.int64)
    fails = np.flatnonzero(~conv)
    if osd:
        for i in fails:
            x[i] = oracle.osd0(H, syn[i], llr[i], hard[i])
        cnt[10] = int((gu.syndromes_of(H, x[fails]) != syn[fails]).any(axis=1).sum()) if len(fails) else 0
    L = np.asarray(code.Lx, np.int64)
    pred = shots.masks_of((x.astype(np.int64) @ L.T) % 2)
    actual = shots.masks_of((errors.astype(np.int64) @ L.T) % 2)
    wrong = pred != actual
    cnt[0], cnt[6], cnt[7] = len(syn), len(fails), int(iters.sum())
    cnt[1], cnt[8] = int(wrong.sum()), int((wrong & ~conv).sum())
    return syn, actual, cnt, pred, conv


@gpu
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
@pytest.mark.parametrize("name", MC_CODES)
def test_decode_shots_across_geometries(name, osd):
    code, dec, prior, _ = mc_setup(name)
    flags = _lib.FLAG_OSD0 if osd else 0
    t = gu.torch()
    errors = oracle.mc_errors(code.n, P_EASY, 1, MC_SEED, MC_BEGIN, MC_T)
    syn, actual, o_cnt, o_pred, o_conv = shots_oracle(code, errors, prior, osd)
    det = shots.pack_bits(syn)
    rb = det.shape[1]
    det_t, prior_t = gu.to_device(det), gu.to_device(prior)
    act_t = gu.to_device(actual.view(np.int64))
    pred_t = t.empty(MC_T + gu.PAD, dtype=t.int64, device="cuda")
    conv_t = t.empty(MC_T + gu.PAD, dtype=t.uint8, device="cuda")
    mid = MC_SPLIT

    def call(lo, hi, cnt):
        dec.decode_shots_device(code.Lx, det_t.data_ptr() + lo * rb, act_t.data_ptr() + 8 * lo, hi - lo,
                                prior_t.data_ptr(), pred_t.data_ptr() + 8 * lo, conv_t.data_ptr() + lo, cnt.data_ptr(),
                                max_iter=MC_ITER, flags=flags, stream=gu.stream_ptr())

    def fetch(cnt):
        t.cuda.synchronize()
        assert bool((pred_t[MC_T:] == -1).all().item()) and bool((conv_t[MC_T:] == 0xFF).all().item())
        pred, conv = pred_t[:MC_T].cpu().numpy(), conv_t[:MC_T].cpu().numpy()
        assert (conv <= 1).all(), np.flatnonzero(conv > 1)[:8]
        assert (pred != -1).all(), np.flatnonzero(pred == -1)[:8]
        return cnt.cpu().numpy()[0], pred.view(np.uint64), conv.astype(bool)

    def run():
        pred_t.fill_(-1)
        conv_t.fill_(0xFF)
        cnt = counters_tensor()
        call(0, MC_T, cnt)
        whole = fetch(cnt)
        assert whole[0][0] == MC_T
        pred_t.fill_(-1)
        conv_t.fill_(0xFF)
        cnt = counters_tensor()
        call(0, mid, cnt)
        call(mid, MC_T, cnt)
        for x, y in zip(fetch(cnt), whole):
            assert np.array_equal(x, y)
        return whole

    got = across_geometries(dec, code.Hx.shape[0], run)
    assert np.array_equal(got[2], o_conv)
    assert np.array_equal(got[1], o_pred), np.flatnonzero(got[1] != o_pred)[:8]
    assert np.array_equal(got[0], o_cnt), (got[0], o_cnt)


# ---- C. general-H and streaming kernels ------------------------------------------------------------------------------------
def general_option_sets():
    for threads in (64, 192, 1024):
        for blocks in (1, 8):
            for mem in (0, 1, 2):
                yield dict(threads=threads, blocks=blocks, mem=mem)
    for mem in (0, 1):
        yield dict(mem=mem, no_r_split=1)
        yield dict(mem=mem, no_lds_tables=1)


def general_batch(name, rows, p):
    return cached(("general", name), lambda: Batch(name, p, rows, 3))


def run_general(name, batch, sizes):
    dec = decoder(name)
    num_cu = dec.info("num_cu")
    with gu.options(dec, kernel=_lib.KERNEL_GENERAL):
        for kw in (SP, DAMPED):
            ref = batch.reference(dec, **kw)                 # (automatic geometry of the general-H kernel, vs oracle)
            assert dec.info("last_kernel") == 2
            for opts in general_option_sets():
                for B in sizes:
                    what = f"general {name} {opts} B={B} variant={kw['variant']}"
                    with gu.options(dec, **opts):
                        got = batch.decode(dec, B, what, **kw)
                        grid, threads = dec.info("grid"), dec.info("threads")
                        assert dec.info("last_kernel") == 2
                    print(f"GENERAL {name} {opts} B={B} grid={grid} threads={threads} variant={kw['variant']}")
                    if "threads" in opts:
                        assert threads == opts["threads"], what
                        per_cu = 1 if opts["mem"] == 2 else opts["blocks"]
                        assert grid == min(B, num_cu * per_cu), (what, grid)
                    gu.assert_same(got, tuple(x[:B] for x in ref), what)


@gpu
@pytest.mark.parametrize("name,p", [("[[288, 12, 18]]", P_EASY), ("long_row", 0.03)])
def test_general_kernel_geometries(name, p):
    """Workgroup width x workgroups per CU x memory mode, and the two A/B switches on top of the global-memory mode
    and of auto; in-place (sum-product) and two-array (damped) message storage; a batch below the CU count (one wide
    workgroup per syndrome) and one above eight per CU (every workgroup fetches further syndromes dynamically)."""
    num_cu = decoder(name).info("num_cu")
    sizes = (num_cu - 1, 8 * num_cu + 37)
    run_general(name, general_batch(name, max(sizes), p), sizes)


@gpu
def test_general_kernel_geometries_space_time():
    """864 x 2592 (messages beyond the LDS in some modes): a few dozen syndromes."""
    H = matrix("st144x12")
    assert H.shape == (864, 2592)
    run_general("st144x12", general_batch("st144x12", 40, 0.01), (40,))


@gpu
@pytest.mark.parametrize("B", [255, 256, 257])
def test_streaming_kernel_block_boundary(B):
    """One lane per syndrome in blocks of 256 lanes: a batch that ends one short of, on and one past the boundary."""
    name = "long_row"
    dec = decoder(name)
    batch = general_batch(name, 8 * dec.info("num_cu") + 37, 0.03)
    with gu.options(dec, kernel=_lib.KERNEL_GENERAL):
        refs = {kw["variant"]: batch.reference(dec, **kw) for kw in (SP, DAMPED)}
    with gu.options(dec, kernel=_lib.KERNEL_STREAM):
        for kw in (SP, DAMPED):
            what = f"streaming {name} B={B} variant={kw['variant']}"
            got = batch.decode(dec, B, what, **kw)
            assert dec.info("last_kernel") == 3 and dec.info("grid") == -(-B // 256) and dec.info("threads") == 256
            gu.assert_same(got, tuple(x[:B] for x in refs[kw["variant"]]), what)


# ---- D. the device entry points as a caller uses them -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["[[72, 12, 6]]", "[[288, 12, 18]]"])
def test_three_launches_on_one_stream_without_sync(name):
    """What bench.py and every driver do: launches of one handle back to back on the caller's stream.  A large batch
    (the work counter is zeroed and used), a batch of grid * S (the memset is skipped: the counter still holds what
    the first launch left), a large batch again after QBP_OPT_SLOTS_PER_BLOCK changed.  One sync, then all three
    against the oracle."""
    t = gu.torch()
    dec = decoder(name)
    H = matrix(name)
    m, n = H.shape
    num_cu = dec.info("num_cu")
    rng = np.random.default_rng(77)
    prior = mc.prior_of(P_EASY, n)
    stream = t.cuda.Stream()
    S2 = gu.slot_values(m)[3]
    plan = ((0, 4 * num_cu * 2 * (1024 // m) + 29), (0, num_cu), (S2, 17 * num_cu * S2 + 5))
    syns = [gu.syndromes_of(H, rng.random((B, n)) < P_EASY) for _, B in plan]
    geoms = []
    with t.cuda.stream(stream):
        prior_t = gu.to_device(prior)
        syn_ts = [gu.to_device(s) for s in syns]
        outs = [gu.Outputs(B, n) for _, B in plan]
        try:
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
            for (S, B), syn_t, out in zip(plan, syn_ts, outs):
                dec.set_option(_lib.OPT_SLOTS_PER_BLOCK, S)
                gu.launch(dec, syn_t, prior_t, B, out)               # (poison and launch on `stream`; no sync)
                geoms.append((dec.info("grid"), dec.info("threads")))
        finally:
            dec.set_option(_lib.OPT_SLOTS_PER_BLOCK, 0)
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)
    stream.synchronize()
    print(f"STREAM {name} plan={plan} (grid, threads)={geoms}")
    assert geoms[0][0] == num_cu and geoms[1][0] == num_cu and geoms[1][1] == gu.threads_of(1, m)   # B = grid * S
    assert geoms[2] == (num_cu, gu.threads_of(S2, m))
    for i, ((S, B), syn, out) in enumerate(zip(plan, syns, outs)):
        got = out.fetch(B, 50, f"{name} launch {i} of three on one stream (S={S}, B={B})")
        o = oracle.decode_batch(H, syn, prior, 50, threads=8)
        gu.assert_same(got, (o[0], o[1], o[2], o[3]), f"{name} launch {i} of three on one stream vs oracle")


@gpu
@pytest.mark.parametrize("kernel", [_lib.KERNEL_ON_CHIP, _lib.KERNEL_GENERAL, _lib.KERNEL_STREAM],
                         ids=["on_chip", "general", "streaming"])
def test_null_outputs(kernel):
    """Each output null in turn, and all four: the others keep their values, the null one's buffer stays untouched."""
    name = "[[144, 12, 12]]"
    dec = decoder(name)
    batch = hard_batch(name)
    B = batch.rows
    ref = batch.reference(dec)
    with gu.options(dec, kernel=kernel):
        full = batch.decode(dec, B, f"kernel {kernel}")
        assert dec.info("last_kernel") == kernel
        for nulls in [(x,) for x in gu.NAMES] + [gu.NAMES]:
            got = batch.decode(dec, B, f"kernel {kernel} null {nulls}", nulls=nulls)
            assert [x is None for x in got] == [x in nulls for x in gu.NAMES]
            gu.assert_same(got, full, f"kernel {kernel} null {nulls}")
    gu.assert_same(full, ref, f"kernel {kernel} vs the default")


@gpu
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
def test_mc_run_device_adds_to_nonzero_counters(osd):
    code, dec, prior, _ = mc_setup("[[72, 12, 6]]")
    flags = _lib.FLAG_OSD0 if osd else 0
    start = 1000003
    cnt = counters_tensor(start=start)
    prior_t = gu.to_device(prior)
    dec.mc_run_device(code.Lx, code.distance, 0.05, prior_t.data_ptr(), 3, 3003, cnt.data_ptr(), draws=2, seed=8,
                      max_iter=30, flags=flags, stream=gu.stream_ptr())
    gu.torch().cuda.synchronize()
    want = dec.mc_run(code.Lx, code.distance, 0.05, prior, 3, 3003, draws=2, seed=8, max_iter=30, flags=flags)
    assert want[0] == 3000 and want[6] > 0
    assert np.array_equal(cnt.cpu().numpy()[0], want + start)


@gpu
def test_osd_device_entry_points_equal_the_host_wrappers():
    """qbp_osd0_batch_device and qbp_osd_batch_device on a caller's buffers and stream, against Decoder.osd0 /
    Decoder.osd on the same inputs (which tests/test_gpu_osd.py pins to the oracle)."""
    t = gu.torch()
    name = "[[144, 12, 12]]"
    dec = decoder(name)
    batch = hard_batch(name)
    hard, conv, iters, llr = batch.reference(dec)
    fails = np.flatnonzero(~conv)[:300]
    assert len(fails) >= 100
    syn, l, hd = batch.syn[fails], llr[fails], hard[fails]
    stream = t.cuda.Stream()
    with t.cuda.stream(stream):
        syn_t, l_t, hd_t = gu.to_device(syn), gu.to_device(l), gu.to_device(hd)
        sols = [t.full((len(fails) + gu.PAD, batch.n), 0xFF, dtype=t.uint8, device="cuda") for _ in range(3)]
        args = (syn_t.data_ptr(), l_t.data_ptr(), hd_t.data_ptr(), len(fails))
        dec.osd0_device(*args, sols[0].data_ptr(), stream=stream.cuda_stream)
        dec.osd_device(*args, sols[1].data_ptr(), method="cs", order=7, stream=stream.cuda_stream)
        dec.osd_device(*args, sols[2].data_ptr(), method="e", order=5, stream=stream.cuda_stream)
    stream.synchronize()
    want = (dec.osd0(syn, l, hd), dec.osd(syn, l, hd, "cs", 7), dec.osd(syn, l, hd, "e", 5))
    for sol, w in zip(sols, want):
        assert bool((sol[len(fails):] == 0xFF).all().item())
        got = sol[:len(fails)].cpu().numpy()
        assert (got <= 1).all()
        assert np.array_equal(got, w), np.flatnonzero((got != w).any(axis=1))[:8]
        assert np.array_equal(gu.syndromes_of(batch.H, got), syn)       # an OSD output satisfies the syndrome
