"""GPU: the two-stage CSS decoder (qbp_css_*) where its two sectors differ, against tests/css_oracle.py.

tests/test_gpu_css.py runs the chain on codes whose Hx and Hz have one shape and one k, with priors that are constant
over the qubits and prior_b1 == 0, and on at most 2000 trials: exchanging the sectors' row counts, logical operators
or syndrome buffers, dropping the conditional prior's sign, or breaking the stride of a glue kernel's loop changes
nothing it sees.  Here:

* the code is the hypergraph product of the 3 x 7 Steane matrix with a 4 x 5 chain, in both orders (css_oracle.hgp):
  "wide_a" has Hx 15 x 47 and Hz 28 x 47, "wide_b" the reverse; n = 47 is no multiple of 4 or 64, neither m of 32; k = 4;
* the priors are per qubit and biased (css_oracle.biased_priors): three different vectors, prior_b1 of both signs;
* the trials go past one pass of the grid-stride loops of css_classify_kernel, css_select_kernel,
  css_sample_pauli_kernel and window_syndrome_kernel (window_fail_list_kernel strides from 524289 records of ONE
  chunk on: the statement would take minutes, and the test stays below it);
* the logical operators of a sector go to bits 32 .. 63 of its mask while the other sector keeps four rows, k = 0 in
  one sector, and a sequence on one handle in which consecutive calls differ in one row of one sector.

Every comparison is exact.  tests/test_css_cpu.py shows on the statement alone that these inputs tell the sectors and
the orientations apart and leave at least five trials to either outcome of BP in both sectors."""
import numpy as np
import pytest

import css_oracle as co
import logical_mask_util as lm
from qldpc_amd import _lib, bp

pytestmark = pytest.mark.gpu

T, B, MAX_ITER = co.ASYM_T, co.ASYM_B, co.ASYM_MAX_ITER
TAGS = ("wide_a", "wide_b")
GRID_LANES = 2048 * 256              # CSS_MAX_GRID * CSS_THREADS of qbp_cond.hpp: the lanes of one pass (window_grid: same)
GRID_WAVES = 2048 * (256 // 64)      # ... and its wavefronts: css_classify_kernel takes one trial per wavefront
POISON = 0xA5


def flags_of(osd):
    return 0 if osd is None else _lib.osd_flags("cs", 0) if osd == 0 else _lib.osd_flags(osd[0], osd[1])


def kw_of(mode):
    m = co.ASYM_MODES[mode]
    return dict(max_iter=MAX_ITER, variant=m.get("variant", _lib.SUM_PRODUCT), alpha=m.get("alpha", 1.0), damping=1.0,
                clip_llr=20.0, flags=flags_of(m["osd"]))


def fresh(s):
    return _lib.CssDecoder(_lib.Decoder(*bp.csr_from_H(s["Hx"]), bp.DEVICE), _lib.Decoder(*bp.csr_from_H(s["Hz"]), bp.DEVICE))


_DEC = {}


def decoder(tag):
    if tag not in _DEC:
        _DEC[tag] = fresh(co.asym_inputs(tag))
    return _DEC[tag]


def test_the_inputs_are_what_the_module_says():
    assert _lib.MIN_SUM == co.MIN_SUM
    for tag in TAGS:
        s = co.asym_inputs(tag)
        dec = decoder(tag)
        assert (dec.n, dec.ma, dec.mb) == ((47, 15, 28) if tag == "wide_a" else (47, 28, 15))
        assert s["Lx"].shape == s["Lz"].shape == (4, 47)
        pa, b0, b1 = s["priors"]
        assert (b1 < 0).any() and (b1 > 0).any()
        assert not np.array_equal(pa, b0) and not np.array_equal(pa, b1) and not np.array_equal(b0, b1)


# ---- a. the Monte-Carlo counters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(co.ASYM_MODES))
@pytest.mark.parametrize("tag", TAGS)
def test_mc_run_errors_equals_the_statement(tag, mode):
    s = co.asym_inputs(tag)
    want = co.asym_statement(tag, mode)
    assert all(5 <= want[r][6] <= T - 5 for r in (0, 1)), want
    got = decoder(tag).mc_run_errors(s["Lx"], s["Lz"], s["d"], s["ea"], s["eb"], *s["priors"], **kw_of(mode))
    print(tag, mode, got.tolist())
    assert np.array_equal(got, want), (got, want)


# ---- b. the decode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "osd0", "cs7"])
@pytest.mark.parametrize("tag", TAGS)
def test_decode_batch_equals_the_statement_and_the_composition(tag, mode):
    """qbp_css_decode_batch stages B * ma and B * mb syndrome bytes, and with OSD runs the redo pass of a caller's
    syndromes in both sectors.  Against css_oracle.decode in all three modes -- both matrices have full row rank, so every
    syndrome lies in the column space and order-w OSD is stated by tests/osd_order_oracle.py -- and against the ordinary
    calls composed by hand."""
    s = co.asym_inputs(tag)
    dec, osd = decoder(tag), co.ASYM_MODES[mode]["osd"]
    assert co.gf2_rank(s["Hx"]) == s["Hx"].shape[0] and co.gf2_rank(s["Hz"]) == s["Hz"].shape[0]
    syn_a, syn_b = co.asym_batch_syndromes(s)
    pa, b0, b1 = s["priors"]
    xa, xb, ca, cb = dec.decode(syn_a, syn_b, pa, b0, b1, MAX_ITER, flags=flags_of(osd))
    assert 5 <= (~ca).sum() <= B - 5 and 5 <= (~cb).sum() <= B - 5, ((~ca).sum(), (~cb).sum())

    want = co.decode(s["Hx"], s["Hz"], syn_a, syn_b, pa, b0, b1, max_iter=MAX_ITER, osd=osd)
    for name, x, y in zip(("x_a", "x_b", "conv_a", "conv_b"), (xa, xb, ca, cb), want):
        assert np.array_equal(x, y), (name, np.flatnonzero((x != y).reshape(B, -1).any(axis=1)))

    def stage(d, syn, out):
        hard, conv, _, llr = out
        x = hard.copy()
        bad = np.flatnonzero(~conv)
        if osd is not None and bad.size:
            x[bad] = d.osd0(syn[bad], llr[bad], hard[bad]) if osd == 0 else d.osd(syn[bad], llr[bad], hard[bad], *osd)
        return x, conv
    want_a, conv_a = stage(dec.a, syn_a, dec.a.decode(syn_a, pa, MAX_ITER))
    want_b, conv_b = stage(dec.b, syn_b, dec.b.decode_cond(syn_b, want_a, b0, b1, MAX_ITER))
    assert np.array_equal(xa, want_a) and np.array_equal(ca, conv_a)
    assert np.array_equal(xb, want_b) and np.array_equal(cb, conv_b)
    if osd is not None:         # the redo pass: every correction meets its (perturbed) syndrome
        assert np.array_equal(co._syn(s["Hx"], xa), syn_a) and np.array_equal(co._syn(s["Hz"], xb), syn_b)


# ---- c. beyond one pass of the grid ----------------------------------------------------------------------------------------
def test_mc_beyond_one_grid_pass():
    """19000 trials of "wide_a" in ONE chunk (the default holds 2^20), OSD-0: css_classify_kernel makes a third trip
    (one trial per wavefront, 8192 per pass), css_select_kernel and window_syndrome_kernel on the 28-row sector a
    second (T n = 893000 and T mb = 532000 lanes against 524288 per pass); the 15-row sector's syndromes stay within
    one pass.  qbp_css_mc_run draws the same errors on the device (css_sample_pauli_kernel: 228000 lanes, one pass;
    its stride is the next test's); five chunks of 4099 trials must count the same."""
    s = co.asym_inputs("wide_a")
    dec = decoder("wide_a")
    n, big = s["n"], 19000
    assert big > GRID_WAVES and big * n > GRID_LANES                  # classify, select
    assert big * dec.mb > GRID_LANES >= big * dec.ma                  # the syndromes of sector B stride, sector A's do not
    assert big <= _lib.MC_OSD_MAX_TRIALS and big <= (1 << 28) // n    # one chunk
    assert big <= GRID_LANES                                          # (window_fail_list_kernel: one pass)
    begin = co.ASYM_BEGIN
    ea, eb = co.sample_pauli(n, *co.BIASED_RATES, co.ASYM_SEED, begin, big)
    kw = dict(co.ASYM_MODES["osd0"], max_iter=MAX_ITER)
    decoded = co.decode(s["Hx"], s["Hz"], co._syn(s["Hx"], ea), co._syn(s["Hz"], eb), *s["priors"], **kw)
    code = (s["Hx"], s["Hz"], s["Lx"], s["Lz"], s["d"])
    want = co.classify(*code, ea, eb, decoded)
    assert all(5 <= want[r][6] <= big - 5 for r in (0, 1)) and want[2][0] == big, want
    # the trials beyond the first pass are not all of one kind: dropping them would change these counters
    head = co.classify(*code, ea[:GRID_WAVES], eb[:GRID_WAVES], tuple(x[:GRID_WAVES] for x in decoded))
    assert all((want - head)[r][i] >= 5 for r in (0, 1) for i in (1, 5, 6, 9)), (want, head)

    run_kw = kw_of("osd0")
    stored = lambda: dec.mc_run_errors(s["Lx"], s["Lz"], s["d"], ea, eb, *s["priors"], **run_kw)
    drawn = lambda: dec.mc_run(s["Lx"], s["Lz"], s["d"], *co.BIASED_RATES, *s["priors"], begin, begin + big,
                               seed=co.ASYM_SEED, **run_kw)
    got = stored()
    print("one chunk", got.tolist())
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(drawn(), want)
    try:
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 4099)
        assert 4 * 4099 < big <= 5 * 4099
        assert np.array_equal(stored(), want)
        assert np.array_equal(drawn(), want)
    finally:
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)
    assert np.array_equal(stored(), want)


def test_sampler_beyond_one_grid_pass():
    """44000 trials of n = 47: 12 lanes per trial (four qubits each), 528000 lanes against 524288 per pass, the trial
    indices across 2^32, into poisoned arrays a few rows longer than T."""
    s = co.asym_inputs("wide_a")
    dec = decoder("wide_a")
    n, big, pad = s["n"], 44000, 3
    n4 = (n + 3) // 4
    assert n4 == 12 and big * n4 > GRID_LANES
    begin = (1 << 32) - 30000
    assert begin < (1 << 32) < begin + big
    seed = co.ASYM_SEED
    want = co.sample_pauli(n, *co.BIASED_RATES, seed, begin, big)
    got = [np.full((big + pad, n), POISON, np.uint8) for _ in range(2)]
    rc = _lib.load().qbp_css_sample_errors(dec._h, *co.BIASED_RATES, seed, begin, big, got[0].ctypes.data, got[1].ctypes.data)
    assert rc == 0, _lib.load().qbp_last_error()
    # the lanes of the second trip: the last four of trial 43690 and all of the trials behind it
    second = GRID_LANES // n4
    assert second == 43690 and GRID_LANES - second * n4 == 8 and second + 1 < big
    for g, w, name in zip(got, want, "ab"):
        assert (g[big:] == POISON).all(), name                       # nothing behind the last trial
        assert (g[:big] <= 1).all(), (name, np.flatnonzero((g[:big] > 1).any(axis=1))[:8])      # every byte written
        assert np.array_equal(g[:big], w), (name, np.flatnonzero((g[:big] != w).any(axis=1))[:8])
        # (said again for the places a broken stride would leave out)
        assert np.array_equal(g[second], w[second]) and np.array_equal(g[second + 1], w[second + 1])
        assert g[big - 1, n - 1] == w[big - 1, n - 1] and g[big - 1, n - 1] <= 1
        assert w[second:].any() and w[:, n - 1].any()                # ... which are not all zero
    assert np.array_equal(got[0][2 ** 32 - begin], want[0][2 ** 32 - begin])   # trial 2^32 itself


# ---- d. the logical operators, sector by sector --------------------------------------------------------------------------
def test_logical_masks_per_sector():
    """css_sector folds a sector's lm in 64 bits with its own shuffle ladder, and McInputs::prepare_lx caches each
    sector's upload: one handle, OSD-0, the placements of tests/logical_mask_util.py in one sector while the other
    keeps its four rows (or another placement).  Every run equals the run with the rows the placements keep, and the
    statement with the same L'."""
    tag = "wide_a"
    s = co.asym_inputs(tag)
    dec = fresh(s)
    Lx, Lz, n = s["Lx"], s["Lz"], s["n"]
    kw = kw_of("osd0")
    run = lambda La, Lb: dec.mc_run_errors(La, Lb, s["d"], s["ea"], s["eb"], *s["priors"], **kw)
    want = lambda La, Lb: co.asym_statement(tag, "osd0", La, Lb)
    PX = {name: (Lp, m) for name, Lp, m in lm.placements(Lx)}
    PZ = {name: (Lp, m) for name, Lp, m in lm.placements(Lz)}
    none = np.zeros((0, n), np.uint8)
    L_ONLY, L_FREE = list(lm.L_ONLY), list(lm.L_FREE)

    base = run(Lx, Lz)
    assert np.array_equal(base, want(Lx, Lz)), (base, want(Lx, Lz))
    assert base[0][1] >= 8 and base[1][1] >= 8 and base[0][1] != base[1][1], base
    # the runs the placements must equal: k = 1, bit 0, in one sector
    one_a = {r: run(np.ascontiguousarray(Lx[r:r + 1]), Lz) for r in lm.SINGLE_ROWS}
    one_b = {r: run(Lx, np.ascontiguousarray(Lz[r:r + 1])) for r in lm.SINGLE_ROWS}
    for one in (one_a, one_b):       # the two rows, and all four, classify differently: a stale or lost row shows
        assert not np.array_equal(one[0], one[1]) and not np.array_equal(one[0], base) and not np.array_equal(one[1], base)

    # ka = 64 beside kb = 4 and the reverse; then k = 33 beside k = 64, both ways
    for what, La, Lb, ref in [
            ("top, Lz", PX["top"][0], Lz, base), ("Lx, top", Lx, PZ["top"][0], base),
            ("k33, straddle", PX["k33"][0], PZ["straddle"][0], one_a[0]),
            ("straddle, k33", PX["straddle"][0], PZ["k33"][0], one_b[0]),
            ("spread, top", PX["spread"][0], PZ["top"][0], base)]:
        got = run(La, Lb)
        assert np.array_equal(got, ref), (what, got, ref)
        assert np.array_equal(got, want(La, Lb)), (what, got)
    assert np.array_equal(one_a[0], run(lm.kept(Lx, PX["k33"][1]), lm.kept(Lz, PZ["straddle"][1])))

    # one row changes between consecutive calls, k = 64 in that sector throughout: sector A, then sector B
    for sector, L, one in (("a", Lx, one_a), ("b", Lz, one_b)):
        for r, b in [(0, 63), (1, 63), (1, 31), (0, 31), (0, 32), (1, 32)]:
            name, Lp, m = lm.single(L, r, b)
            got = run(Lp, Lz) if sector == "a" else run(Lx, Lp)
            assert np.array_equal(got, one[r]), (sector, name, got, one[r])
            ref = want(Lp, Lz) if sector == "a" else want(Lx, Lp)
            assert np.array_equal(got, ref), (sector, name, got, ref)
            assert np.array_equal(lm.kept(L, m), L[r:r + 1])

    # k = 0 in one sector, between calls with k = 64 there
    for what, La, Lb, row, other in (("ka = 0", none, Lz, 0, 1), ("kb = 0", Lx, none, 1, 0)):
        got = run(La, Lb)
        assert not got[row][L_ONLY].any(), (what, got)
        assert np.array_equal(got[row][L_FREE], base[row][L_FREE]) and np.array_equal(got[other], base[other]), (what, got)
        assert got[2][1] == got[other][1] and got[2][1] == base[other][1], (what, got)
        assert np.array_equal(got, want(La, Lb)), (what, got)
    assert np.array_equal(run(PX["top"][0], PZ["top"][0]), base)

    # the inputs are sensitive: a fold that lost bits 32 .. 63 of lm would classify with low_half(L'), and the
    # statement with it differs from the true one in both sectors
    lost_a, lost_b = want(lm.low_half(PX["top"][0]), Lz), want(Lx, lm.low_half(PZ["top"][0]))
    assert not np.array_equal(lost_a[0], base[0]) and np.array_equal(lost_a[1], base[1])
    assert not np.array_equal(lost_b[1], base[1]) and np.array_equal(lost_b[0], base[0])
    assert not np.array_equal(want(lm.low_half(PX["k33"][0]), lm.low_half(PZ["straddle"][0])), one_a[0])


def test_k_out_of_range_is_refused():
    """k = 65 or -1 in either sector: QBP_E_INVALID before anything is written, qbp_css_mc_run_errors' SET included."""
    s = co.asym_inputs("wide_a")
    dec = decoder("wide_a")
    lib = _lib.load()
    n = s["n"]
    L65 = np.ones((65, n), np.uint8)
    Lx, Lz = np.ascontiguousarray(s["Lx"]), np.ascontiguousarray(s["Lz"])
    ea, eb = np.ascontiguousarray(s["ea"][:8]), np.ascontiguousarray(s["eb"][:8])
    pri = [np.ascontiguousarray(p, np.float64) for p in s["priors"]]
    tail = (*(p.ctypes.data for p in pri), MAX_ITER, _lib.SUM_PRODUCT, 1.0, 1.0, 20.0, int(_lib.FLAG_OSD0))
    for ka, kb in [(65, 4), (4, 65), (-1, 4), (4, -1)]:
        La, Lb = (L65 if ka != 4 else Lx), (L65 if kb != 4 else Lz)
        cnt = np.full((3, _lib.NUM_COUNTERS), -7777, np.int64)
        rc = lib.qbp_css_mc_run_errors(dec._h, La.ctypes.data, ka, Lb.ctypes.data, kb, s["d"], ea.ctypes.data, eb.ctypes.data, 8,
                                       *tail, cnt.ctypes.data)
        assert rc == _lib.E_INVALID and b"logical operators" in lib.qbp_last_error(), (ka, kb, lib.qbp_last_error())
        assert (cnt == -7777).all(), (ka, kb)
        rc = lib.qbp_css_mc_run(dec._h, La.ctypes.data, ka, Lb.ctypes.data, kb, s["d"], *co.BIASED_RATES, co.ASYM_SEED, 0, 8,
                                *tail, cnt.ctypes.data)
        assert rc == _lib.E_INVALID and (cnt == -7777).all(), (ka, kb)
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run_errors(L65, Lz, s["d"], ea, eb, *pri, max_iter=MAX_ITER)
    assert e.value.code == _lib.E_INVALID
    # the handle is as it was
    got = dec.mc_run_errors(Lx, Lz, s["d"], s["ea"], s["eb"], *pri, **kw_of("osd0"))
    assert np.array_equal(got, co.asym_statement("wide_a", "osd0"))


# ---- e. the BP kernel of one sector alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "osd0"])
@pytest.mark.parametrize("tag", TAGS)
def test_general_kernel_in_sector_a_alone(tag, mode):
    """QBP_OPT_FORCE_GENERIC on sector A's handle: stage A runs the general-H kernel, stage B what it ran before, and
    the counters stay those of the statement (which the automatic choice gives too: test (a))."""
    s = co.asym_inputs(tag)
    dec = decoder(tag)
    run = lambda: dec.mc_run_errors(s["Lx"], s["Lz"], s["d"], s["ea"], s["eb"], *s["priors"], **kw_of(mode))
    want = co.asym_statement(tag, mode)
    auto = run()
    assert dec.a.info("last_kernel") == 1          # both matrices fit the on-chip kernel
    try:
        dec.a.set_option(_lib.OPT_FORCE_GENERIC, 1)
        forced = run()
        assert dec.a.info("last_kernel") == 2
    finally:
        dec.a.set_option(_lib.OPT_FORCE_GENERIC, 0)
    assert np.array_equal(forced, auto) and np.array_equal(forced, want), (forced, auto, want)
    assert np.array_equal(run(), want) and dec.a.info("last_kernel") == 1
