"""Randomised cross-check of the record kernels against their numpy statements: order-w OSD (one-wavefront and blocked),
Relay-BP, layered BP, BP guided decimation, LSD (each in its LDS and its large build), fixed-point min-sum (int8 and
int16), BP with a prior per record, and the Monte-Carlo second stages.  tests/fuzz_records_util.py draws the cases:
matrices on word, sort, thread-count and m = 256 boundaries with empty, light, weight-8 / 9 and long rows, isolated and
heavy columns, duplicated rows and columns; uniform, per-column and extreme priors; syndromes in and outside the column
space.  Every comparison is exact: np.array_equal, NaN equal to NaN, LLR bits through view(np.uint64).

The CPU tests (unmarked) run every statement on every case of the default seed and assert that the situations and the
outcome classes are present; the GPU tests compare, one function per kernel family.  ``QBP_FUZZ_CASES`` sets the case
count (60; a third of it for LSD, a quarter for the Monte-Carlo compositions), ``QBP_FUZZ_SEED`` the seed;
``QBP_FUZZ_CASES=2000 python -m pytest tests/test_gpu_fuzz_records.py -s`` is the long campaign
(profiles/r30_fuzz_records.txt holds one).

CPU statement time at the default count, seconds per GPU test function (measured once): osd_order 2.6, relay 2.8,
layered 1.6, gd 1.7, lsd 1.3, quant 4.9, cond 0.6 -- test_statement_cost_stays_small holds each under 30; the
statements inside the Monte-Carlo compositions run with their GPU test (15 cases of at most 130 x 300, 0.3 s with the
launches).  On the GPU the eight functions take 0.3 to 2.4 s each, statements included."""
import numpy as np
import pytest

import fuzz_records_util as fu
import lsd_oracle as lso
import osd_order_oracle as oo
from oracle import oracle
from qldpc_amd import _lib, bp, gd, mc, quant, relay

gpu = pytest.mark.gpu
BATCH_FAMILIES = fu.FAMILIES[:-1]
STATEMENT_SECONDS_LIMIT = 30.0


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


def assert_same(got, want, names, tag):
    """Exact equality of every output: values, NaN equal to NaN, float64 outputs also bit for bit."""
    for x, y, what in zip(got, want, names):
        if x is None:
            continue
        y = np.asarray(y)
        assert x.shape == y.shape, f"{what}: shape {x.shape} vs {y.shape}: {tag}"
        if not np.array_equal(x, y, equal_nan=True):
            rows = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1) if x.dtype.kind != "f" else
                                  ~((x == y) | (np.isnan(x) & np.isnan(y))).reshape(len(x), -1).all(axis=1))
            raise AssertionError(f"{what} differs from the statement on {len(rows)} records, first {rows[:8]}: {tag}")
        if x.dtype == np.float64:
            assert ((x.view(np.uint64) == y.astype(np.float64).view(np.uint64)) | np.isnan(y)).all(), f"{what} bits: {tag}"


def rows_of(want, rows):
    return tuple(np.asarray(x)[rows] for x in want)


# ---- CPU: reachability, outcome classes, statement cost ---------------------------------------------------------------------
def test_statements_run_and_inputs_cover_every_situation():
    """Every statement runs to completion on every drawn case; pooled over the families every situation of the
    generator occurs, and every family meets a work-item count below, on and above its thread count."""
    total = {}
    for family in fu.FAMILIES:
        for c in fu.cases(family):
            assert fu.fits(family, c.H), c.tag
            if family != "counters":
                fu.statement(c)
        seen = fu.situations(family)
        print(family, seen)
        for k in ("pass_below", "pass_exact", "pass_above"):
            assert seen[k] >= 1, (family, seen)
        for k in fu.INPUT_SITUATIONS:
            assert family not in ("osd_order", "lsd") or seen[k] >= 1, (family, seen)
        total = fu.pooled([total, seen])
    assert all(total[k] >= 1 for k in fu.SITUATIONS + fu.INPUT_SITUATIONS), total
    assert {c.par["stage"] for c in fu.cases("counters")} == set(fu.STAGES)


@pytest.mark.parametrize("family", BATCH_FAMILIES)
def test_statements_show_every_outcome_class(family):
    """Pooled over the cases, at least 8 records of every class the family's own test names."""
    pooled = fu.pooled(fu.classes(c) for c in fu.cases(family))
    print(family, pooled)
    assert all(v >= 8 for v in pooled.values()), (family, pooled)


def test_statement_cost_stays_small():
    seconds = {}
    for family in BATCH_FAMILIES:
        for c in fu.cases(family):
            fu.statement(c)
        seconds[family] = round(fu.SECONDS.get(family, 0.0), 1)
    print("statement seconds per family", seconds, "records", {f: sum(c.B for c in fu.cases(f)) for f in BATCH_FAMILIES})
    if fu.CASES <= 60:
        assert all(s < STATEMENT_SECONDS_LIMIT for s in seconds.values()), seconds


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def second_rows(c, dec=None):
    """The rows of the repeated call of every fifth case, or None."""
    if c.index % 5:
        return None
    return fu.second_batch(fu.SEED, c, dec.info("num_cu") if dec is not None else 0)


class Tally:
    def __init__(self, name):
        self.name, self.cases, self.records, self.builds, self.classes = name, 0, 0, {}, {}

    def add(self, c, **builds):
        self.cases += 1
        self.records += c.B
        for k, v in builds.items():
            self.builds[k] = self.builds.get(k, 0) + int(v)

    def done(self):
        assert all(v > 0 for v in self.builds.values()), (self.name, self.builds)
        print(f"fuzz {self.name}: {self.cases} cases, {self.records} records, cases per build {self.builds}, "
              f"classes {self.classes}")


@gpu
def test_fuzz_osd_order():
    t = Tally("osd_order")
    for c in fu.cases("osd_order"):
        want = fu.statement(c)
        method, w = c.par["method"], c.par["w"]
        dec = fresh(c.H)
        sol = dec.osd(c.syn, c.llr, c.hard, method=method, order=w)
        assert_same((sol,), (want["solution"],), ("solution",), c.tag)
        ok = want["consistent"]
        assert np.array_equal(sol[ok].astype(np.int64) @ c.H.T.astype(np.int64) % 2, c.syn[ok]), f"syndrome: {c.tag}"
        rows = second_rows(c)
        if rows is not None:
            again = dec.osd(c.syn[rows], c.llr[rows], c.hard[rows], method=method, order=w)
            assert_same((again,), (want["solution"][rows],), ("solution, second batch",), c.tag)
        blocked = c.index % 3 == 0
        if blocked:
            # QBP_FLAG_OSD_LARGE changes nothing where the one-wavefront kernel takes the matrix; QBP_OPT_OSD_BIG = 1 on
            # a handle of its own takes the matrix from that kernel, and osd_order_blocked_kernel serves the call
            assert np.array_equal(dec.osd(c.syn, c.llr, c.hard, method=method, order=w, large=True), sol), c.tag
            own = fresh(c.H)
            own.set_option(_lib.OPT_OSD_BIG, 1)
            big = own.osd(c.syn, c.llr, c.hard, method=method, order=w, large=True)
            assert_same((big,), (want["solution"],), ("solution of the blocked kernel",), c.tag)
            own.close()
        dec.close()
        t.add(c, **{"osd_order_kernel " + method: 1, "osd_order_blocked_kernel": blocked})
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


RELAY_NAMES = ("hard", "converged", "iters", "llr", "legs", "solutions")


@gpu
def test_fuzz_relay():
    t = Tally("relay")
    for c in fu.cases("relay"):
        r = fu.statement(c)
        want = tuple(r[k] for k in RELAY_NAMES)
        for large in (False, "force") if c.index % 3 == 0 else (False,):
            cfg = relay.RelayConfig(c.gammas, c.leg_iters, c.par["stop_after"], c.par["alpha"], large=large)
            dec = fresh(c.H)
            assert_same(dec.relay_decode(c.syn, c.prior, cfg), want, RELAY_NAMES, f"{c.tag} large={large}")
            rows = second_rows(c, dec)
            if rows is not None:
                got = dec.relay_decode(c.syn[rows], c.prior, want_llr=False)
                assert got[3] is None
                assert_same(got, rows_of(want, rows), RELAY_NAMES, f"{c.tag} large={large}, second batch")
            dec.close()
        t.add(c, bp_relay_kernel=1, bp_relay_kernel_LARGE=c.index % 3 == 0)
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


BP_NAMES = ("hard", "converged", "iters", "llr")


@gpu
def test_fuzz_layered():
    t = Tally("layered")
    for c in fu.cases("layered"):
        want = fu.statement(c)
        p = c.par
        flags = _lib.FLAG_LAYERED | (_lib.FLAG_FORCE_FULL if p["force_full"] else 0)
        kw = dict(max_iter=p["max_iter"], variant=p["variant"], alpha=p["alpha"], damping=1.0, clip_llr=20.0, flags=flags)
        for large in (False, True) if c.index % 3 == 0 else (False,):
            dec = fresh(c.H)
            dec.set_option(_lib.OPT_LAYERED_SLOTS, p["slots"])
            dec.set_option(_lib.OPT_LAYERED_MEM, 1 if large else 0)
            dec.layered_configure(fu.order_perm(c))
            assert_same(dec.decode(c.syn, c.prior, **kw), want, BP_NAMES, f"{c.tag} large={large}")
            assert dec.info("last_kernel") == 4
            rows = second_rows(c, dec)
            if rows is not None:
                dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
                got = dec.decode(c.syn[rows], c.prior, want_llr=False, **kw)
                assert_same(got, rows_of(want, rows), BP_NAMES, f"{c.tag} large={large}, second batch")
            dec.close()
        t.add(c, bp_layered_kernel=1, bp_layered_kernel_LARGE=c.index % 3 == 0)
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


GD_NAMES = ("hard", "converged", "iters", "llr", "rounds")


@gpu
def test_fuzz_gd():
    t = Tally("gd")
    for c in fu.cases("gd"):
        r = fu.statement(c)
        want = tuple(r[k] for k in GD_NAMES)
        p = c.par
        for large in (False, True) if c.index % 3 == 0 else (False,):
            cfg = gd.GDConfig(p["T"], p["max_rounds"], p["decim_llr"], p["variant"], p["alpha"], 20.0, large=large)
            dec = fresh(c.H)
            assert_same(dec.gd_decode(c.syn, c.prior, cfg), want, GD_NAMES, f"{c.tag} large={large}")
            rows = second_rows(c, dec)
            if rows is not None:
                dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
                got = dec.gd_decode(c.syn[rows], c.prior, want_llr=False)
                assert got[3] is None
                assert_same(got, rows_of(want, rows), GD_NAMES, f"{c.tag} large={large}, second batch")
            dec.close()
        t.add(c, bp_gd_kernel=1, bp_gd_kernel_LARGE=c.index % 3 == 0)
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


LSD_NAMES = ("solution", "stats")


@gpu
def test_fuzz_lsd():
    t = Tally("lsd")
    for c in fu.cases("lsd"):
        r = fu.statement(c)
        want = tuple(r[k] for k in LSD_NAMES)
        g = c.par["g"]
        for large in (False, "force") if c.index % 3 == 0 else (False,):
            dec = fresh(c.H)
            assert_same(dec.lsd(c.syn, c.llr, c.hard, g, large=large), want, LSD_NAMES, f"{c.tag} large={large}")
            rows = second_rows(c, dec)
            if rows is not None:
                dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
                got = dec.lsd(c.syn[rows], c.llr[rows], c.hard[rows], want_stats=False)
                assert got[1] is None
                assert_same(got, rows_of(want, rows), LSD_NAMES, f"{c.tag} large={large}, second batch")
                dec.set_option(_lib.OPT_BLOCKS_PER_CU, 0)
            if c.index % 4 == 0:
                # another step size on the configured handle, and the first one again
                head = slice(0, min(c.B, 3))
                r2 = lso.lsd_decode_batch(c.H, c.syn[head], c.llr[head], c.hard[head], c.par["g2"])
                got = dec.lsd(c.syn[head], c.llr[head], c.hard[head], c.par["g2"], large=large)
                assert_same(got, (r2["solution"], r2["stats"]), LSD_NAMES, f"{c.tag} large={large}, then g={c.par['g2']}")
                got = dec.lsd(c.syn[head], c.llr[head], c.hard[head], g, large=large)
                assert_same(got, rows_of(want, head), LSD_NAMES, f"{c.tag} large={large}, g again")
            dec.close()
        t.add(c, lsd_kernel=1, lsd_large_kernel=c.index % 3 == 0, two_step_sizes=c.index % 4 == 0)
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


QUANT_NAMES = ("hard", "converged", "iters", "posterior_q", "llr")


@gpu
def test_fuzz_quant():
    t = Tally("quant")
    for c in fu.cases("quant"):
        want = fu.statement(c)
        p = c.par
        dec = fresh(c.H)
        dec.set_option(_lib.OPT_QUANT_SLOTS, p["slots"])
        dec.quant_configure(quant.QuantConfig(p["bits"], p["scale"], p["alpha"], p["beta"]))
        assert_same(dec.quant_decode(c.syn, c.prior, p["max_iter"]), want, QUANT_NAMES, c.tag)
        assert dec.info("last_kernel") == 5
        rows = second_rows(c, dec)
        if rows is not None:
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
            got = dec.quant_decode(c.syn[rows], c.prior, p["max_iter"], want_posterior=False, want_llr=False)
            assert got[3] is None and got[4] is None
            assert_same(got, rows_of(want, rows), QUANT_NAMES, f"{c.tag}, second batch")
        dec.close()
        wide = p["bits"] > 8
        t.add(c, bp_quant_kernel_int8=not wide, bp_quant_kernel_int16=wide)
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


@gpu
def test_fuzz_cond():
    t = Tally("cond")
    for c in fu.cases("cond"):
        want = fu.statement(c)
        p = c.par
        args = (p["max_iter"], p["variant"], p["alpha"])
        dec = fresh(c.H)
        assert_same(dec.decode_cond(c.syn, c.sel, c.prior0, c.prior1, *args, 20.0), want, BP_NAMES, c.tag)
        if p["constant"]:
            prior = c.prior1 if int(c.sel[0, 0]) & 1 else c.prior0
            assert_same(dec.decode(c.syn, prior, *args, 1.0, 20.0), want, BP_NAMES, f"{c.tag}, qbp_decode_batch")
        rows = second_rows(c, dec)
        if rows is not None:
            dec.set_option(_lib.OPT_BLOCKS_PER_CU, 1)
            got = dec.decode_cond(c.syn[rows], c.sel[rows], c.prior0, c.prior1, *args, 20.0, want_llr=False)
            assert got[3] is None
            assert_same(got, rows_of(want, rows), BP_NAMES, f"{c.tag}, second batch")
        dec.close()
        t.add(c, **{("bp_cond_kernel sum-product", "", "bp_cond_kernel min-sum")[p["variant"]]: 1},
              constant_selector=p["constant"])
        t.classes = fu.pooled([t.classes, fu.classes(c)])
    t.done()


def osd_composition(dec, c, prior, w, variant, max_iter, alpha):
    """qbp_decode_batch (first stage), the order-w statement on its failures, oracle.classify_trials' rules."""
    H = c.H
    syn = (c.errors.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    hard, conv, iters, llr = dec.decode(syn, prior, max_iter, variant=variant, alpha=alpha)
    det = hard.copy()
    f = np.flatnonzero(~conv)
    if len(f):
        det[f] = oo.osd_order_batch(H, syn[f], llr[f], hard[f], w, "cs")
    cnt = oracle.classify_trials(H, c.Lx, c.distance, c.errors, syn, det, conv, iters)
    cnt[10] = int(((det[f].astype(np.int64) @ H.T.astype(np.int64) % 2) != syn[f]).any(1).sum())
    return cnt


@gpu
def test_fuzz_second_stage_counters():
    """qbp_mc_run_errors under every second-stage flag set against the compositions the families' own tests state:
    first-stage decode, the statement on its failures, oracle.classify_trials."""
    import test_gpu_gd as tg
    import test_gpu_layered as tlay
    import test_gpu_lsd as tl
    import test_gpu_quant as tq
    import test_gpu_relay as tr
    t = Tally("second-stage counters")
    for c in fu.cases("counters"):
        H, L, d, errors, p = c.H, c.Lx, c.distance, c.errors, c.par
        n, stage, variant = c.n, p["stage"], p["variant"]
        prior = mc.prior_of(c.p, n)
        dec = fresh(H)
        if stage == "relay":
            cfg = relay.RelayConfig(relay.relay_gammas(n, 3, 0.125, (-0.24, 0.66), c.seed), [6, 9, 5], 2, 0.9)
            dec.relay_configure(cfg)
            want, _ = tr.compose(dec, H, L, d, errors, prior, cfg, variant)
            kw = dict(max_iter=tr.MC_ITERS, variant=variant, alpha=tr.ALPHA, flags=_lib.FLAG_RELAY)
        elif stage == "gd":
            cfg = gd.GDConfig(4, 6, 25.0, _lib.MIN_SUM if variant == _lib.SUM_PRODUCT else _lib.SUM_PRODUCT, 0.9, 20.0)
            dec.gd_configure(cfg)
            want, _ = tg.compose(dec, H, L, d, errors, prior, cfg, variant, False)
            kw = dict(max_iter=tg.MC_ITERS, variant=variant, alpha=tg.ALPHA, flags=_lib.FLAG_GD)
        elif stage == "lsd":
            dec.lsd_configure(p["g"])
            want, _ = tl.compose(dec, H, L, d, errors, prior, p["g"], variant, False)
            kw = dict(max_iter=tl.MC_ITERS, variant=variant, alpha=tl.ALPHA, flags=_lib.FLAG_LSD)
        elif stage == "osd_cs":
            want = osd_composition(dec, c, prior, p["w"], variant, 8, 0.9)
            kw = dict(max_iter=8, variant=variant, alpha=0.9, flags=_lib.FLAG_OSD0 | _lib.osd_flags("cs", p["w"]))
        elif stage == "layered":
            alpha = 1.0 if variant == _lib.SUM_PRODUCT else 0.8
            dec.layered_configure(None)
            want, _ = tlay.expected_counters(H, L, d, errors, prior, variant, alpha)
            kw = dict(max_iter=tlay.MC_ITERS, variant=variant, alpha=alpha, flags=_lib.FLAG_LAYERED)
        else:
            params = tq.MC_PARAMS if c.index % 2 else tq.MC_PARAMS_WIDE
            _, (syn, hard, conv, iters, llr) = tq.expected(H, L, d, errors, prior, params)
            f = np.flatnonzero(~conv)
            r = lso.lsd_decode_batch(H, syn[f], llr[f], hard[f], p["g"])
            det = hard.copy()
            det[f] = r["solution"]
            want = oracle.classify_trials(H, L, d, errors, syn, det, conv, iters)
            want[10] = int((r["stats"][:, 3] == 0).sum())
            dec.quant_configure(tq.cfg_of(params))
            dec.lsd_configure(p["g"])
            kw = dict(max_iter=tq.MC_ITERS, variant=_lib.MIN_SUM, flags=_lib.FLAG_QUANT | _lib.FLAG_LSD)
        got = dec.mc_run_errors(L, d, errors, prior, **kw)
        assert got[0] == c.B and np.array_equal(got, want), f"{c.tag}: {got.tolist()} vs {np.asarray(want).tolist()}"
        rows = second_rows(c)
        if rows is not None and c.B >= 2:                                 # the record buffers reused: a split of the list
            cut = max(1, c.B // 3)
            parts = dec.mc_run_errors(L, d, errors[:cut], prior, **kw) + dec.mc_run_errors(L, d, errors[cut:], prior, **kw)
            assert np.array_equal(parts, want), f"{c.tag}, split at {cut}"
        dec.close()
        t.add(c, **{stage: 1})
        t.classes["second_stage_records"] = t.classes.get("second_stage_records", 0) + int(got[6])
    assert set(t.builds) == set(fu.STAGES)
    t.done()
