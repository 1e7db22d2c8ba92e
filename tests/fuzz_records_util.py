"""Case generator of tests/test_gpu_fuzz_records.py (pure numpy, usable without a GPU): random matrices aimed at the
record kernels -- order-w OSD, Relay-BP, layered BP, BP guided decimation, LSD, fixed-point min-sum and BP with a prior
per record --, their priors, syndromes and second-stage inputs, the parameters of every family, and the numpy
statements' outputs on them, computed once per (family, count, seed) and shared by the CPU and the GPU tests.

The shape kinds of tests/test_gpu_fuzz.py (``random_matrix``) are kept and extended by kinds that put m, n and the
work-item counts on the boundaries the kernels' loops, bit-packed words, ballots and LDS carve-ups turn on.  Before a
matrix is handed to a family, ``fits`` asks the library's limits as tests/record_kernel_util.py, tests/lsd_util.py,
``quant.lds_bytes`` and the headers state them; only shapes the LDS builds accept are drawn, and the large builds are
forced by option on the same shapes."""
import os
import time

import numpy as np

import css_oracle as co
import gd_oracle as go
import layered_oracle as lo
import lsd_oracle as lso
import lsd_util as lu
import osd_order_oracle as oo
import quant_oracle as qo
import record_kernel_util as ru
import relay_oracle as ro
from oracle import oracle
from qldpc_amd import quant, relay
from test_gpu_fuzz import capped_matrix, random_matrix

CASES = int(os.environ.get("QBP_FUZZ_CASES", "60"))
SEED = int(os.environ.get("QBP_FUZZ_SEED", "20261021"))
FAMILIES = ("osd_order", "relay", "layered", "gd", "lsd", "quant", "cond", "counters")
BATCHES = (1, 3, 17, 64, 150)
SUM_PRODUCT, MIN_SUM = 0, 2
# the thread count of the family's workgroup where it is fixed, or its upper limit (ru.gd_threads, ru.relay_threads):
# the "passes" kind puts a work-item count one below, on and one above it
THREADS = dict(osd_order=256, relay=ru.RELAY_MAX_THREADS, layered=ru.LAYERED_THREADS, gd=ru.GD_MAX_THREADS, lsd=256,
               quant=256, cond=512, counters=256)
SITUATIONS = ("word_m", "word_n", "pow2_n", "pow2_n_plus_1", "pass_below", "pass_exact", "pass_above", "m_at_256",
              "row_0", "row_1", "row_8", "row_9", "row_long", "col_0", "col_heavy", "dup_cols", "dup_rows",
              "prior_uniform", "prior_per_column", "prior_extreme", "syn_outside")
INPUT_SITUATIONS = ("llr_ties", "llr_nan", "llr_bp")              # order-w OSD and LSD
EXTREMES = (0.0, np.inf, -np.inf, -1.5, 700.0)
# qbp_relay_decode_batch, qbp_gd_decode_batch and QBP_FLAG_LAYERED refuse a prior that is not finite (check_prior with
# must_be_finite in qbp.hip); the other entries refuse NaN only
FINITE_ONLY = ("relay", "layered", "gd", "counters")


# ---- the library's limits, restated ------------------------------------------------------------------------------------
def osd_order_lds_bytes(m, n):
    """osd_order_lds of qbp_osd_order.hpp on osd_region0_bytes of qbp_osd_parts.hpp (W = ceil(n / 32), NP = the power
    of two >= n)."""
    W, NP = -(-n // 32), 1
    while NP < n:
        NP <<= 1
    region0 = (max(8 * NP, 4 * m * (W + 1)) + 7) & ~7
    pivcol = region0 + ((2 * NP + 3) & ~3)
    absl = (pivcol + 4 * m + 7) & ~7
    return absl + 8 * n + 8 * m + 4 * n + 2 * n + n + 16


def osd_blocked_ok(m, n):
    """osd_blocked_plan of qbp.hip: what QBP_FLAG_OSD_LARGE needs once QBP_OPT_OSD_BIG = 1 has taken the matrix from
    the one-wavefront kernel."""
    NP = 1
    while NP < n:
        NP <<= 1
    wc = (n + 63) // 64 + 1
    table = min(96 * 1024, 256 * wc * 8)
    lds = max(table, 8 * NP) + 64 * wc + 4 * NP + ((n + 15) & ~15) + 4 * m
    if lds > 160 * 1024 - 64:
        lds = table + 64 * wc + 4 * m
    return m <= 8192 and lds <= 160 * 1024 - 64 and 16 * wc <= table


def fits(family, H):
    """The LDS build of `family` takes H (and, for order-w OSD, both of its kernels do)."""
    sh = ru.Shape(H)
    m, n, E = sh.m, sh.n, sh.E
    if m < 1 or n < 1 or n > lu.MAX_COLS:
        return False
    osd = osd_order_lds_bytes(m, n) <= 64 * 1024 and m <= lu.MAX_ROWS and osd_blocked_ok(m, n)
    lsd = lu.lsd_lds_bytes(m, n) <= lu.LDS_LIMIT and m <= lu.MAX_ROWS
    rly = ru.relay_lds_bytes(m, n, E, records=True) <= ru.LDS_LIMIT
    lay = ru.layered_lds_bytes(m, n, E, 1, True) <= ru.LDS_LIMIT
    gdd = ru.gd_lds_bytes(m, n, E, True) <= ru.LDS_LIMIT
    qnt = quant.lds_bytes(m, n, E, 1, True) <= ru.LDS_LIMIT and sh.col_w.max(initial=0) <= 32767
    # cond_lds_bytes of qbp_cond.hpp: BPGD's rows and tables plus a byte per edge and a few head words
    cnd = ru.gd_lds_bytes(m, n, E, True) + E + 256 <= ru.LDS_LIMIT
    return dict(osd_order=osd, relay=rly, layered=lay, gd=gdd, lsd=lsd, quant=qnt, cond=cnd,
                counters=osd and lsd and rly and lay and gdd and qnt)[family]


# ---- matrices ---------------------------------------------------------------------------------------------------------
def _sparse(rng, m, n):
    return capped_matrix(rng, m, n, 8, 4, rng.uniform(0.5, 1.0)) if rng.random() < 0.7 else \
        capped_matrix(rng, m, n, 6, 3, rng.uniform(0.5, 1.0))


def _one_class_columns(rng, m, n, w):
    """n columns of weight exactly w on m >= w rows: one column class, so Shape.var_items = pad64(n)."""
    H = np.zeros((m, n), np.int64)
    for v in range(n):
        H[rng.choice(m, w, replace=False), v] = 1
    return H


def _passes(rng, family, notes, delta, max_m):
    """A work-item count on the thread count T of the family, one below or one above: the last pass of the strided
    loop over the items is full, short by one item, or has one item alone."""
    T = THREADS[family]
    # delta = -1, 0, 1: T - 1, T, T + 1 items
    notes.add(("pass_below", "pass_exact", "pass_above")[delta + 1])
    count = T + delta
    if count <= max_m and rng.random() < 0.5:
        # checks: `count` rows of weight 3 (one row class: check_items = pad64(count))
        n = int(rng.integers(count // 2, count + 40))
        H = _one_class_columns(rng, n, count, 3).T.copy()
        assert ru.Shape(H).check_items == ru.pad64(count)
        return H
    # variables: `count` columns of weight 2 (one column class: var_items = pad64(count)) on count / 3 rows or so
    m = min(int(rng.integers(max(3, count // 4), max(4, count // 3))), max_m)
    H = _one_class_columns(rng, m, count, 2)
    assert ru.Shape(H).var_items == ru.pad64(count)
    return H


def _decorate(rng, H, notes):
    """Rows, columns and duplicates written over a matrix in place (its shape stays)."""
    m, n = H.shape
    if m >= 6 and n >= 12 and rng.random() < 0.4:
        rows = rng.choice(m, 5, replace=False)
        long_w = int(rng.integers(20, 41))               # one long row: weight 20 .. 40
        # weight 0, 1, exactly 8 and 9: check_row's one-pass form ends at 8, the two-pass loop starts at 9
        for r, w in zip(rows, (0, 1, 8, 9, long_w)):
            H[r] = 0
            H[r, rng.choice(n, min(w, n), replace=False)] = 1
    if m >= 13 and rng.random() < 0.4:
        cols = rng.choice(n, 2, replace=False)
        H[:, cols[0]] = 0                                # an isolated variable
        H[:, cols[1]] = 0
        H[rng.choice(m, int(rng.integers(6, 13)), replace=False), cols[1]] = 1     # one heavy column: weight 6 .. 12
    if n >= 4 and m >= 4 and rng.random() < 0.35:
        k = int(rng.integers(1, 4))
        src, dst = rng.choice(n, (2, k), replace=False) if 2 * k <= n else (np.array([0]), np.array([1]))
        H[:, dst] = H[:, src]                            # tied reliabilities: the index tie-break
        src, dst = rng.choice(m, (2, 1), replace=False)
        H[dst] = H[src]                                  # a dependent row: rank deficiency
    return H


def _near(rng, unit, ks):
    """k * unit - 1, k * unit or k * unit + 1."""
    return int(rng.choice(ks)) * unit + int(rng.integers(-1, 2))


def draw_matrix(rng, family, index, max_m=320, max_n=720):
    """(kind, H, notes): a matrix the LDS build of `family` takes.  Every fifth case is of the "passes" kind, below, on
    and above the thread count in turn; the other kinds are drawn."""
    for _ in range(100):
        notes = set()
        kind = "passes" if index % 5 == 3 else str(rng.choice(["base", "word", "word", "pow2", "m256", "rows"]))
        if kind == "base":
            kind, H = random_matrix(rng)
            H = H.copy()
        elif kind == "word":
            # m and n around multiples of 64 and of 32: the last word of a bit-packed row [H | residual] is empty, full
            # or holds one bit; the syndrome ballot's last 64 checks likewise
            unit = int(rng.choice([32, 64]))
            m = _near(rng, unit, [1, 2, 3, 4] if unit == 64 else [1, 3, 5, 7])
            n = _near(rng, unit, [1, 2, 3, 4, 6, 8] if unit == 64 else [1, 3, 5, 9, 13])
            H = _sparse(rng, m, n)
        elif kind == "pow2":
            # n on a power of two (the bitonic sort runs without a padding key) and one past it (NP - 1 padding keys)
            n = int(rng.choice([32, 64, 128, 256, 512])) + int(rng.integers(0, 2))
            H = _sparse(rng, int(rng.integers(max(4, n // 4), max(5, min(n, 300)))), n)
        elif kind == "passes":
            H = _passes(rng, family, notes, index % 3 - 1, max_m)
        elif kind == "m256":
            # m straddling 256: the syndrome test of the 256-thread kernels (layered, quant) takes a second pass
            m = int(rng.choice([255, 256, 257, 258]))
            H = _sparse(rng, m, int(rng.integers(m, 2 * m + 8)))
        else:
            m = int(rng.integers(8, 200))
            H = _sparse(rng, m, int(rng.integers(max(12, m // 2), 2 * m + 40)))
        if kind != "passes":
            H = _decorate(rng, H, notes)
        m, n = H.shape
        if m > max_m or (n > max_n and kind != "passes") or not fits(family, H):
            continue
        return kind, np.ascontiguousarray(H, np.int64), notes | shape_notes(H)
    raise AssertionError(f"no matrix for {family}")


def shape_notes(H):
    """The situations a matrix shows, read off the matrix itself."""
    m, n = H.shape
    rw, cw = H.sum(1), H.sum(0)
    out = set()
    if m % 32 in (31, 0, 1):
        out.add("word_m")
    if n % 32 in (31, 0, 1):
        out.add("word_n")
    if n >= 32 and n & (n - 1) == 0:
        out.add("pow2_n")
    if n > 32 and (n - 1) & (n - 2) == 0:
        out.add("pow2_n_plus_1")
    if 255 <= m <= 258:
        out.add("m_at_256")
    for w in (0, 1, 8, 9):
        if (rw == w).any():
            out.add(f"row_{w}")
    if (rw >= 20).any():
        out.add("row_long")
    if (cw == 0).any():
        out.add("col_0")
    if (cw >= 6).any():
        out.add("col_heavy")
    live = H[:, cw > 0]
    if live.shape[1] and len(np.unique(live, axis=1).T) < live.shape[1]:
        out.add("dup_cols")
    live = H[rw > 0]
    if len(live) and len(np.unique(live, axis=0)) < len(live):
        out.add("dup_rows")
    return out


# ---- priors, syndromes, second-stage inputs --------------------------------------------------------------------------
def draw_prior(rng, n, family, notes, integer=False, uniform=None):
    """(prior, pv): uniform or per column; with probability 0.15 a few entries from EXTREMES, as far as the family's
    entry accepts them; integer-valued for the fixed-point decoder (clamping at +-M and exact zeros occur)."""
    if rng.random() < 0.5 if uniform is None else uniform:
        pv = np.full(n, rng.uniform(0.005, 0.2))
        notes.add("prior_uniform")
    else:
        pv = rng.uniform(0.005, 0.3, n)
        notes.add("prior_per_column")
    prior = np.log((1 - pv) / pv)
    if integer:
        prior = np.rint(prior * rng.choice([0.5, 1.0, 3.0]))
    if rng.random() < 0.15:
        allowed = [x for x in EXTREMES if np.isfinite(x) or family not in FINITE_ONLY]
        prior[rng.choice(n, max(1, n // 8), replace=False)] = rng.choice(allowed)
        notes.add("prior_extreme")
    return prior, pv


def draw_weight(rng, n):
    """The expected number of errors of a case's records: light (BP solves most, at once or late) in three cases of
    five, else up to n / 10 (most records are never solved).  A rate per bit, as tests/test_gpu_fuzz.py draws it, leaves
    the record kernels' matrices -- n in the hundreds -- with unsolved records only."""
    return float(rng.uniform(0.3, 5.0) if rng.random() < 0.6 else rng.uniform(5.0, max(6.0, n / 10)))


def draw_syndromes(rng, H, pv, B, notes, weight):
    """Errors of `weight` expected flips, spread over the columns as their probabilities pv, and their syndromes --
    sometimes with a row outside the column space."""
    err = (rng.random((B, H.shape[1])) < np.minimum(0.5, pv / pv.sum() * weight)).astype(np.uint8)
    syn = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    if rng.random() < 0.2:
        syn[rng.integers(0, B)] = rng.random(H.shape[0]) < 0.5           # a syndrome outside the model
        notes.add("syn_outside")
    return err, syn


def draw_decoder_outputs(rng, H, prior, pv, B, notes):
    """(syn, llr, hard) for order-w OSD and LSD: random llr, a share rounded (ties) with a few NaN; or what BP(50)
    leaves of Bernoulli errors (light residuals, as in use).  In two cases of five, half of the records get syndrome
    bits flipped afterwards: on a matrix with an empty or a dependent row they leave the column space."""
    m, n = H.shape
    if rng.random() < 0.4:
        _, syn = draw_syndromes(rng, H, pv, B, set(), draw_weight(rng, n) * 1.5)
        finite = np.where(np.isfinite(prior), prior, 0.0)
        hard, _, _, llr = oracle.decode_batch(H, syn, finite, 50, threads=8)
        llr, hard = np.ascontiguousarray(llr), np.ascontiguousarray(hard, np.uint8)
        flip = 2.0 / m
        notes.add("llr_bp")
    else:
        llr = rng.normal(0, 5, (B, n))
        if rng.random() < 0.6:
            llr = np.round(llr)                                          # many ties in |llr|
            notes.add("llr_ties")
            if rng.random() < 0.5:
                llr[rng.integers(0, B, 3), rng.integers(0, n, 3)] = np.nan
                notes.add("llr_nan")
        hard = (llr < 0).astype(np.uint8)
        err = (rng.random((B, n)) < 0.1).astype(np.int64)
        syn = (err @ H.T % 2).astype(np.uint8)
        if rng.random() < 0.4:                                           # light residuals
            hard = ((err + (rng.random((B, n)) < 0.02)) % 2).astype(np.uint8)
        flip = 0.5
    if rng.random() < 0.4:
        rows = rng.choice(B, -(-B // 2), replace=False)
        syn[rows] ^= (rng.random((len(rows), m)) < flip).astype(np.uint8)
        notes.add("syn_outside")
    return syn, llr, hard


def draw_B(rng, cap):
    """B from BATCHES, from those the statement's cost allows (`cap` records; 1 is always allowed)."""
    return int(rng.choice([b for b in BATCHES if b <= max(1, cap)]))


# ---- the cases -----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, index, kind, H, notes, **kw):
        self.family, self.index, self.kind, self.notes = family, index, kind, notes
        self.H = np.ascontiguousarray(H, np.uint8)
        self.m, self.n = H.shape
        self.par = {}
        self.__dict__.update(kw)

    @property
    def tag(self):
        par = {k: (v if np.isscalar(v) or isinstance(v, (str, tuple)) else "...") for k, v in self.par.items()}
        return f"case {self.index} {self.family} {self.kind} {self.m}x{self.n} B={self.B} {par}"


def count_of(family, cases=None):
    """Cases per family: QBP_FUZZ_CASES, a third of it where the statement is the cost (LSD), a quarter for the
    Monte-Carlo compositions."""
    cases = CASES if cases is None else cases
    return max(cases // 3, 6) if family == "lsd" else max(cases // 4, 6) if family == "counters" else cases


def _osd_order(rng, i):
    kind, H, notes = draw_matrix(rng, "osd_order", i)
    m, n = H.shape
    B = draw_B(rng, 2_500_000 // (m * n))
    prior, pv = draw_prior(rng, n, "osd_order", notes)
    syn, llr, hard = draw_decoder_outputs(rng, H, prior, pv, B, notes)
    c = Case("osd_order", i, kind, H, notes, B=B, syn=syn, llr=llr, hard=hard)
    c.par = dict(method=str(rng.choice(["cs", "e"])), w=int(rng.integers(1, 9)))
    return c


def _relay(rng, i):
    kind, H, notes = draw_matrix(rng, "relay", i)
    m, n = H.shape
    B = draw_B(rng, 60_000 // n)
    prior, pv = draw_prior(rng, n, "relay", notes)
    # half of the cases between light and heavy: where leg 0 fails on some records and a later leg solves them, and
    # where a second solution is lighter than the first
    _, syn = draw_syndromes(rng, H, pv, B, notes, rng.uniform(1.5, 8.0) if rng.random() < 0.5 else draw_weight(rng, n))
    legs = int(rng.choice([1, 2, 3, 4], p=[0.1, 0.2, 0.3, 0.4]))       # (a second solution needs a second leg)
    gammas = relay.relay_gammas(n, legs, float(rng.choice([0.0, 0.125, 0.3])), (-0.24, 0.66), int(rng.integers(0, 1000)))
    if rng.random() < 0.3:
        gammas[rng.integers(0, legs)] = 0.0                              # an all-zero leg: plain min-sum
    c = Case("relay", i, kind, H, notes, B=B, syn=syn, prior=prior, gammas=gammas,
             leg_iters=rng.integers(2, 13, legs).astype(np.int32))
    c.par = dict(legs=legs, leg_iters=tuple(c.leg_iters.tolist()), stop_after=int(rng.choice([1, 2, 3], p=[0.25, 0.35, 0.4])),
                 alpha=float(rng.uniform(0.6, 1.0)))
    return c


def _layered(rng, i):
    kind, H, notes = draw_matrix(rng, "layered", i)
    m, n = H.shape
    B = draw_B(rng, 60_000 // n)
    prior, pv = draw_prior(rng, n, "layered", notes)
    _, syn = draw_syndromes(rng, H, pv, B, notes, draw_weight(rng, n))
    variant = int(rng.choice([SUM_PRODUCT, MIN_SUM]))
    c = Case("layered", i, kind, H, notes, B=B, syn=syn, prior=prior)
    c.par = dict(variant=variant, alpha=1.0 if variant == SUM_PRODUCT else float(rng.uniform(0.6, 1.0)),
                 max_iter=int(rng.choice([1, 2, 7, 30])), order=str(rng.choice(["default", "ascending", "random"])),
                 slots=int(rng.choice([0, 1, 2, 5])), force_full=bool(rng.random() < 0.3))
    return c


def _gd(rng, i):
    rounds = rng.choice(["0", "1", "6", "n"])
    if rounds == "n" and i % 5 == 3:
        rounds = "6"                                     # (the "passes" kind is no small matrix)
    # max_rounds = n runs the candidates to exhaustion: a record BPGD never solves costs the statement n rounds, so
    # those cases take the small kinds
    kind, H, notes = draw_matrix(rng, "gd", i, *((64, 96) if rounds == "n" else ()))
    m, n = H.shape
    B = draw_B(rng, (3_000 if rounds == "n" else 40_000) // n)
    prior, pv = draw_prior(rng, n, "gd", notes, uniform=rng.random() < 0.6)       # uniform: ties in |V|
    _, syn = draw_syndromes(rng, H, pv, B, notes, draw_weight(rng, n))
    variant = int(rng.choice([SUM_PRODUCT, MIN_SUM]))
    c = Case("gd", i, kind, H, notes, B=B, syn=syn, prior=prior)
    c.par = dict(variant=variant, alpha=1.0 if variant == SUM_PRODUCT else float(rng.uniform(0.6, 1.0)),
                 T=int(rng.choice([1, 3, 8])), max_rounds=n if rounds == "n" else int(rounds),
                 decim_llr=float(rng.choice([25.0, 1e3])))
    return c


def _lsd(rng, i):
    g = int(rng.choice([0, 1, 3]))
    # the statement is the cost: m <= 130 and B <= 17 for g >= 1, twice that size for g = 0 (every candidate at once)
    kind, H, notes = draw_matrix(rng, "lsd", i, *((130, 300) if g else (260, 520)))
    m, n = H.shape
    B = draw_B(rng, min(17 if g else 64, 1_500_000 // (m * n)))
    prior, pv = draw_prior(rng, n, "lsd", notes)
    syn, llr, hard = draw_decoder_outputs(rng, H, prior, pv, B, notes)
    c = Case("lsd", i, kind, H, notes, B=B, syn=syn, llr=llr, hard=hard)
    c.par = dict(g=g, g2=int(rng.choice([x for x in (0, 1, 3) if x != g])))
    return c


ALPHAS = ((1, 0), (1, 1), (3, 2), (7, 3), (13, 4))       # dyadic fractions num / 2^shift


def _quant(rng, i):
    kind, H, notes = draw_matrix(rng, "quant", i)
    m, n = H.shape
    B = draw_B(rng, 4_000_000 // (m * n))                # (the statement keeps dense [B, m, n] arrays)
    prior, pv = draw_prior(rng, n, "quant", notes, integer=True)
    _, syn = draw_syndromes(rng, H, pv, B, notes, draw_weight(rng, n))
    E = int(H.sum())
    c = Case("quant", i, kind, H, notes, B=B, syn=syn, prior=prior)
    c.par = dict(bits=int(rng.choice([2, 4, 6, 8, 9, 16])), scale=float(rng.choice([0.5, 1.0, 2.0])),
                 alpha=tuple(int(x) for x in ALPHAS[rng.integers(0, len(ALPHAS))]), beta=int(rng.integers(0, 2)),
                 slots=int(rng.choice([0, 1, 3])), max_iter=int(rng.choice([x for x in (1, 2, 7, 30) if x == 1 or x * E <= 15_000])))
    return c


def _cond(rng, i):
    kind, H, notes = draw_matrix(rng, "cond", i)
    m, n = H.shape
    B = draw_B(rng, 30_000 // n)
    prior0, pv = draw_prior(rng, n, "cond", notes)
    prior1, _ = draw_prior(rng, n, "cond", notes)
    if rng.random() < 0.3:
        prior1 = np.zeros(n)                             # the depolarizing second table
    _, syn = draw_syndromes(rng, H, pv, B, notes, draw_weight(rng, n))
    constant = rng.random() < 0.25
    if constant:
        sel = np.full((B, n), rng.choice([0, 1, 2, 0xFD]), np.uint8)
    else:
        sel = ((rng.random((B, n)) < rng.choice([0.05, 0.5])) * rng.choice([1, 3, 255], (B, n))).astype(np.uint8)
    variant = int(rng.choice([SUM_PRODUCT, MIN_SUM]))
    c = Case("cond", i, kind, H, notes, B=B, syn=syn, prior0=prior0, prior1=prior1, sel=sel)
    c.par = dict(variant=variant, alpha=1.0 if variant == SUM_PRODUCT else float(rng.uniform(0.6, 1.0)),
                 max_iter=int(rng.choice([1, 2, 7, 25])), constant=bool(constant))
    return c


STAGES = ("relay", "gd", "lsd", "osd_cs", "layered", "quant_lsd")


def _counters(rng, i):
    kind, H, notes = draw_matrix(rng, "counters", i, 130, 300)
    m, n = H.shape
    stage = STAGES[i % len(STAGES)]
    B = draw_B(rng, 8 if stage in ("lsd", "quant_lsd") else 40_000 // n)
    p = float(rng.uniform(0.01, 0.08))
    errors = (rng.random((B, n)) < min(0.5, rng.uniform(1.0, 6.0) / n)).astype(np.uint8)   # a few flips per record
    k = int(rng.integers(1, 10))
    c = Case("counters", i, kind, H, notes, B=B, errors=errors, p=p, Lx=(rng.random((k, n)) < 0.3).astype(np.uint8),
             distance=int(rng.integers(2, 12)), seed=int(rng.integers(0, 1000)))
    c.par = dict(stage=stage, k=k, distance=c.distance, w=int(rng.integers(1, 9)), g=int(rng.choice([0, 1, 3])),
                 variant=int(rng.choice([SUM_PRODUCT, MIN_SUM])))
    return c


_DRAW = dict(osd_order=_osd_order, relay=_relay, layered=_layered, gd=_gd, lsd=_lsd, quant=_quant, cond=_cond,
             counters=_counters)
_CASES, _STATEMENTS = {}, {}
SECONDS = {}                                             # family -> seconds its statements took


def cases(family, cases=None, seed=None):
    """The cases of a family: the same list for the same (count, seed), drawn once."""
    count, seed = count_of(family, cases), SEED if seed is None else seed
    key = (family, count, seed)
    if key not in _CASES:
        rng = np.random.default_rng([seed, FAMILIES.index(family)])
        _CASES[key] = [_DRAW[family](rng, i) for i in range(count)]
    return _CASES[key]


# ---- the statements --------------------------------------------------------------------------------------------------------
def order_perm(c):
    return lo.order_of(c.H, c.par["order"])


def statement(c):
    """The numpy statement on one case, computed once and left unchanged."""
    key = id(c)
    if key in _STATEMENTS:
        return _STATEMENTS[key][1]
    p, H = c.par, c.H
    start = time.perf_counter()
    if c.family == "osd_order":
        reds = [oo.reduce(H, s, l, h) for s, l, h in zip(c.syn, c.llr, c.hard)]
        sol = np.stack([oo.osd_order(H, s, l, h, p["w"], p["method"], red=r)
                        for s, l, h, r in zip(c.syn, c.llr, c.hard, reds)])
        out = dict(solution=sol, consistent=np.array([r.consistent for r in reds]),
                   improved=np.array([bool((x != r.x0).any()) for x, r in zip(sol, reds)]))
    elif c.family == "relay":
        out = ro.relay_decode_batch(H, c.syn, c.prior, c.gammas, c.leg_iters, p["stop_after"], p["alpha"])
    elif c.family == "layered":
        out = lo.layered_decode_batch(H, c.syn, c.prior, p["max_iter"], p["variant"], p["alpha"], 20.0, order_perm(c))
    elif c.family == "gd":
        out = go.gd_decode_batch(H, c.syn, c.prior, p["T"], p["max_rounds"], p["decim_llr"], p["variant"], p["alpha"], 20.0)
    elif c.family == "lsd":
        out = lso.lsd_decode_batch(H, c.syn, c.llr, c.hard, p["g"])
    elif c.family == "quant":
        out = qo.decode_batch(H, c.syn, c.prior, p["max_iter"], p["bits"], p["scale"], *p["alpha"], p["beta"])
    elif c.family == "cond":
        out = co.decode_cond(H, c.syn, c.sel, c.prior0, c.prior1, p["max_iter"], p["variant"], p["alpha"], 20.0)
    else:
        raise KeyError(c.family)
    SECONDS[c.family] = SECONDS.get(c.family, 0.0) + time.perf_counter() - start
    _STATEMENTS[key] = (c, out)
    return out


def iteration_classes(conv, iters):
    """(converged at the first iteration, converged later, never converged)"""
    conv, iters = np.asarray(conv, bool), np.asarray(iters)
    return dict(first=int((conv & (iters == 0)).sum()), late=int((conv & (iters > 0)).sum()), never=int((~conv).sum()))


def classes(c):
    """The outcome classes of a case's statement, as its family's own test names them."""
    r = statement(c)
    if c.family == "relay":
        return ro.classes(r)
    if c.family == "gd":
        return go.classes(r)
    if c.family == "lsd":
        s = r["stats"]
        return dict(one_cluster=int(((s[:, 2] == 1) & (s[:, 3] == 1)).sum()), merged=int(r["merged"].sum()),
                    invalid=int((s[:, 3] == 0).sum()))
    if c.family in ("layered", "quant", "cond"):
        return iteration_classes(r[1], r[2])
    if c.family == "osd_order":
        return dict(improved=int(r["improved"].sum()), osd0=int((~r["improved"]).sum()))
    raise KeyError(c.family)


def pooled(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


def situations(family, cases=None, seed=None):
    """How many cases of a family show each situation."""
    out = {k: 0 for k in SITUATIONS + (INPUT_SITUATIONS if family in ("osd_order", "lsd") else ())}
    for c in globals()["cases"](family, cases, seed):
        for k in c.notes:
            out[k] += 1
    return out


def second_batch(rng_seed, c, num_cu=0):
    """Row indices of the repeated call of a case (every fifth): another B from BATCHES, or -- `num_cu` given -- more
    records than a grid of one workgroup per CU; the case's records in turn, so the statement's rows serve again."""
    rng = np.random.default_rng([rng_seed, c.index])
    B2 = int(rng.choice([b for b in BATCHES if b != c.B]))
    if num_cu and rng.random() < 0.5:
        B2 += num_cu
    return (np.arange(B2) + int(rng.integers(0, c.B))) % c.B
