"""Helpers of tests/test_gpu_record_kernel_sizes.py: the launch arithmetic of the three per-record decoders restated in
Python (record_threads of qbp_record_bp.hpp, gd_lds_bytes of qbp_gd.hpp, relay_lds_bytes of qbp_relay.hpp,
layered_lds_bytes of qbp_layered.hpp, the grids of gd_launch / relay_launch / layered_launch and layered_slots of
qbp.hip -- usable without a GPU), the matrices large enough that a workgroup walks its strided loops more than once,
and launches of the device entries into poisoned buffers (geometry_util.Outputs plus the decoders' extra int32
outputs).

Work items: the general-H tables pad every weight class to whole wavefronts, so the check step has
sum_{k=1..8} pad64(#rows of weight k) items and the variable step sum_{k=1..4} pad64(#columns of weight k); rows beyond
8 and columns beyond 4 are "long" and take loops of their own, columns of weight 0 sit before col_off[1]."""
import functools
import os
import re

import numpy as np

import geometry_util as gu
import layered_oracle as lo
from qldpc_amd import _lib, dem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC, CC = 8, 4                                # GENERIC_MAX_ROW_CLASS, GENERIC_MAX_COL_CLASS
GD_MAX_THREADS, RELAY_MAX_THREADS = 512, 1024
GD_HEAD_WORDS = 8 + 4 * (GD_MAX_THREADS // 64)
LAYERED_THREADS, LAYERED_MAX_SLOTS, LAYERED_WG_WORDS, LAYERED_SLOT_HEAD = 256, 32, 32, 10
LDS_LIMIT = 160 * 1024
LDS_DEFAULT = 64 * 1024                      # dynamic LDS a kernel gets without hipFuncSetAttribute
INT_POISON = -1


@functools.lru_cache(maxsize=None)
def np_lds_bytes():
    """NP_LDS_BYTES = sizeof(NpImage) of qbp_math.hpp: the members are arrays of uint64_t."""
    text = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp_math.hpp")).read()
    body = re.search(r"struct NpImage \{(.*?)\n\};", text, re.S).group(1)
    total = 0
    for dims in re.findall(r"^\s*uint64_t \w+((?:\[\d+\])+);", body, re.M):
        total += 8 * int(np.prod([int(d) for d in re.findall(r"\d+", dims)]))
    assert total > 0
    return total


# ---- work items and launch geometry (no GPU) ------------------------------------------------------------------------
def pad64(x):
    return -(-int(x) // 64) * 64


class Shape:
    """What the launch arithmetic needs of a matrix: m, n, E, the padded work counts and the long / empty classes."""

    def __init__(self, H):
        Hb = np.asarray(H) != 0
        self.m, self.n = Hb.shape
        self.row_w, self.col_w = Hb.sum(axis=1), Hb.sum(axis=0)
        self.E = int(self.row_w.sum())
        self.check_items = sum(pad64((self.row_w == k).sum()) for k in range(1, RC + 1))
        self.var_items = sum(pad64((self.col_w == k).sum()) for k in range(1, CC + 1))
        self.long_rows = int((self.row_w > RC).sum())
        self.long_edges = int(self.row_w[self.row_w > RC].sum())
        self.long_cols = int((self.col_w > CC).sum())
        self.empty_cols = int((self.col_w == 0).sum())
        self.work = max(self.check_items, self.var_items, 64)


def _threads(work, limit):
    passes = -(-work // limit)
    return pad64(-(-work // passes))


def gd_threads(sh):
    return _threads(sh.work, GD_MAX_THREADS)


def relay_threads(sh):
    return _threads(sh.work, RELAY_MAX_THREADS)


def passes(items, threads):
    return -(-int(items) // int(threads))


def gd_lds_bytes(m, n, E, tables):
    mw, nw = (m + 31) >> 5, (n + 31) >> 5
    words = (GD_HEAD_WORDS + 3 * mw + nw + 1) & ~1
    return (np_lds_bytes() if tables else 0) + 8 * (E + 2 * n) + 4 * words


def relay_lds_bytes(m, n, E, records=False):
    words = (8 + 3 * ((m + 31) >> 5) + 1) & ~1
    return 8 * (E + 3 * n) + 4 * words + (((n + 7) & ~7) if records else 0)


def layered_lds_bytes(m, n, E, S, tables):
    slot_words = (LAYERED_SLOT_HEAD + ((m + 31) >> 5) + 1) & ~1
    return (np_lds_bytes() if tables else 0) + 8 * (n + S * (E + n)) + 4 * (LAYERED_WG_WORDS + S * slot_words)


def gd_grid(sh, B, num_cu, sum_product, blocks_per_cu=0):
    lds = gd_lds_bytes(sh.m, sh.n, sh.E, sum_product)
    per_cu = max(1, min((20 if sum_product else 28) // (gd_threads(sh) // 64), LDS_LIMIT // lds))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return max(1, min(B, num_cu * per_cu))


def relay_grid(sh, B, num_cu):
    lds = relay_lds_bytes(sh.m, sh.n, sh.E)
    per_cu = max(1, min(28 // (relay_threads(sh) // 64), LDS_LIMIT // lds))
    return max(1, min(B, num_cu * per_cu))


def layered_slots(sh, max_width, B, tables, opt_slots=0):
    S = opt_slots
    if S <= 0:
        S = max(1, min(LAYERED_MAX_SLOTS, LAYERED_THREADS // max(1, max_width)))
        while S > 1 and layered_lds_bytes(sh.m, sh.n, sh.E, S, tables) > 80 * 1024:
            S -= 1
    while S > 1 and layered_lds_bytes(sh.m, sh.n, sh.E, S, tables) > LDS_LIMIT:
        S -= 1
    return max(1, min(S, B))


def layered_grid(sh, S, B, num_cu, tables):
    per_cu = max(1, min(5, LDS_LIMIT // layered_lds_bytes(sh.m, sh.n, sh.E, S, tables)))
    return max(1, min(-(-B // S), num_cu * per_cu))


def level_widths(H, order):
    return [len(g) for g in lo.levels_of(H, order)]


# ---- the matrices ---------------------------------------------------------------------------------------------------------
def disjoint300():
    """300 pairwise disjoint checks (one level, wider than the layered kernel's 256 threads): weight 3, but for checks
    270 and 299 of weight 9 -- long rows, both in the ragged second pass of the level in the default order.  Disjoint
    rows of these weights take 298 * 3 + 2 * 9 = 912 columns."""
    weights = np.full(300, 3)
    weights[[270, 299]] = 9
    n = int(weights.sum())
    perm = np.random.default_rng(300).permutation(n)
    H = np.zeros((300, n), np.uint8)
    start = np.concatenate(([0], np.cumsum(weights)))
    for c in range(300):
        H[c, perm[start[c]:start[c + 1]]] = 1
    return H


def ph_shape(T):
    """Shape of dem.phenomenological("[[72, 12, 6]]", T, ...) without building it: m = 36 T, n = 108 T, E = 288 T - 36,
    every row of weight 8 but the first 36 (7), the data columns of weight 3, the measurement columns 2 (last round: 1)."""
    sh = Shape.__new__(Shape)
    sh.m, sh.n, sh.E = 36 * T, 108 * T, 288 * T - 36
    return sh


def largest_rounds(lds_of):
    """The largest T whose ph_shape fits 160 KiB under `lds_of(shape)`."""
    T = 1
    while lds_of(ph_shape(T + 1)) <= LDS_LIMIT:
        T += 1
    return T


NEAR_LIMIT = {
    "relay": lambda sh: relay_lds_bytes(sh.m, sh.n, sh.E),
    "gd_min_sum": lambda sh: gd_lds_bytes(sh.m, sh.n, sh.E, False),
    "gd_sum_product": lambda sh: gd_lds_bytes(sh.m, sh.n, sh.E, True),
    # qbp_layered_configure refuses by the sum-product size (the tables included), whatever variant runs later
    "layered": lambda sh: layered_lds_bytes(sh.m, sh.n, sh.E, 1, True),
}

# tag -> (error rates of the three thirds of the pool -- dem_synth: factors on the model's own probabilities --, seed)
BATCH, POOL = 48, 480
RATES = {"ph72x6": ((0.01, 0.03, 0.05), 6), "ph72x12": ((0.008, 0.02, 0.035), 12), "dem_synth": ((2.0, 5.0, 9.0), 3),
         "disjoint300": ((0.001, 0.003, 0.006), 30)}
TAGS = tuple(RATES)
# The batches are rows of a pool of POOL seeded error patterns per matrix.  The rows were chosen once, on the statements'
# output alone, so that 48 records show every class: a Relay-BP solution replaced by a lighter one is found on about
# one record in sixty, and a record BPGD never solves costs the numpy statement n rounds with max_rounds = n.  The
# tests assert the class counts on the statements' output every time they run.
#   MAIN: every "replaced" record of the pool (at most 14), ten Relay-BP never solves, ten it solves after leg 0, the rest
#         solved in leg 0 (those layered BP solves after iteration 2 first);
#   EASY: records both BPGD variants solve within 40 decimations (those beyond 6 first).
MAIN = {
    "ph72x6": [
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 43, 53, 74, 81, 93, 98, 148, 163, 164, 169, 170, 171, 174,
        176, 178, 179, 182, 188, 229, 233, 239, 248, 263, 273, 274, 296, 298, 309, 316, 318, 339, 414, 479],
    "ph72x12": [
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 41, 63, 92, 98, 108, 115, 117, 124, 142, 160, 172, 181, 183, 186, 191,
        196, 202, 208, 212, 273, 321, 323, 328, 329, 331, 332, 335, 338, 363, 365, 369, 402, 433, 442, 449, 474],
    "dem_synth": [
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 19, 21, 31, 36, 39, 57, 58, 59, 85, 96, 106, 121, 160, 162, 164, 165,
        167, 169, 172, 174, 177, 179, 180, 182, 185, 187, 189, 208, 215, 224, 289, 334, 373, 388, 469],
    "disjoint300": [
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 82, 114, 131,
        137, 139, 141, 146, 163, 166, 167, 170, 194, 195, 220, 250, 318, 330, 332, 351, 353, 354, 356],
}
EASY = {
    "ph72x6": [
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 81, 98, 151, 160, 161,
        165, 166, 170, 174, 175, 177, 183, 184, 187, 193, 194, 199, 218, 236, 251, 292, 298, 317, 427],
    "ph72x12": [
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 52, 63, 75, 90, 96, 108, 122,
        127, 167, 170, 173, 179, 185, 188, 205, 237, 277, 296, 309, 316, 353, 364, 376, 403, 420, 424],
    "dem_synth": [
        0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 85, 96, 103,
        106, 110, 162, 164, 165, 170, 171, 172, 178, 181, 188, 258, 265, 269, 270, 273, 421, 446],
    "disjoint300": [
        0, 1, 2, 3, 5, 6, 7, 10, 12, 13, 14, 15, 16, 17, 18, 20, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
        35, 36, 37, 39, 40, 43, 44, 45, 46, 47, 48, 49, 50, 52, 53, 54, 55, 56, 57],
}


class Case:
    """One matrix with its logical rows, per-column probabilities, non-uniform prior and B error patterns."""

    def __init__(self, tag, H, L, probs, prior, errors):
        self.tag, self.H, self.L, self.probs, self.prior, self.errors = tag, H, L, probs, prior, errors
        self.n = H.shape[1]
        self.syn = gu.syndromes_of(H, errors)
        self.shape = Shape(H)

    def subset(self, rows):
        rows = np.asarray(rows)
        assert len(set(rows.tolist())) == len(rows)
        return Case(self.tag, self.H, self.L, self.probs, self.prior, self.errors[rows])


def _dense(H):
    return np.ascontiguousarray(H.toarray() if hasattr(H, "toarray") else H, dtype=np.uint8)


def noisy_prior(p, n, rng):
    """log((1 - p) / p) * uniform(0.5, 1.5) per variable: with a uniform prior, ties hide permutation mistakes."""
    return np.log((1 - p) / p) * rng.uniform(0.5, 1.5, n)


def draw(probs_list, per, rng):
    return np.concatenate([(rng.random((per, len(pr))) < pr).astype(np.uint8) for pr in probs_list])


def phenomenological(T, p, seed, B):
    """dem.phenomenological("[[72, 12, 6]]", T, p): dense H, L, probs, the noisy prior and B errors at rate p."""
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", T, p, p)
    rng = np.random.default_rng(seed)
    H = _dense(H)
    prior = noisy_prior(p, H.shape[1], rng)
    return Case(f"ph72x{T}", H, L, probs, prior, draw([probs], B, rng))


@functools.lru_cache(maxsize=None)
def case(tag):
    """The batch of the tests: the rows MAIN[tag] of the pool."""
    return pool(tag).subset(MAIN[tag])


@functools.lru_cache(maxsize=None)
def easy(tag):
    """The rows EASY[tag] of the pool: the batch of the BPGD runs with max_rounds = n."""
    return pool(tag).subset(EASY[tag])


@functools.lru_cache(maxsize=None)
def pool(tag):
    rates, seed = RATES[tag]
    rng = np.random.default_rng(seed)
    per = POOL // len(rates)
    if tag.startswith("ph72x"):
        T = int(tag[5:])
        H, L, probs = dem.phenomenological("[[72, 12, 6]]", T, rates[1], rates[1])
        H = _dense(H)
        prior = noisy_prior(rates[1], H.shape[1], rng)
        errors = draw([np.full(H.shape[1], r) for r in rates], per, rng)
    elif tag == "dem_synth":
        from test_gpu_dem import synthetic_dem_text
        H, L, probs = dem.parse_dem(synthetic_dem_text())
        H = _dense(H)
        from qldpc_amd import mc
        prior = mc.dem_prior(probs)                      # the DEM's own probabilities: a different prior per column
        errors = draw([np.minimum(0.5, probs * r) for r in rates], per, rng)
    else:
        H = disjoint300()
        L = (rng.random((3, H.shape[1])) < 0.1).astype(np.uint8)
        probs = np.full(H.shape[1], rates[1])
        prior = noisy_prior(rates[1], H.shape[1], rng)
        errors = draw([np.full(H.shape[1], r) for r in rates], per, rng)
    return Case(tag, H, L, probs, prior, errors)


# ---- launches into poisoned buffers ----------------------------------------------------------------------------------------
class RecordOutputs(gu.Outputs):
    """geometry_util.Outputs plus `extra` int32 outputs (Relay-BP: legs, solutions; BPGD: rounds), poisoned with -1."""

    def __init__(self, rows, n, extra):
        super().__init__(rows, n)
        t = gu.torch()
        self.extra = {k: t.empty(rows + gu.PAD, dtype=t.int32, device="cuda") for k in extra}

    def poison(self):
        super().poison()
        for x in self.extra.values():
            x.fill_(INT_POISON)

    def fetch_all(self, B, iter_limit, what):
        """The four common outputs (checked by Outputs.fetch) and the extra ones: written in [0, B), poison behind."""
        out = list(self.fetch(B, iter_limit, what))
        for k, x in self.extra.items():
            a = x.cpu().numpy()
            assert np.all(a[B:] == INT_POISON), f"{what}: {k} written beyond row B = {B}"
            assert np.all(a[:B] >= 0), f"{what}: {np.flatnonzero(a[:B] < 0)[:8]} never got their {k}"
            out.append(a[:B])
        return tuple(out)

    def untouched(self):
        gu.torch().cuda.synchronize()
        return all(self.poisoned(k, 0) for k in gu.NAMES) and all(bool((x == INT_POISON).all().item())
                                                                   for x in self.extra.values())


def relay_launch(dec, syn_t, prior_t, B, out, stream=0):
    out.poison()
    dec.relay_decode_device(syn_t.data_ptr(), prior_t.data_ptr(), B, out.ptr("hard"), out.ptr("converged"),
                            out.ptr("iters"), out.ptr("llr"), out.extra["legs"].data_ptr(),
                            out.extra["solutions"].data_ptr(), stream=stream)


def gd_launch(dec, syn_t, prior_t, B, out, stream=0):
    out.poison()
    dec.gd_decode_device(syn_t.data_ptr(), prior_t.data_ptr(), B, out.ptr("hard"), out.ptr("converged"),
                         out.ptr("iters"), out.ptr("llr"), out.extra["rounds"].data_ptr(), stream=stream)


def relay_want(r, rows=slice(None)):
    return tuple(r[k][rows] for k in ("hard", "converged", "iters", "llr", "legs", "solutions"))


def gd_want(r, rows=slice(None)):
    return tuple(r[k][rows] for k in ("hard", "converged", "iters", "llr", "rounds"))


def assert_same(got, want, what):
    """geometry_util.assert_same on the four common outputs, np.array_equal on the extra int32 ones."""
    gu.assert_same(got[:4], want[:4], what)
    for i, (x, y) in enumerate(zip(got[4:], want[4:])):
        bad = np.flatnonzero(x != y)
        assert len(bad) == 0, f"{what}: extra output {i} differs on {len(bad)} records, first {bad[:8]}"


def info(dec):
    return dict(threads=dec.info("threads"), grid=dec.info("grid"), lds_bytes=dec.info("lds_bytes"))
