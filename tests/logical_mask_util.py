"""Inputs of tests/test_logical_mask_cpu.py and tests/test_gpu_logical_mask.py: logical operators placed on the high
bits of the 64-bit word a trial's classification folds (lm, the XOR of lx_cols[v] over the residual's support; bit l
of lx_cols[v] is Lx[l][v]), and what a classification that looks at ``lm != 0`` alone must then return.  No GPU here.

A placement is ``(name, L', map)``: ``map[i]`` is the row of L' that holds base row i, -1 where L' leaves it out;
every other row of L' is zero.  ``lm' != 0`` exactly when ``L[map >= 0] @ residual`` is non-zero, so the counters
of a run with L' are those of the run with ``L[map >= 0]``, digit for digit."""
import numpy as np

import lsd_util
from qldpc_amd import codes

P, MAX_ITER, TRIALS, SEED = 0.06, 8, 1500, 3
SINGLE_BITS = (31, 32, 63)
SINGLE_ROWS = (0, 1)
L_FREE = (0, 6, 7, 9, 10)          # counters that do not look at the logical operators
L_ONLY = (1, 3, 4, 8)              # counters of logical errors: zero without logical operators


def _placed(L, rows, map_, k):
    L = np.asarray(L, np.uint8)
    out = np.zeros((k, L.shape[1]), np.uint8)
    full = np.full(L.shape[0], -1, np.int64)
    for i, b in zip(rows, map_):
        out[b] = L[i]
        full[i] = b
    return out, full


def single(L, r, b):
    """64 rows, only row b non-zero: base row r."""
    return (f"single({r},{b})",) + _placed(L, [r], [b], 64)


def placements(L):
    """The named placements of a base L [k0, n], k0 <= 12, in the order the GPU tests run them on one handle:
    consecutive ``single`` calls keep k = 64 and differ in one row, which a stale upload would not notice."""
    k0 = np.asarray(L).shape[0]
    assert 2 <= k0 <= 12
    rows = list(range(k0))
    yield ("top",) + _placed(L, rows, [64 - k0 + i for i in rows], 64)
    yield ("straddle",) + _placed(L, rows, [32 - k0 // 2 + i for i in rows], 64)
    yield ("spread",) + _placed(L, rows, [5 * i + 4 for i in rows], 64)
    yield ("k33",) + _placed(L, [0], [32], 33)
    for b in SINGLE_BITS:
        for r in SINGLE_ROWS:
            yield single(L, r, b)


def kept(L, map_):
    """The base rows a placement keeps, in base order: the L of the run it must equal."""
    return np.ascontiguousarray(np.asarray(L, np.uint8)[np.asarray(map_) >= 0])


def move_bits(masks, map_):
    """uint64 masks over the base rows -> masks over the rows of L': bit i goes to bit map[i], dropped where -1."""
    masks = np.asarray(masks, np.uint64)
    out = np.zeros_like(masks)
    for i, b in enumerate(np.asarray(map_)):
        if b >= 0:
            out |= ((masks >> np.uint64(i)) & np.uint64(1)) << np.uint64(b)
    return out


def low_half(Lp):
    """L' with rows 32 .. 63 zeroed: what a fold through a 32-bit temporary would classify with."""
    out = np.array(Lp, np.uint8)
    out[32:] = 0
    return out


def code72():
    c = codes.load_code("[[72, 12, 6]]")
    return np.asarray(c.Hx, np.uint8), np.asarray(c.Lx, np.uint8), c.distance


def irregular():
    """The irregular 20 x 37 matrix of the Relay-BP / BPGD / LSD tests (lsd_util.irregular37: rows of weight 1 .. 13,
    columns of weight 1 .. 7, the general-H kernel) with 12 random logical rows.  Their density is 0.15 (3 to 9 ones per
    row), chosen on the CPU oracle: at 0.3 any six of the rows already see all but 7 of the 480 logical errors, and
    the loss of the other six would hardly show."""
    H = lsd_util.irregular37()
    L = (np.random.default_rng(12).random((12, H.shape[1])) < 0.15).astype(np.uint8)
    return H, L, 4


def prior_of(n, p=P):
    return np.full(n, np.log((1 - p) / p))


def extra_row(L):
    """k = 13: the 12 rows of L, the same bytes, and one random row more."""
    L = np.asarray(L, np.uint8)
    row = (np.random.default_rng(13).random((1, L.shape[1])) < 0.3).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([L, row]))
