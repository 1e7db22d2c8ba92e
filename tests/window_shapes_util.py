"""Inputs, thresholds and the vectorised classification shared by tests/test_gpu_window_shapes.py and its CPU companion
tests/test_window_shapes_cpu.py.  Nothing here needs a GPU."""
import numpy as np

import window_oracle as wo
from test_window_plan import P_OF, matrix

# qbp_window.hpp: WINDOW_MAX_GRID = 2048 blocks of WINDOW_THREADS = 256 lanes are the most window_grid()
# (qbp_tu_window.hip) gives a launch; the grid-stride loops cover the rest in further passes.
GRID_LANES = 2048 * 256               # items of one pass of window_gather_kernel, window_commit_kernel<false>,
#                                       window_syndrome_kernel and window_fail_list_kernel
GRID_WAVES = 2048 * 4                 # records of one pass of the wavefront-per-record kernels: window_commit_kernel<true>
#                                       and window_classify_kernel

MAX_ITER, ALPHA, DAMPING, CLIP = 8, 0.9, 0.75, 20.0          # (those of tests/test_gpu_window.py)
SIZES = ((3, 1), (4, 2))
STRIDE_B, STRIDE_SEED = 60000, 31                            # A1 and A10: records of one decode call
MC_T, MC_BEGIN, MC_SEED, MC_DISTANCE = 60000, 1000, 77, 6    # A2 and A3: trials of one chunk
LIST_B, LIST_SEED = GRID_LANES + 4099, 47                    # A4: records of one decode call
LIST_TAIL = GRID_LANES - 4099                                # ... every row from here on is compared, below it every 64th


def inputs(name, batch, seed):
    """(H, check_round, errors, syndromes, prior) as tests/test_gpu_window.py draws them."""
    H, cr = matrix(name)
    p = P_OF[name]
    errors = (np.random.default_rng(seed).random((batch, H.shape[1])) < p).astype(np.uint8)
    return H, cr, errors, syndromes_of(H, errors), np.full(H.shape[1], np.log((1 - p) / p))


def syndromes_of(H, errors):
    return (errors.astype(np.int32) @ np.asarray(H, np.int32).T & 1).astype(np.uint8)


def mc_inputs(name="steane"):
    """(L, probs) of the Monte-Carlo tests: five random rows, a probability per column."""
    n = matrix(name)[0].shape[1]
    L = (np.random.default_rng(2).random((5, n)) < 0.3).astype(np.uint8)
    return L, np.linspace(0.5, 1.5, n) * P_OF[name]


def list_rows():
    """The rows of A4 the statement is computed on: every 64th below LIST_TAIL, every one from there on."""
    return np.concatenate([np.arange(0, LIST_TAIL, 64), np.arange(LIST_TAIL, LIST_B)])


# ---- the thresholds ----------------------------------------------------------------------------------------------------
def window_work(H, cr, W, F):
    """Per decoded window of wo.plan: (m_k = |C_k|, n_commit = |M_k|, n_upd = the checks of H, inside or outside the
    window, with an entry in a column of M_k).  window_commit_kernel<false> has n_upd + n_commit + 1 items per record."""
    H = wo.dense(H)
    out = []
    for C, U, M, _ in wo.windows(H, wo.plan(H, cr, W, F)):
        if C.size and U.size:
            out.append((int(C.size), int(M.sum()), int(H[:, U[M]].any(axis=1).sum())))
    return out


def assert_every_loop_strides(B, H, cr, W, F):
    """Every glue kernel of a B-record decode call takes a second trip in every window; -> the first row that no
    window's gather reaches in its first pass.  Prints the figures."""
    work = window_work(H, cr, W, F)
    assert work
    for k, (mk, n_commit, n_upd) in enumerate(work):
        gather, commit = B * mk, B * (n_upd + n_commit + 1)
        print(f"(W, F) = ({W}, {F}) window {k}: gather {B} x {mk} = {gather} lanes, commit {B} x ({n_upd} + {n_commit} + 1) "
              f"= {commit} lanes against {GRID_LANES}; final {B} records against {GRID_WAVES}")
        assert gather > GRID_LANES and commit > GRID_LANES and B > GRID_WAVES, (W, F, k, work[k])
    return GRID_LANES // max(mk for mk, _, _ in work)


def kinds(want):
    """How many records of a statement's output are of each kind: every window's BP converged, a second stage ran
    (window_fails > 0), the correction misses the syndrome (converged == 0)."""
    _, conv, _, _, fails = want
    return int((fails == 0).sum()), int((fails > 0).sum()), int((~np.asarray(conv, bool)).sum())


def assert_kinds(want, osd, what):
    """At least 8 records of each kind, the last without OSD only (OSD-0 meets every syndrome of the column space)."""
    k = kinds(want)
    print(f"{what}: all windows converged {k[0]}, second stage {k[1]}, missed {k[2]}")
    assert k[0] >= 8 and k[1] >= 8 and (osd or k[2] >= 8), (what, k)
    return k


# ---- the classification ------------------------------------------------------------------------------------------------
def classify(H, L, distance, errors, x, iters, fails):
    """window_classify_kernel's rule on whole arrays: oracle.classify_trials with detection = x and converged =
    (window_fails == 0) -- [5] asks H x == s itself, so it also counts a correction that OSD made valid -- and [10] the
    corrections that miss the syndrome.  -> (counters int64[12], valid bool[T])."""
    H, L = np.asarray(H, np.int32), np.asarray(L, np.int32)
    e, d = np.asarray(errors, np.int32) & 1, np.asarray(x, np.int32) & 1
    residual = e ^ d
    logical = (residual @ L.T & 1).any(axis=1)
    valid = ~((residual @ H.T) & 1).any(axis=1)              # H x == H e
    differs = residual.any(axis=1)
    light = e.sum(axis=1) < distance // 2
    conv = np.asarray(fails) == 0
    cnt = np.zeros(12, np.int64)
    cnt[0] = e.shape[0]
    cnt[1] = logical.sum()
    cnt[3] = (logical & light).sum()
    cnt[4] = (logical & ~light).sum()
    cnt[5] = (valid & ~logical & differs).sum()
    cnt[6] = (~conv).sum()
    cnt[7] = np.asarray(iters, np.int64).sum()
    cnt[8] = (logical & ~conv).sum()
    cnt[9] = (~differs).sum()
    cnt[10] = (~valid).sum()
    return cnt, valid


# ---- matrices whose windows leave the on-chip kernel ------------------------------------------------------------------
# The on-chip BP kernel takes rows of at most 8 entries and columns of at most 4 (DC_WIDE, DV_WIDE of qbp_launch.hpp).
ON_CHIP_MAX_ROW, ON_CHIP_MAX_COL = 8, 4
HEAVY_P = 0.03


def ring(heavy_row=False):
    """6 x 12: row i has columns 2i .. 2i + 3 (mod 12) -- rows of weight 4, columns of weight 2; ``heavy_row``: row 0
    has columns 0 .. 8 instead, weight 9."""
    Hx = np.zeros((6, 12), np.uint8)
    for i in range(6):
        Hx[i, (2 * i + np.arange(4)) % 12] = 1
    if heavy_row:
        Hx[0] = 0
        Hx[0, :9] = 1
    return Hx


def heavy_everywhere():
    """36 x 108, six rounds of the ring with the weight-9 row: every window holds rows of weight 10 or 11."""
    return wo.spacetime(ring(True), 6)


def heavy_last_round():
    """37 x 108: six rounds of the plain ring, and one more check of weight 9 in round 5 on that round's columns
    60 .. 68.  Only the windows that hold round 5 leave the on-chip kernel."""
    H, cr = wo.spacetime(ring(), 6)
    row = np.zeros((1, H.shape[1]), np.uint8)
    row[0, 60:69] = 1
    return np.vstack([H, row]), np.append(cr, 5).astype(np.int32)


def heavy_inputs(make, batch=257, seed=5):
    H, cr = make()
    errors = (np.random.default_rng(seed).random((batch, H.shape[1])) < HEAVY_P).astype(np.uint8)
    return H, cr, errors, syndromes_of(H, errors), np.full(H.shape[1], np.log((1 - HEAVY_P) / HEAVY_P))


def fits_on_chip(Hk):
    return bool(Hk.sum(axis=1).max() <= ON_CHIP_MAX_ROW and Hk.sum(axis=0).max() <= ON_CHIP_MAX_COL)
