"""Helpers of tests/test_gpu_geometry.py: launch-geometry arithmetic (a restatement of make_cfg / work_chunk in
qldpc_amd/csrc, usable without a GPU) and decode launches into POISONED device buffers.

Poison: before every launch the outputs are filled with values no decode can produce -- hard and converged 0xFF,
iters -1, llr 1.2345e300 (finite: NaN LLRs are legitimate on some priors) -- and are a few rows longer than the batch.
After the launch no sentinel may be left in the first B rows and nothing but sentinels beyond them, so a syndrome a
kernel never wrote, wrote twice at the wrong index, or wrote out of range cannot hide behind an earlier call's result."""
import contextlib

import numpy as np

import golden_util
from qldpc_amd import _lib

LLR_POISON = 1.2345e300
PAD = 3                                      # rows behind the batch that must stay poison
NAMES = ("hard", "converged", "iters", "llr")
FUSED_MAX_THREADS = 1024

OPTS = dict(slots=_lib.OPT_SLOTS_PER_BLOCK, blocks=_lib.OPT_BLOCKS_PER_CU, full_wg=_lib.OPT_EARLY_EXIT_FULL_WG,
            two_barriers=_lib.OPT_FORCED_TWO_BARRIERS, kernel=_lib.OPT_KERNEL, threads=_lib.OPT_GENERAL_THREADS,
            mem=_lib.OPT_GENERAL_MEM, no_r_split=_lib.OPT_GENERAL_NO_R_SPLIT, no_lds_tables=_lib.OPT_GENERAL_NO_LDS_TABLES)


# ---- geometry arithmetic (no GPU) -------------------------------------------------------------------------------
def chunk_factor(m):
    """The small-code factor f of work_chunk (qbp_kernels.hpp)."""
    return 4 if m <= 36 else 2 if m <= 72 else 1


def work_chunk(B, total_slots, m, handed_out, by_cost):
    """work_chunk of bp_fused_kernel: indices a slot leader fetches when `handed_out` are gone."""
    rem = B - handed_out
    share = 8 if rem >= 16 * total_slots else 4 if rem >= 8 * total_slots else 2 if rem >= 4 * total_slots else 1
    ch = max(share, by_cost)
    f = chunk_factor(m)
    return 8 * f if (f > 1 and ch == 8 and rem >= 16 * f * total_slots) else ch


def simulate_chunks(B, total_slots, m, by_cost=1):
    """Chunk sizes handed out when every slot takes one syndrome per round (all syndromes cost the same) and the
    running-cost rule never asks for more than `by_cost`; and the indices handed out, with their multiplicity."""
    counter = 0
    seen = np.zeros(B, np.int64)
    seen[:min(B, total_slots)] += 1
    sizes = []
    nxt, end = [B] * total_slots, [B] * total_slots
    if B > total_slots:
        for s in range(total_slots):
            ch = work_chunk(B, total_slots, m, 9 * total_slots, 1)
            nxt[s], end[s] = total_slots + counter, total_slots + counter + ch
            counter += ch
            sizes.append(ch)
    busy = True
    while busy:
        busy = False
        for s in range(total_slots):
            if nxt[s] >= B:
                continue
            busy = True
            seen[nxt[s]] += 1
            nx = nxt[s] + 1
            if nx == end[s]:
                ch = work_chunk(B, total_slots, m, nx, by_cost)
                nx = total_slots + counter
                counter += ch
                end[s] = nx + ch
                sizes.append(ch)
            nxt[s] = nx
    return sizes, seen


def slot_values(m):
    """QBP_OPT_SLOTS_PER_BLOCK values of the tests: 1, 2, the largest, and one whose S * m is no multiple of 64."""
    smax = FUSED_MAX_THREADS // m
    odd = next(s for s in range(3, smax) if (s * m) % 64)
    return [1, 2, smax, odd]


def auto_slots(m, B, num_cu, forced, full_wg):
    """make_cfg's choice of slots per workgroup without QBP_OPT_SLOTS_PER_BLOCK (LDS limit apart)."""
    S = max(1, FUSED_MAX_THREADS // m)
    if not forced and not full_wg and (FUSED_MAX_THREADS // 2) // m >= 1 and S >= 2:
        S = (FUSED_MAX_THREADS // 2) // m
    return max(1, min(S, -(-B // num_cu)))


def expected_slots(m, B, num_cu, S_opt, forced=False, full_wg=False):
    S = S_opt if S_opt > 0 else auto_slots(m, B, num_cu, forced, full_wg)
    return max(1, min(S, FUSED_MAX_THREADS // m, B))


def threads_of(S, m):
    return min(FUSED_MAX_THREADS, 64 * (-(-S * m // 64)))


def auto_blocks_bound(S, m):
    """Upper bound of make_cfg's automatic workgroups per CU (twice the resident ones; LDS can only lower it)."""
    return 2 * max(1, (FUSED_MAX_THREADS // 64) // (threads_of(S, m) // 64))


def ragged_batch(m, num_cu, deep=False):
    """Batch of the S = 1, one-workgroup-per-CU geometry: 17 f (deep: 33 f) syndromes per slot plus a ragged tail."""
    return (33 if deep else 17) * chunk_factor(m) * num_cu + 13


def several_rounds_batch(S, blocks, m, num_cu):
    """A little above four syndromes per slot, odd remainder (blocks 0: for the automatic count's upper bound)."""
    per_cu = blocks if blocks > 0 else auto_blocks_bound(S, m)
    return 4 * num_cu * per_cu * S + 2 * S + 13


# ---- device buffers -----------------------------------------------------------------------------------------------
def torch():
    import torch as t
    return t


def to_device(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


def stream_ptr():
    return torch().cuda.current_stream().cuda_stream


@contextlib.contextmanager
def options(dec, **opts):
    """Set tuning options for the block and put every one of them back to 0 (auto) afterwards."""
    try:
        for k, v in opts.items():
            dec.set_option(OPTS[k], v)
        yield
    finally:
        for k in opts:
            dec.set_option(OPTS[k], 0)


class Outputs:
    """The four output tensors of a decode launch, rows + PAD rows each, poisoned before every launch."""

    def __init__(self, rows, n):
        t = torch()
        self.rows, self.n = rows, n
        R = rows + PAD
        self.t = dict(hard=t.empty((R, n), dtype=t.uint8, device="cuda"),
                      converged=t.empty(R, dtype=t.uint8, device="cuda"),
                      iters=t.empty(R, dtype=t.int32, device="cuda"),
                      llr=t.empty((R, n), dtype=t.float64, device="cuda"))

    def poison(self):
        self.t["hard"].fill_(0xFF)
        self.t["converged"].fill_(0xFF)
        self.t["iters"].fill_(-1)
        self.t["llr"].fill_(LLR_POISON)

    def poisoned(self, name, lo, hi=None):
        """Rows [lo, hi) of one output still hold nothing but the sentinel."""
        x = self.t[name][lo:hi]
        want = {"hard": 0xFF, "converged": 0xFF, "iters": -1, "llr": LLR_POISON}[name]
        return bool((x == want).all().item())

    def ptr(self, name, nulls=()):
        return 0 if name in nulls else self.t[name].data_ptr()

    def fetch(self, B, max_iter, what, nulls=()):
        """After the launch: sync, no sentinel in rows [0, B) of the outputs that were passed, nothing but sentinels
        behind them and in the outputs that were not passed.  Returns the numpy arrays (None for a null output)."""
        torch().cuda.synchronize()
        out = []
        for name in NAMES:
            if name in nulls:
                assert self.poisoned(name, 0), f"{what}: {name} was passed as null and has been written"
                out.append(None)
                continue
            assert self.poisoned(name, B), f"{what}: {name} written beyond row B = {B}"
            a = self.t[name][:B].cpu().numpy()
            if name in ("hard", "converged"):
                bad = a > 1
            elif name == "iters":
                bad = (a < 0) | (a >= max_iter)
            else:
                bad = a.view(np.uint64) == np.float64(LLR_POISON).view(np.uint64)
            if bad.any():
                rows = np.flatnonzero(bad.reshape(B, -1).any(axis=1))
                raise AssertionError(f"{what}: {len(rows)} of {B} syndromes never got their {name} (first {rows[:8]})")
            out.append(a.astype(bool) if name == "converged" else a)
        return tuple(out)


def launch(dec, syn_t, prior_t, B, out, max_iter=50, variant=0, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0,
           nulls=()):
    """Poison `out`, enqueue one qbp_decode_batch_device on the current torch stream (no sync)."""
    out.poison()
    dec.decode_device(syn_t.data_ptr(), prior_t.data_ptr(), B, max_iter, variant, alpha, damping, clip_llr, flags,
                      out.ptr("hard", nulls), out.ptr("converged", nulls), out.ptr("iters", nulls),
                      out.ptr("llr", nulls), stream_ptr())


def decode(dec, syn_t, prior_t, B, out, what, max_iter=50, nulls=(), **kw):
    launch(dec, syn_t, prior_t, B, out, max_iter=max_iter, nulls=nulls, **kw)
    return out.fetch(B, max_iter, what, nulls)


def assert_same(got, want, what):
    """Bit for bit; names the first differing syndrome."""
    for name, x, y in zip(NAMES, got, want):
        if x is None:
            continue
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        if name == "llr":
            if np.array_equal(x.view(np.uint64), y.view(np.uint64)):
                continue
            ok = golden_util.same_bits(x, y)                # (any NaN equals any NaN)
            if ok.all():
                continue
        else:
            if np.array_equal(x, y):
                continue
            ok = x == y
        rows = np.flatnonzero(~ok.reshape(len(x), -1).all(axis=1))
        raise AssertionError(f"{what}: {name} differs on {len(rows)} of {len(x)} syndromes, first index {rows[0]} "
                             f"(then {rows[1:8]})")


def syndromes_of(H, errors):
    """H e mod 2 as uint8 (float32 BLAS product: exact, the row weights are far below 2^24)."""
    return ((errors.astype(np.float32) @ np.asarray(H).T.astype(np.float32)) % 2).astype(np.uint8)
