"""Exhaustive enumeration of the errors of one weight (qbp_mc_run_enum, qbp_enum_failures; include/qbp.h).

The order: for n columns and weight w, rank r in [0, C(n, w)) is the r-th tuple of
``itertools.combinations(range(n), w)`` -- lexicographic order of the ascending column tuple.  ``unrank``, ``rank``
and ``patterns`` are the numpy / Python-int statement of that order for ranks of any size; the device follows the same
rule for classes of up to 2^62 patterns.  ``failing_patterns`` decodes a whole class on the GPU and returns the
patterns the decoder gets wrong -- each one an int64 rank."""
import math

import numpy as np

MAX_COUNT = 1 << 62         # the largest class the library enumerates (qbp_enum_count)

WHAT = {"logical": 1, "unconverged": 2, "either": 3}


def count(n, w):
    """C(n, w), the patterns of weight w on n columns.  ValueError where the library refuses to enumerate: w outside
    [0, n] or more than 2^62 patterns."""
    n, w = int(n), int(w)
    if n < 0 or not 0 <= w <= n:
        raise ValueError(f"weight = {w} out of [0, {n}] (n columns)")
    c = math.comb(n, w)
    if c > MAX_COUNT:
        raise ValueError(f"C({n}, {w}) = {c} patterns are beyond 2^62")
    return c


def _unrank_one(n, w, r):
    """Columns of rank r: for i = 0 .. w - 1 the smallest column c >= lo whose block of C(n - 1 - c, w - 1 - i)
    patterns holds the remaining rank."""
    cols, lo = [], 0
    for i in range(w):
        c = lo
        while True:
            block = math.comb(n - 1 - c, w - 1 - i)
            if r < block:
                break
            r -= block
            c += 1
        cols.append(c)
        lo = c + 1
    return cols


def unrank(n, w, ranks):
    """int64[len(ranks), w]: the ascending columns of every rank (Python ints of any size)."""
    n, w = int(n), int(w)
    total = math.comb(n, w) if 0 <= w <= n else 0
    out = np.zeros((len(ranks), w), np.int64)
    for k, r in enumerate(ranks):
        r = int(r)
        if not 0 <= r < total:
            raise ValueError(f"rank {r} out of [0, C({n}, {w}) = {total})")
        out[k] = _unrank_one(n, w, r)
    return out


def rank(n, w, cols):
    """The ranks (a list of Python ints) of ascending column tuples ``cols`` [len, w]."""
    n, w = int(n), int(w)
    cols = np.asarray(cols, np.int64)
    cols = cols.reshape(len(cols), w) if w == 0 else cols.reshape(-1, w)
    out = []
    for row in cols:
        row = [int(c) for c in row]
        if any(not 0 <= c < n for c in row) or any(a >= b for a, b in zip(row, row[1:])):
            raise ValueError(f"columns must ascend strictly within [0, {n}), got {row}")
        r, lo = 0, 0
        for i, c in enumerate(row):
            # every tuple with a smaller column in place i comes first (hockey stick over lo .. c - 1)
            r += math.comb(n - lo, w - i) - math.comb(n - c, w - i)
            lo = c + 1
        out.append(r)
    return out


def patterns(n, w, ranks):
    """uint8[len(ranks), n]: the error rows of the ranks."""
    cols = unrank(n, w, ranks)
    out = np.zeros((len(cols), int(n)), np.uint8)
    if w:
        out[np.arange(len(cols))[:, None], cols] = 1
    return out


def failing_patterns(H, L, w, *, prior, what="logical", cap=1 << 20, rank_begin=0, rank_end=None, max_iter=50,
                     variant=0, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0,
                     osd_large=False, device=0):
    """Decode every weight-w pattern of H [m, n] (ranks [rank_begin, rank_end), by default the whole class) on the GPU
    and return those the decoder fails on: ``what`` = "logical" (L x != L e), "unconverged" (BP did not converge) or
    "either".  BP with ``prior`` [n], then OSD where BP did not converge if ``osd``.  Returns a dict: ``ranks``
    int64[F], ``kinds`` uint8[F] (bit 0 logical, bit 1 unconverged), ``columns`` int64[F, w], ``found`` (may exceed
    ``cap``; F = min(found, cap)) and ``counters`` int64[12] as ``Decoder.decode_shots`` counts."""
    from . import bp, mc
    if what not in WHAT:
        raise ValueError(f"what must be one of {sorted(WHAT)}, got {what!r}")
    flags = mc.osd_run_flags(osd, osd_method, osd_order, osd_large)
    H = np.asarray(H)
    n = H.shape[1]
    total = count(n, w)
    end = total if rank_end is None else int(rank_end)
    dec = bp.decoder_for(H, device=device)
    ranks, kinds, found, counters = dec.enum_failures(L, w, prior, rank_begin, end, what=WHAT[what], cap=cap,
                                                      max_iter=max_iter, variant=variant, alpha=alpha, damping=damping,
                                                      clip_llr=clip_llr, flags=flags)
    return dict(ranks=ranks, kinds=kinds, columns=unrank(n, w, ranks), found=found, counters=counters)
