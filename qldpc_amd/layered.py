"""Layered (check-serial) BP on the GPU (include/qbp.h, ``qbp_layered_configure``, states the rules): the checks are
visited one after another in a fixed order and each sees the posteriors its predecessors of the same iteration just
updated.  On the degenerate Tanner graphs of the BB codes this is the standard way to break the symmetric trapping
sets the flooding schedule oscillates on.

    order, levels = layered_order(H)
    hard, converged, llr, iters = performLayeredBP(H, syndrome, prior, maxIter=50, variant="min-sum", order=order)

``layered=True`` on ``Decoder.decode``, ``mc.run_sweep``, ``mc.run_dem`` and ``mc.run_weights`` selects the same decoder
there (OSD and Relay-BP act on what it leaves unconverged).

``large``: where a record's messages live.  False (default): in LDS, and a matrix whose single-slot state passes
160 KiB (40 rounds of the [[72,12,6]] phenomenological matrix, 2592 x 7776) is refused; True: in LDS where they fit,
else in a per-workgroup global workspace (the space-time and detector-error-model matrices, n up to about 20 000).
``layered="large"`` is the same choice on the Monte-Carlo drivers.  The outputs do not depend on it.
"""
from __future__ import annotations

import numpy as np

from . import _lib

VARIANTS = {"sum-product": _lib.SUM_PRODUCT, "min-sum": _lib.MIN_SUM}


def _variant(variant):
    if variant in VARIANTS:
        return VARIANTS[variant]
    if variant in (_lib.SUM_PRODUCT, _lib.MIN_SUM) and not isinstance(variant, bool):
        return int(variant)
    raise ValueError(f"layered BP runs 'sum-product' or 'min-sum', got {variant!r}")


def layered_order(H, order=None):
    """The layered schedule of H (host only, qbp_layered_plan) -> ``(order int32[m], levels)``: the checks level after
    level, and the levels as a list of arrays -- checks of one level share no variable and are updated at once.
    ``order`` None: the default order, greedy colouring by ascending index, ordered by (colour, index); else a
    permutation of the checks, returned sorted by level (the same schedule)."""
    from . import bp
    row_ptr, col_idx, m, n = bp.csr_from_H(H)
    out, lptr = _lib.layered_plan(row_ptr, col_idx, m, n, order)
    return out, [out[lptr[i]:lptr[i + 1]].copy() for i in range(len(lptr) - 1)]


def performLayeredBPBatch(H, syndromes, initialBelief, maxIter=50, variant="sum-product", alpha=1.0, clip_llr=20.0,
                          order=None, device=None, large=False):
    """Layered BP of B syndromes uint8[B, m] -> ``(hard uint8[B, n], converged bool[B], iters int32[B],
    llr float64[B, n])``.  ``large``: see the module's text."""
    _lib.msg_mem_value("layered", large)
    from . import bp
    v = _variant(variant)
    prior = np.ascontiguousarray(initialBelief, np.float64)
    if not np.all(np.isfinite(prior)):
        raise ValueError("layered BP needs a finite prior")
    dec = bp.decoder_for(H, device=bp.DEVICE if device is None else device)
    with dec._lock:                      # (the order and the decode of one call belong together)
        dec.layered_configure(order, large)
        return dec.decode(syndromes, prior, maxIter, v, alpha, 1.0, clip_llr, layered=True)


def performLayeredBP(H, syndrome, initialBelief, maxIter=50, variant="sum-product", alpha=1.0, clip_llr=20.0,
                     order=None, device=None, large=False):
    """Layered BP of one syndrome, in the shape of rework/decoding.py's decoders: ``(candidateError, converged,
    values, iterations)``."""
    hard, conv, iters, llr = performLayeredBPBatch(H, np.asarray(syndrome).reshape(1, -1), initialBelief, maxIter,
                                                   variant, alpha, clip_llr, order, device, large)
    return hard[0].astype(np.int8), bool(conv[0]), llr[0], int(iters[0])
