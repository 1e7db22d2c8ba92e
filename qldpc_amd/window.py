"""Sliding-window decoding of multi-round matrices (include/qbp.h, qbp_window_*): windows of W rounds are decoded one
after another on the GPU, each commits its first F rounds, and the committed correction is folded into the syndrome of
the later rounds.  The caller says which round every check belongs to (``check_round``)."""
import numpy as np

from . import _lib, bp


def phenomenological_rounds(code, rounds):
    """``check_round`` of ``dem.phenomenological(code, rounds, ...)``: check c of the space-time matrix is check
    c % m0 of round c // m0, m0 the checks of the code."""
    from . import codes
    c = codes.load_code(code) if isinstance(code, str) else code
    m0 = int(np.asarray(c.Hx).shape[0])
    return (np.arange(m0 * int(rounds)) // m0).astype(np.int32)


def window_plan(H, check_round, W, F):
    """Host-only: the windows of H (``_lib.window_plan`` of its CSR form)."""
    return _lib.window_plan(*bp.csr_from_H(H), check_round, W, F)


def decoder_for(H, check_round, W, F, device=None) -> _lib.WindowDecoder:
    """A new ``_lib.WindowDecoder`` of H (keep it: it owns a decoder per window class and its workspaces)."""
    return _lib.WindowDecoder(*bp.csr_from_H(H), check_round, W, F, bp.DEVICE if device is None else device)


def performWindowBP(H, check_round, syndromes, prior, W, F, maxIter=50, osd=False, osd_method="cs", osd_order=0,
                    osd_large=False, variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, decoder=None):
    """Window-decode ``syndromes`` [B, m] (or one syndrome [m]) -> (correction, converged, iters, llr, window_fails).
    ``osd``: OSD on the windows BP does not converge on (``osd_order`` 0: OSD-0; else order-w by ``osd_method``).
    ``decoder``: a ``decoder_for(H, check_round, W, F)`` to reuse."""
    flags = _lib.osd_flags(osd_method, osd_order, osd_large) if osd else 0
    syn = np.asarray(syndromes, np.uint8)
    one = syn.ndim == 1
    dec = decoder_for(H, check_round, W, F) if decoder is None else decoder
    out = dec.decode(syn[None, :] if one else syn, prior, maxIter, variant, alpha, damping, clip_llr, flags)
    return tuple(a[0] for a in out) if one else out
