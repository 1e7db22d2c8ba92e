"""Two-stage decoding of a CSS code under Pauli noise: decode the sector Hx detects with its marginal prior, then
the sector Hz detects with a prior conditioned, qubit by qubit and record by record, on what the first stage found
(include/qbp.h, qbp_css_*, states the rule; the second stage is ``qbp_decode_batch_cond``, BP with a prior per
record).

    prior_a, prior_b0, prior_b1 = pauli_priors(p / 3, p / 3, p / 3, code.n)       # depolarizing noise of strength p
    dec = CssDecoder(code.Hx, code.Hz)
    x_a, x_b, conv_a, conv_b = dec.decode(syn_a, syn_b, prior_a, prior_b0, prior_b1, osd=True)

Sector A holds the errors Hx detects (Z and Y), sector B those Hz detects (X and Y)."""
from __future__ import annotations

import math

import numpy as np

from . import _lib, bp


def pauli_priors(px, py, pz, n):
    """-> (prior_a, prior_b0, prior_b1), float64[n] each, for independent Pauli noise (px, py, pz) per qubit.

    prior_a  = log((1 - py - pz) / (py + pz))    the marginal of sector A: the qubit has Z or Y;
    prior_b0 = log((1 - px - py - pz) / px)      sector B (X or Y) given that sector A has no error there;
    prior_b1 = log(pz / py)                      ... given that it has one.
    Depolarizing noise of strength p, px = py = pz = p / 3: prior_b1 = 0 exactly, prior_b0 = log(3 (1 - p) / p).
    A zero denominator gives +inf, a zero numerator -inf; 0 / 0 is a ValueError."""
    px, py, pz = float(px), float(py), float(pz)
    if min(px, py, pz) < 0.0 or px + py + pz > 1.0:
        raise ValueError(f"Pauli probabilities ({px}, {py}, {pz}) must be >= 0 and sum to at most 1")

    def llr(num, den):
        if num == 0.0 and den == 0.0:
            raise ValueError(f"Pauli probabilities ({px}, {py}, {pz}) leave a conditional prior undefined (0 / 0)")
        if den == 0.0:
            return math.inf
        return -math.inf if num == 0.0 else math.log(num / den)
    n = int(n)
    return (np.full(n, llr(1.0 - py - pz, py + pz)), np.full(n, llr(1.0 - px - py - pz, px)),
            np.full(n, 0.0 if py == pz else llr(pz, py)))


def marginal_prior_b(px, py, pz, n):
    """log((1 - px - py) / (px + py)): the prior of sector B decoded on its own (the independent baseline)."""
    return pauli_priors(pz, py, px, n)[0]


def performBeliefPropagationCond(H, syndromes, sel, prior0, prior1, maxIter=50, variant=_lib.SUM_PRODUCT, alpha=1.0,
                                 clip_llr=20.0):
    """BP on every row of ``syndromes`` with the prior ``np.where(sel[b] & 1, prior1, prior0)`` of its own ->
    (hard uint8[B, n], converged bool[B], iters int32[B], llr float64[B, n]), as ``bp.performBeliefPropagationBatch``
    would give row by row with that prior."""
    return bp.decoder_for(H).decode_cond(np.atleast_2d(syndromes), np.atleast_2d(sel), prior0, prior1, maxIter, variant,
                                         alpha, clip_llr)


class CssDecoder(_lib.CssDecoder):
    """The two-stage decoder of the CSS code (Hx, Hz) on one GPU."""

    def __init__(self, Hx, Hz, device=None):
        super().__init__(bp.decoder_for(Hx, device=device), bp.decoder_for(Hz, device=device))

    def decode(self, syn_a, syn_b, prior_a, prior_b0, prior_b1, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0,
               damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, flags=0):
        """-> (x_a, x_b, conv_a, conv_b): the corrections of both sectors and the BP stages' converged flags.
        ``osd``: the records a stage's BP leaves unconverged go through OSD (order 0, or ``osd_method`` / ``osd_order``)."""
        if osd:
            flags = int(flags) | _lib.osd_flags(osd_method, osd_order)
        return super().decode(syn_a, syn_b, prior_a, prior_b0, prior_b1, max_iter, variant, alpha, damping, clip_llr,
                              flags)
