"""BP guided decimation (BPGD) on the GPU: flooding BP in rounds of a few iterations; a round that ends without a
solution freezes the most reliable variable at +-``decim_llr`` and the next round continues on the same messages
(include/qbp.h, ``qbp_gd_decode_batch``, states the rules).  No elimination and no tables: the third way, next to OSD and
Relay-BP, to decode what BP leaves unconverged.

    hard, converged, llr, iters = performBPGD(H, syndrome, prior, iters_per_round=8, max_rounds=H.shape[1])

``GDConfig`` is the same configuration as an object, for the ``gd=`` argument of ``mc.run_sweep``, ``mc.run_dem`` and
``mc.run_weights`` (trials the first-stage BP leaves unconverged go to BPGD instead of OSD).

``large``: where a record's messages live.  False (default): in LDS, and a matrix whose record state passes 160 KiB
(about 40 rounds of the [[72,12,6]] phenomenological matrix, 2592 x 7776) is refused; True: always in a per-workgroup
global workspace; "auto": in LDS where they fit, else in the workspace (the space-time and detector-error-model
matrices).  The outputs do not depend on it.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib

SUM_PRODUCT, MIN_SUM = 0, 2
GDResult = namedtuple("GDResult", "hard converged iters llr rounds")
_INT32_MAX = int(np.iinfo(np.int32).max)


def _integer(name, value, lo):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= _INT32_MAX:
        raise ValueError(f"{name} must be an integer >= {lo}, got {value!r}")
    return int(value)


class GDConfig:
    """iters_per_round, max_rounds, decim_llr, variant, alpha, clip_llr -- validated as qbp_gd_configure does (ValueError
    where the library answers QBP_E_INVALID) --, and ``large`` (False, True or "auto": QBP_OPT_GD_MEM 0, 1 or 2)."""

    def __init__(self, iters_per_round=8, max_rounds=0, decim_llr=25.0, variant=MIN_SUM, alpha=1.0, clip_llr=20.0,
                 large=False):
        _lib.msg_mem_value("gd", large)
        self.large = large
        self.iters_per_round = _integer("iters_per_round", iters_per_round, 1)
        self.max_rounds = _integer("max_rounds", max_rounds, 0)
        if isinstance(variant, (bool, np.bool_)) or variant not in (SUM_PRODUCT, MIN_SUM):
            raise ValueError(f"variant must be sum-product (0) or min-sum (2), got {variant!r}")
        self.variant = int(variant)
        try:
            self.decim_llr, self.alpha, self.clip_llr = float(decim_llr), float(alpha), float(clip_llr)
        except (TypeError, ValueError):
            raise ValueError("decim_llr, alpha and clip_llr must be numbers") from None
        if not (np.isfinite(self.decim_llr) and self.decim_llr > 0.0):
            raise ValueError(f"decim_llr must be > 0 and finite, got {decim_llr!r}")
        if not np.isfinite(self.alpha) or not np.isfinite(self.clip_llr):
            raise ValueError("alpha and clip_llr must be finite")


def as_config(gd):
    """The ``gd=`` argument of the Monte-Carlo drivers as a ``GDConfig``: a ``GDConfig``, or a dict of its arguments."""
    if isinstance(gd, GDConfig):
        return gd
    if isinstance(gd, dict):
        unknown = sorted(set(gd) - {"iters_per_round", "max_rounds", "decim_llr", "variant", "alpha", "clip_llr",
                                    "large"})
        if unknown:
            raise ValueError(f"unknown gd settings: {unknown}")
        return GDConfig(**gd)
    raise ValueError(f"gd must be a GDConfig or a dict, got {type(gd).__name__}")


def performBPGDBatch(H, syndromes, prior, iters_per_round=8, max_rounds=0, decim_llr=25.0, variant=MIN_SUM, alpha=1.0,
                     clip_llr=20.0, device=None, large=False):
    """BPGD of B syndromes uint8[B, m] on the GPU -> ``GDResult(hard uint8[B, n], converged bool[B], iters int32[B],
    llr float64[B, n], rounds int32[B])``.  ``large``: as in ``GDConfig``."""
    from . import bp
    cfg = GDConfig(iters_per_round, max_rounds, decim_llr, variant, alpha, clip_llr, large)
    dec = bp.decoder_for(H, device=bp.DEVICE if device is None else device)
    return GDResult(*dec.gd_decode(syndromes, prior, cfg))


def performBPGD(H, syndrome, initialBelief, iters_per_round=8, max_rounds=0, decim_llr=25.0, variant=MIN_SUM, alpha=1.0,
                clip_llr=20.0, device=None, large=False):
    """BPGD of one syndrome, in the shape of the reference's decoders: ``(candidateError, converged, values,
    iterations)`` -- iterations executed over all rounds."""
    r = performBPGDBatch(H, np.asarray(syndrome).reshape(1, -1), initialBelief, iters_per_round, max_rounds, decim_llr,
                         variant, alpha, clip_llr, device, large)
    return r.hard[0], bool(r.converged[0]), r.llr[0], int(r.iters[0])
