"""Fixed-point min-sum BP on the GPU (include/qbp.h, ``qbp_quant_configure``, states the rules): messages of ``bits``
bits with saturating integer arithmetic, the decoder an FPGA or ASIC runs.  What logical error rate is left at q bits,
at this scale, with this normalisation?

    cfg = QuantConfig(bits=6, scale=2.0, alpha=(13, 4), beta=0)          # alpha = 13 / 2^4
    hard, converged, values, iterations = performQuantMinSum(H, syndrome, prior, cfg, maxIter=50)

``values`` are the integer posteriors as doubles, in units of 1 / scale.  ``quant=cfg`` on ``mc.run_sweep``,
``mc.run_dem``, ``mc.run_weights`` and ``mc.run_weights_matrix`` selects the same decoder as the first stage there (OSD,
Relay-BP, BPGD and LSD act on what it leaves unconverged).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass(frozen=True)
class QuantConfig:
    """``bits`` q in [2, 16], M = 2^(q-1) - 1; ``scale`` > 0, integer units per unit of LLR; ``alpha`` = (num, shift),
    the normalisation num / 2^shift with 0 <= shift <= 15 and 1 <= num <= 2^shift; ``beta`` in [0, M], the offset."""
    bits: int
    scale: float
    alpha: tuple = (1, 0)
    beta: int = 0

    def __post_init__(self):
        def integer(x):
            return not isinstance(x, bool) and isinstance(x, (int, np.integer))
        if not integer(self.bits) or not 2 <= self.bits <= 16:
            raise ValueError(f"bits must be an integer in [2, 16], got {self.bits!r}")
        try:
            scale = float(self.scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a number, got {self.scale!r}") from None
        if not math.isfinite(scale) or not scale > 0.0:
            raise ValueError(f"scale must be finite and > 0, got {self.scale!r}")
        try:
            num, shift = self.alpha
        except (TypeError, ValueError):
            raise ValueError(f"alpha must be (num, shift), got {self.alpha!r}") from None
        if not integer(shift) or not 0 <= shift <= 15:
            raise ValueError(f"alpha shift must be an integer in [0, 15], got {shift!r}")
        if not integer(num) or not 1 <= num <= (1 << shift):
            raise ValueError(f"alpha num must be an integer in [1, 2^{shift}], got {num!r}")
        if not integer(self.beta) or not 0 <= self.beta <= self.M:
            raise ValueError(f"beta must be an integer in [0, {self.M}], got {self.beta!r}")
        object.__setattr__(self, "bits", int(self.bits))
        object.__setattr__(self, "scale", scale)
        object.__setattr__(self, "alpha", (int(num), int(shift)))
        object.__setattr__(self, "beta", int(self.beta))

    @property
    def M(self) -> int:
        return (1 << (int(self.bits) - 1)) - 1


def as_config(quant) -> QuantConfig:
    """A ``QuantConfig``, or its dict form ``{"bits":, "scale":, "alpha":, "beta":}``."""
    if isinstance(quant, QuantConfig):
        return quant
    if isinstance(quant, dict):
        return QuantConfig(**quant)
    raise ValueError(f"quant must be a QuantConfig or its dict form, got {quant!r}")


def lds_bytes(m, n, E, slots, wide) -> int:
    """Dynamic LDS of one workgroup of bp_quant_kernel with ``slots`` records (what QBP_INFO_LDS_BYTES reports after a
    launch): the quantised prior and, per record, the posterior as int32 [n], the E messages of 1 byte (``wide`` False:
    bits <= 8) or 2, rounded up to a word, and the bookkeeping words."""
    slot_words = (10 + (int(m) + 31) // 32 + 1) & ~1
    msg_words = (int(E) * (2 if wide else 1) + 3) // 4
    state_words = (int(n) + int(slots) * (int(n) + msg_words) + 1) & ~1          # (the words behind hold 64-bit cells)
    return 4 * (state_words + 32 + int(slots) * slot_words)


def quantize_prior(prior, cfg) -> np.ndarray:
    """Rule 1 in numpy: int32 P, 0 where the prior is NaN, else clamp(rint(prior * scale), -M, M) -- one IEEE double
    multiply, rint rounds half to even, +-inf clamps to +-M."""
    cfg = as_config(cfg)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(prior, np.float64) * np.float64(cfg.scale)
        r = np.clip(np.rint(x), -float(cfg.M), float(cfg.M))
    return np.where(np.isnan(x), 0.0, r).astype(np.int32)


def performQuantMinSumBatch(H, syndromes, initialBelief, cfg, maxIter=50, force_full=False, device=None):
    """Fixed-point min-sum of B syndromes uint8[B, m] -> ``(hard uint8[B, n], converged bool[B], iters int32[B],
    llr float64[B, n], posterior_q int32[B, n])``; llr is posterior_q as doubles, in units of 1 / scale."""
    from . import bp
    cfg = as_config(cfg)
    prior = np.ascontiguousarray(initialBelief, np.float64)
    if np.any(np.isnan(prior)):
        raise ValueError("the prior must not hold a NaN (+-inf are legal)")
    dec = bp.decoder_for(H, device=bp.DEVICE if device is None else device)
    with dec._lock:                      # (the configuration and the decode of one call belong together)
        dec.quant_configure(cfg)
        hard, conv, iters, post, llr = dec.quant_decode(syndromes, prior, maxIter,
                                                        _lib.FLAG_FORCE_FULL if force_full else 0)
    return hard, conv, iters, llr, post


def performQuantMinSum(H, syndrome, initialBelief, cfg, maxIter=50, device=None):
    """Fixed-point min-sum of one syndrome, in the shape of rework/decoding.py's decoders: ``(candidateError, converged,
    values, iterations)``."""
    hard, conv, iters, llr, _ = performQuantMinSumBatch(H, np.asarray(syndrome).reshape(1, -1), initialBelief, cfg,
                                                        maxIter, device=device)
    return hard[0].astype(np.int8), bool(conv[0]), llr[0], int(iters[0])
