"""Relay-BP on the GPU: min-sum with a memory strength per variable, run as a chain of legs (include/qbp.h,
``qbp_relay_decode_batch``, states the rules).  The alternative to BP + OSD: no elimination, a few hundred min-sum
iterations per syndrome, the lightest of the first few solutions.

    gammas = relay_gammas(n, legs=10, gamma0=0.125, interval=(-0.24, 0.66), seed=0)
    hard, converged, llr, iters = performRelayBP(H, syndrome, prior, gammas, [30] * 10, stop_after=3)

``RelayConfig`` is the same configuration as an object, for the ``relay=`` argument of ``mc.run_sweep``, ``mc.run_dem``
and ``mc.run_weights`` (trials the first-stage BP leaves unconverged go to Relay-BP instead of OSD).

``large``: where a record's messages live.  False (default): in LDS, and a matrix whose record state passes 160 KiB
(34 rounds of the [[72,12,6]] phenomenological matrix, 2592 x 7776) is refused; True: in LDS where they fit, else in a
per-workgroup global workspace (the space-time and detector-error-model matrices); "force": the workspace always (tests).
The outputs do not depend on it.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib

RelayResult = namedtuple("RelayResult", "hard converged iters llr legs solutions")


def relay_gammas(n, legs, gamma0, interval, seed=0):
    """Memory strengths float64[legs, n]: leg 0 is uniform ``gamma0``; every later leg draws its n strengths uniformly
    from ``interval`` = (lo, hi) with ``np.random.default_rng(seed)``, leg by leg."""
    n, legs = int(n), int(legs)
    lo, hi = (float(x) for x in interval)
    if n < 1 or legs < 1:
        raise ValueError(f"relay_gammas needs n >= 1 and legs >= 1, got n = {n}, legs = {legs}")
    if not (np.isfinite(gamma0) and np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"gamma0 and interval must be finite with lo <= hi, got {gamma0!r}, {interval!r}")
    rng = np.random.default_rng(seed)
    g = np.empty((legs, n), np.float64)
    g[0] = float(gamma0)
    for leg in range(1, legs):
        g[leg] = rng.uniform(lo, hi, n)
    return g


class RelayConfig:
    """gammas float64[L, n], leg_iters int32[L], stop_after, alpha, clip_llr -- validated as qbp_relay_configure does
    (ValueError where the library answers QBP_E_INVALID) --, and ``large`` (False, True or "force": QBP_OPT_RELAY_MEM 0,
    2 or 1)."""

    def __init__(self, gammas, leg_iters, stop_after=1, alpha=1.0, clip_llr=20.0, large=False):
        g = np.ascontiguousarray(gammas, np.float64)
        it = np.asarray(leg_iters)
        if g.ndim != 2 or g.shape[0] < 1 or g.shape[1] < 1:
            raise ValueError(f"gammas must have shape (legs, n), got {g.shape}")
        if it.ndim != 1 or it.dtype.kind not in "iu" or it.shape[0] != g.shape[0]:
            raise ValueError(f"leg_iters must be {g.shape[0]} integers (one per leg), got {leg_iters!r}")
        if np.any(it < 1) or np.any(it > np.iinfo(np.int32).max):
            raise ValueError(f"every leg needs at least one iteration, got {leg_iters!r}")
        if isinstance(stop_after, bool) or int(stop_after) != stop_after or int(stop_after) < 1:
            raise ValueError(f"stop_after must be an integer >= 1, got {stop_after!r}")
        if not np.all(np.isfinite(g)) or not np.isfinite(alpha) or not np.isfinite(clip_llr):
            raise ValueError("gammas, alpha and clip_llr must be finite")
        _lib.msg_mem_value("relay", large)
        self.large = large
        self.gammas = g
        self.leg_iters = np.ascontiguousarray(it, np.int32)
        self.stop_after, self.alpha, self.clip_llr = int(stop_after), float(alpha), float(clip_llr)

    @property
    def n(self):
        return self.gammas.shape[1]

    def as_dict(self):
        """The dict form ``as_config`` reads back."""
        return dict(gammas=self.gammas, leg_iters=self.leg_iters, stop_after=self.stop_after, alpha=self.alpha,
                    clip_llr=self.clip_llr, large=self.large)


def as_config(relay, n):
    """The ``relay=`` argument of the Monte-Carlo drivers as a ``RelayConfig`` for n variables.  A ``RelayConfig``, or a
    dict: either ``gammas`` and ``leg_iters`` (as ``performRelayBP``), or ``legs``, ``iters`` (per leg), ``gamma0``,
    ``interval`` and optionally ``seed`` (``relay_gammas``); both forms take ``stop_after``, ``alpha``, ``clip_llr``
    and ``large``."""
    if isinstance(relay, RelayConfig):
        cfg = relay
    elif isinstance(relay, dict):
        d = dict(relay)
        rest = {k: d.pop(k) for k in ("stop_after", "alpha", "clip_llr", "large") if k in d}
        if "gammas" in d:
            gammas, leg_iters = d.pop("gammas"), d.pop("leg_iters")
        else:
            legs = int(d.pop("legs"))
            gammas = relay_gammas(n, legs, d.pop("gamma0"), d.pop("interval"), d.pop("seed", 0))
            leg_iters = [int(d.pop("iters"))] * legs
        if d:
            raise ValueError(f"unknown relay settings: {sorted(d)}")
        cfg = RelayConfig(gammas, leg_iters, **rest)
    else:
        raise ValueError(f"relay must be a RelayConfig or a dict, got {type(relay).__name__}")
    if cfg.n != int(n):
        raise ValueError(f"the relay configuration is for {cfg.n} variables, the matrix has {n}")
    return cfg


def performRelayBPBatch(H, syndromes, prior, gammas, leg_iters, stop_after=1, alpha=1.0, clip_llr=20.0, device=None,
                        large=False):
    """Relay-BP of B syndromes uint8[B, m] on the GPU -> ``RelayResult(hard uint8[B, n], converged bool[B],
    iters int32[B], llr float64[B, n], legs int32[B], solutions int32[B])``.  ``large``: as in ``RelayConfig``."""
    from . import bp
    cfg = RelayConfig(gammas, leg_iters, stop_after, alpha, clip_llr, large)
    dec = bp.decoder_for(H, device=bp.DEVICE if device is None else device)
    return RelayResult(*dec.relay_decode(syndromes, prior, cfg))


def performRelayBP(H, syndrome, prior, gammas, leg_iters, stop_after=1, alpha=1.0, clip_llr=20.0, device=None,
                   large=False):
    """Relay-BP of one syndrome, in the shape of the reference's decoders: ``(candidateError, converged, values,
    iterations)`` -- iterations executed over all legs."""
    r = performRelayBPBatch(H, np.asarray(syndrome).reshape(1, -1), prior, gammas, leg_iters, stop_after, alpha,
                            clip_llr, device, large)
    return r.hard[0], bool(r.converged[0]), r.llr[0], int(r.iters[0])
