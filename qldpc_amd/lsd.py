"""Localized statistics decoding (BP+LSD; Hillmann et al. 2024) on the GPU: clusters grow around the checks BP leaves
unsatisfied, in the order of BP's reliabilities, and only the small systems inside the clusters are solved
(include/qbp.h, ``qbp_lsd_batch``, states the rules).  A drop-in alternative to OSD-0, with its inputs:

    solution = performLSD(H, syndrome, llr, hard, bits_per_step=1)

``bits_per_step``: the variables an invalid cluster activates per round (0: all of its neighbours).  The ``lsd=``
argument of ``mc.run_sweep``, ``mc.run_dem`` and ``mc.run_weights`` sends the trials the first-stage BP leaves
unconverged through LSD instead of OSD.  ``large``: False -- the kernel that keeps a record's rows in LDS, which refuses
matrices beyond 160 KiB or 2048 rows; True -- beyond those the build with the rows in a global workspace
(QBP_OPT_LSD_MEM = 2); "force" -- that build always.  The output does not depend on it.
"""
from __future__ import annotations

import numpy as np

_INT32_MAX = int(np.iinfo(np.int32).max)


def check_bits_per_step(value):
    """``bits_per_step`` as an int, validated as qbp_lsd_configure does (ValueError where it answers QBP_E_INVALID)."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= _INT32_MAX:
        raise ValueError(f"bits_per_step must be an integer >= 0, got {value!r}")
    return int(value)


def performLSDBatch(H, syndromes, llr, hard, bits_per_step=1, device=None, large=False):
    """LSD of B records on the GPU: syndromes uint8[B, m], BP's posteriors float64[B, n] and hard decisions uint8[B, n]
    -> ``(solutions int8[B, n], stats int32[B, 4])``, stats = rounds, active variables, clusters, valid."""
    from . import bp
    g = check_bits_per_step(bits_per_step)
    H = np.asarray(H)
    if H.ndim != 2:
        raise ValueError(f"H must be a matrix, got shape {H.shape}")
    m, n = H.shape
    syn = np.asarray(syndromes)
    l = np.asarray(llr)
    hd = np.asarray(hard)
    if syn.ndim != 2 or syn.shape[1] != m:
        raise ValueError(f"syndromes must have shape (B, {m}), got {syn.shape}")
    if l.shape != (syn.shape[0], n) or hd.shape != l.shape:
        raise ValueError(f"llr and hard must have shape ({syn.shape[0]}, {n}), got {l.shape} and {hd.shape}")
    dec = bp.decoder_for(H, device=bp.DEVICE if device is None else device)
    sol, stats = dec.lsd(syn, l, hd, g, large=large)
    return sol.astype(np.int8), stats


def performLSD(H, syndrome, llr, hard, bits_per_step=1, device=None, large=False):
    """LSD of one record, in the shape of the reference's ``performOSD``: -> solution int8[n]."""
    syn, l, hd = np.asarray(syndrome), np.asarray(llr), np.asarray(hard)
    if syn.ndim != 1 or l.ndim != 1 or hd.ndim != 1:
        raise ValueError("syndrome, llr and hard must be vectors")
    return performLSDBatch(H, syn[None, :], l[None, :], hd[None, :], bits_per_step, device, large)[0][0]
