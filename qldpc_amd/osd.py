"""Mirror of ``decoding/OSD.py``: ``performOSD(H, syndrome, llr, hard)`` (OSD-0), on the GPU.

Same positional signature and return type (int64 vector, ``(hard + e_correction) % 2``,
OSD.py:26-28).  Equal ``|llr|`` values are ordered by column index (the reference's ``np.argsort``
leaves that order to the numpy build).

A syndrome outside the column space of H (none of the reference's callers passes one) gets the reference's
output as well: there it depends on the row swaps of the elimination, which a second kernel follows
(qbp_osd.hpp, osd_flag_inconsistent; tests/golden/osd_inconsistent.npz).

``performOSD_enhanced`` (decoding/OSD_enhanced.py:5 = rework/decoding.py:193) returns its OSD-0
solution whenever that solution reproduces the syndrome (OSD_enhanced.py "if np.all(osd0_syndrome
== syndrome): return osd0_solution", before any higher-order search) -- which is the case for every
syndrome in the column space of H, i.e. every syndrome that comes from an error.  The mirror below
therefore is OSD-0 on the GPU for every ``order``; only an INCONSISTENT syndrome with ``order > 0``
would reach the reference's combinatorial search, which is not implemented here.

A real higher-order OSD -- the OSD-0 solution, then a search over flip sets of the least reliable non-pivot
columns (combination sweep "cs" or exhaustive "e", include/qbp.h qbp_osd_batch) -- is ``performOSD_order`` /
``performOSD_order_batch`` (no reference counterpart: the reference's order-7 call returns OSD-0).
"""
from __future__ import annotations

import numpy as np

from . import bp
from .bp import decoder_for


def _from_last_batch(dec, syn, l, hd):
    """The reference driver calls performOSD once per sample its batch decode did not converge on,
    with rows of the arrays that decode returned (paperResults_GPU.py:113-123): 3 450 launches of
    240 us for a batch that took 3 ms to decode.  The first such call runs OSD-0 for ALL failing rows of
    that batch in one launch; this and the following calls are then answered from its output -- after
    checking that the arguments still hold exactly the values the solution was computed from (OSD is a
    pure function of them).  Anything else (other arrays, changed contents, converged rows) returns None
    and takes the one-syndrome path."""
    lb = bp._last_batch()
    if lb is None or lb.dec is not dec or not isinstance(l, np.ndarray) or not l.flags.c_contiguous:
        return None
    L, Hd = lb.llr, lb.hard
    if L is None or Hd is None:                      # the caller let go of the batch's arrays: nothing to recognise
        bp._set_last_batch(None)
        return None
    off = l.__array_interface__["data"][0] - lb.addr
    if off < 0 or off % lb.rowbytes or off // lb.rowbytes >= lb.rows:
        return None
    with lb.lock:
        if lb.solutions is None:
            idx = np.flatnonzero(~lb.conv)
            inputs = (np.ascontiguousarray(lb.syn[idx]).view(np.uint8), L[idx], Hd[idx].view(np.uint8))
            lb.solutions = dec.osd0(*inputs)
            lb.inputs = inputs
            lb.pos = np.full(lb.rows, -1, np.int64)
            lb.pos[idx] = np.arange(len(idx))
    row = off // lb.rowbytes
    k = lb.pos[row]
    if k < 0:
        return None
    s_in, l_in, h_in = lb.inputs
    if not (np.array_equal(l, l_in[k]) and np.array_equal(hd, h_in[k]) and np.array_equal(syn, s_in[k])):
        return None
    sol = lb.solutions[k].astype(np.int64)
    lb.served.add(int(row))
    if len(lb.served) >= lb.n_fail:                  # every failing row answered: the record has done its job
        bp._set_last_batch(None)
    return sol


def performOSD(H, syndrome, llr, hard):
    return _osd0(decoder_for(H), syndrome, llr, hard)


def _osd0(dec, syndrome, llr, hard):
    syn = (np.asarray(syndrome).astype(np.int64) % 2).astype(np.uint8)
    hd = (np.asarray(hard).astype(np.int64) % 2).astype(np.uint8)
    l = np.asarray(llr, dtype=np.float64)
    if syn.shape != (dec.m,) or hd.shape != (dec.n,) or l.shape != (dec.n,):
        raise ValueError(f"expected syndrome ({dec.m},), llr ({dec.n},), hard ({dec.n},)")
    sol = _from_last_batch(dec, syn, l, hd)
    if sol is not None:
        return sol
    return dec.osd0(syn[None, :], l[None, :], hd[None, :])[0].astype(np.int64)


def performOSD_batch(H, syndromes, llrs, hards):
    """Batch form (no reference counterpart): uint8[B, n] solutions."""
    return decoder_for(H).osd0(syndromes, llrs, hards)


def performOSD_enhanced(H, syndrome, llr, hard, order=0, max_combinations=None):
    dec = decoder_for(H)
    sol = _osd0(dec, syndrome, llr, hard)
    if order == 0:
        return sol
    # (sol @ H.T) % 2 == syndrome, through the decoder's CSR: XOR of the solution bits of every row's columns
    rp, ci = dec.row_ptr, dec.col_idx
    par = np.zeros(dec.m, np.int64)
    full = np.flatnonzero(rp[1:] > rp[:-1])          # (reduceat has no identity for an empty row)
    if len(full):
        par[full] = np.bitwise_xor.reduceat(sol[ci], rp[:-1][full]) & 1
    if np.array_equal(par, np.asarray(syndrome).astype(np.int64) % 2):
        return sol                                   # the reference returns here as well
    raise NotImplementedError("performOSD_enhanced(order > 0) on a syndrome outside the column space "
                              "of H: the reference's combinatorial search is not implemented")


def performOSD_order(H, syndrome, llr, hard, order, method="cs"):
    """Order-w OSD of one decoder output on the GPU (include/qbp.h, qbp_osd_batch): int64 vector like
    ``performOSD``; order 0 is OSD-0."""
    dec = decoder_for(H)
    syn = (np.asarray(syndrome).astype(np.int64) % 2).astype(np.uint8)
    hd = (np.asarray(hard).astype(np.int64) % 2).astype(np.uint8)
    l = np.asarray(llr, dtype=np.float64)
    if syn.shape != (dec.m,) or hd.shape != (dec.n,) or l.shape != (dec.n,):
        raise ValueError(f"expected syndrome ({dec.m},), llr ({dec.n},), hard ({dec.n},)")
    return dec.osd(syn[None, :], l[None, :], hd[None, :], method=method, order=order)[0].astype(np.int64)


def performOSD_order_batch(H, syndromes, llrs, hards, order, method="cs"):
    """Batch form of ``performOSD_order``: uint8[B, n] solutions."""
    return decoder_for(H).osd(syndromes, llrs, hards, method=method, order=order)
