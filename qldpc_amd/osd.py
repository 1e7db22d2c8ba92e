"""Mirror of ``decoding/OSD.py``: ``performOSD(H, syndrome, llr, hard)`` (OSD-0), on the GPU.

Same positional signature and return type (int64 vector, ``(hard + e_correction) % 2``,
OSD.py:26-28).  Equal ``|llr|`` values are ordered by column index (the reference's ``np.argsort``
leaves that order to the numpy build) -- unless the caller gives the order: every function here takes a keyword
``column_order``, an int array ``[n]`` (``[B, n]`` for the batch forms) that lists the columns from the least
reliable on, or the string ``"numpy"`` for ``numpy_order(llr)``, the reference's own expression
``np.argsort(np.abs(llr))`` evaluated by this host's numpy.  With ``QBP_OSD_NUMPY_ORDER=1`` in the environment
``"numpy"`` is the default of every function here (and so of the ``decoding`` drop-in package): ``performOSD`` is
then the reference's function on tied inputs too, wherever the host's numpy is the reference's numpy.

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

import os

import numpy as np

from . import bp
from .bp import decoder_for

# the drop-in's switch for the reference's own tie order (off unless asked for, like QBP_FAST_MATH)
NUMPY_ORDER = os.environ.get("QBP_OSD_NUMPY_ORDER", "0") not in ("0", "")


def numpy_order(llr):
    """``np.argsort(np.abs(llr))`` row by row on 1-D arrays -- decoding/OSD.py:10-11 as written, so that equal
    values come in the order the reference's numpy call leaves them in on this host.  int32, shape of ``llr``."""
    l = np.asarray(llr, dtype=np.float64)
    if l.ndim == 1:
        return np.argsort(np.abs(l)).astype(np.int32)
    return np.stack([np.argsort(np.abs(row)) for row in l]).astype(np.int32) if len(l) else np.zeros(l.shape, np.int32)


def _column_order(column_order, llr):
    """The ``column_order`` argument of the functions below as int array of llr's shape, or None (the device's
    (|llr|, column) sort).  None stands for "numpy" under QBP_OSD_NUMPY_ORDER=1."""
    if column_order is None:
        if not NUMPY_ORDER:
            return None
        column_order = "numpy"
    if isinstance(column_order, str):
        if column_order != "numpy":
            raise ValueError(f"column_order must be an integer array, 'numpy' or None, got {column_order!r}")
        return numpy_order(llr)
    co = np.asarray(column_order)
    if co.dtype.kind not in "iu" or co.shape != np.shape(llr):
        raise ValueError(f"column_order must be an integer array of shape {np.shape(llr)}")
    return co


def _from_last_batch(dec, syn, l, hd, co=None):
    """The reference driver calls performOSD once per sample its batch decode did not converge on,
    with rows of the arrays that decode returned (paperResults_GPU.py:113-123): 3 450 launches of
    240 us for a batch that took 3 ms to decode.  The first such call runs OSD-0 for ALL failing rows of
    that batch in one launch; this and the following calls are then answered from its output -- after
    checking that the arguments still hold exactly the values the solution was computed from (OSD is a
    pure function of them).  Anything else (other arrays, changed contents, converged rows) returns None
    and takes the one-syndrome path.  ``co``: the call's column order -- only numpy_order(l) is served from
    the record (whose launch then ran on numpy_order of every failing row: a function of the row alone, so the
    answer is that of the one-syndrome path), any other order takes the one-syndrome path."""
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
            if co is None:
                lb.solutions = dec.osd0(*inputs)
                lb.orders = None
            else:
                lb.orders = numpy_order(inputs[1])
                lb.solutions = dec.osd(*inputs, order=0, column_order=lb.orders)
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
    orders = lb.orders
    if (co is None) != (orders is None) or (co is not None and not np.array_equal(co, orders[k])):
        return None                                  # the record was computed in another order than this call's
    sol = lb.solutions[k].astype(np.int64)
    lb.served.add(int(row))
    if len(lb.served) >= lb.n_fail:                  # every failing row answered: the record has done its job
        bp._set_last_batch(None)
    return sol


def performOSD(H, syndrome, llr, hard, *, column_order=None):
    return _osd0(decoder_for(H), syndrome, llr, hard, column_order)


def _osd0(dec, syndrome, llr, hard, column_order=None):
    syn = (np.asarray(syndrome).astype(np.int64) % 2).astype(np.uint8)
    hd = (np.asarray(hard).astype(np.int64) % 2).astype(np.uint8)
    l = np.asarray(llr, dtype=np.float64)
    if syn.shape != (dec.m,) or hd.shape != (dec.n,) or l.shape != (dec.n,):
        raise ValueError(f"expected syndrome ({dec.m},), llr ({dec.n},), hard ({dec.n},)")
    numpy_asked = isinstance(column_order, str) or (column_order is None and NUMPY_ORDER)
    co = _column_order(column_order, l)
    if co is None or numpy_asked:                    # (an order of the caller's own is never a record's)
        sol = _from_last_batch(dec, syn, l, hd, co)
        if sol is not None:
            return sol
    if co is None:
        return dec.osd0(syn[None, :], l[None, :], hd[None, :])[0].astype(np.int64)
    return dec.osd(syn[None, :], l[None, :], hd[None, :], order=0, column_order=co[None, :])[0].astype(np.int64)


def performOSD_batch(H, syndromes, llrs, hards, *, column_order=None):
    """Batch form (no reference counterpart): uint8[B, n] solutions."""
    dec = decoder_for(H)
    co = _column_order(column_order, np.asarray(llrs, dtype=np.float64))
    if co is None:
        return dec.osd0(syndromes, llrs, hards)
    return dec.osd(syndromes, llrs, hards, order=0, column_order=co)


def performOSD_enhanced(H, syndrome, llr, hard, order=0, max_combinations=None, *, column_order=None):
    dec = decoder_for(H)
    sol = _osd0(dec, syndrome, llr, hard, column_order)
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


def performOSD_order(H, syndrome, llr, hard, order, method="cs", *, column_order=None, osd_large=False):
    """Order-w OSD of one decoder output on the GPU (include/qbp.h, qbp_osd_batch): int64 vector like
    ``performOSD``; order 0 is OSD-0.  ``osd_large``: order >= 1 also on matrices beyond the one-wavefront kernel
    (FLAG_OSD_LARGE)."""
    dec = decoder_for(H)
    syn = (np.asarray(syndrome).astype(np.int64) % 2).astype(np.uint8)
    hd = (np.asarray(hard).astype(np.int64) % 2).astype(np.uint8)
    l = np.asarray(llr, dtype=np.float64)
    if syn.shape != (dec.m,) or hd.shape != (dec.n,) or l.shape != (dec.n,):
        raise ValueError(f"expected syndrome ({dec.m},), llr ({dec.n},), hard ({dec.n},)")
    co = _column_order(column_order, l)
    kw = {"large": True} if osd_large else {}
    return dec.osd(syn[None, :], l[None, :], hd[None, :], method=method, order=order,
                   column_order=None if co is None else co[None, :], **kw)[0].astype(np.int64)


def performOSD_order_batch(H, syndromes, llrs, hards, order, method="cs", *, column_order=None):
    """Batch form of ``performOSD_order``: uint8[B, n] solutions."""
    co = _column_order(column_order, np.asarray(llrs, dtype=np.float64))
    return decoder_for(H).osd(syndromes, llrs, hards, method=method, order=order, column_order=co)
