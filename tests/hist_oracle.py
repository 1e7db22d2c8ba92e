"""The statement of qbp_message_histograms in numpy -- TEST INFRASTRUCTURE.

rework/Alvarado.py:31-49 with counts instead of densities: the check->variable messages of the dump
(oracle.check_messages), split by the true value of the bit they address, one np.histogram per class over the
common range of all messages.  np.histogram itself is called, its binning rule is not restated here."""
import numpy as np

from oracle import oracle


def message_histograms(H, syndromes, errors, prior, variant, bins, alpha, damping, clip_llr, iteration, flags=0):
    """(edges float64[bins + 1], hist0 int64[bins], hist1 int64[bins], messages float64[B, E]).  ValueError where
    np.histogram raises: a range that is not finite (a NaN or an infinite message)."""
    H = np.asarray(H)
    messages = oracle.check_messages(H, syndromes, prior, variant, alpha, damping, clip_llr, iteration, flags=flags)
    rows, cols = np.nonzero(H)                               # CSR edge order: row by row, ascending column
    cls = np.asarray(errors)[:, cols] & 1                    # class of message (b, e) = errors[b, cols[e]]
    lo, hi = messages.min(), messages.max()
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
    hist0, edges = np.histogram(messages[cls == 0], bins=bins, range=(lo, hi))
    hist1, edges1 = np.histogram(messages[cls == 1], bins=bins, range=(lo, hi))
    assert np.array_equal(edges, edges1)
    return edges, hist0.astype(np.int64), hist1.astype(np.int64), messages
