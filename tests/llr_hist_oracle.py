"""Numpy statement of the semantics of ``qbp_mc_run_llr_hist`` (include/qbp.h) on top of the CPU oracle: the table
int64[K, 4, bins + 3] of the posterior LLRs of a ladder of BP iteration limits b_0 < ... < b_{K-1}.

For budget row j, ``(hard, conv, it, llr)`` is what a decode of the trial's syndrome with max_iter = b_j returns -- one
decode per budget, nothing shared between rows -- and every one of the trial's n values llr[v] adds 1 to
``hist[j, 2 * (not conv) + error[v], col(llr[v])]``: column 0 below ``lo`` (-inf too), columns 1 .. bins the counts of
``np.histogram(x, bins, range=(lo, hi))`` itself, column bins + 1 above ``hi`` (+inf too), column bins + 2 NaN.
"""
import numpy as np

from oracle import oracle

ROWS = 4


def dense(H):
    """H as a dense int64 array (detector error models come as scipy-sparse matrices)."""
    return np.asarray(H.toarray() if hasattr(H, "toarray") else H).astype(np.int64)


def columns(x, bins, lo, hi):
    """int64[bins + 3]: the counts of the values x in the columns of one table row."""
    x = np.asarray(x, np.float64).ravel()
    out = np.zeros(bins + 3, np.int64)
    nan = np.isnan(x)
    out[bins + 2] = nan.sum()
    x = x[~nan]
    out[0] = (x < lo).sum()
    out[bins + 1] = (x > hi).sum()
    inside = x[(x >= lo) & (x <= hi)]
    out[1:bins + 1] = np.histogram(inside, bins, range=(lo, hi))[0]
    return out


def table_of_outputs(errors, outputs, bins, lo, hi):
    """The table from the decodes themselves: ``outputs[j] = (conv bool[T], llr float64[T, n])`` of budget j."""
    errors = np.asarray(errors).astype(bool)
    hist = np.zeros((len(outputs), ROWS, bins + 3), np.int64)
    for j, (conv, llr) in enumerate(outputs):
        conv = np.asarray(conv).astype(bool)
        for r in range(ROWS):
            pick = (conv != bool(r >> 1))[:, None] & (errors == bool(r & 1))
            hist[j, r] = columns(np.asarray(llr)[pick], bins, lo, hi)
    return hist


def llr_hist_of_errors(H, errors, prior, budgets, bins, lo, hi, decode=None, **kw):
    """The table of GIVEN error patterns uint8[T, n].  ``decode(syndromes, max_iter) -> (hard, conv, iters, llr)``:
    by default the CPU oracle with ``kw`` (variant, alpha, damping, clip_llr)."""
    H = dense(H)
    errors = np.asarray(errors, np.uint8)
    syndromes = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    if decode is None:
        def decode(syn, max_iter):
            return oracle.decode_batch(H, syn, prior, max_iter, **kw)
    outputs = []
    for b in budgets:
        _, conv, _, llr = decode(syndromes, int(b))
        outputs.append((conv, llr))
    return table_of_outputs(errors, outputs, bins, lo, hi)


def llr_hist(H, p, prior, trial_begin, trial_end, budgets, bins, lo, hi, draws=1, seed=0, decode=None, **kw):
    """The table of the sampler's trials [trial_begin, trial_end): ``p`` a uniform error rate, or one per column."""
    H = dense(H)
    if np.ndim(p) == 0:
        errors = oracle.mc_errors(H.shape[1], float(p), draws, seed, trial_begin, trial_end - trial_begin)
    else:
        from dem_sampler import errors_probs
        errors = errors_probs(p, draws, seed, trial_begin, trial_end - trial_begin)
    return llr_hist_of_errors(H, errors, prior, budgets, bins, lo, hi, decode=decode, **kw)
