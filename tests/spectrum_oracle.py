"""Numpy statement of the semantics of ``qbp_mc_run_spectrum`` (include/qbp.h) on top of the CPU oracle: the counters
of ``qbp_mc_run_probs`` plus, per trial (rework/main.py:78-112, spectrum.py:37-54),

  detection = BP's hard decision if BP converged or there is no OSD pass, else the OSD output
  residual  = detection ^ error,  w = popcount(residual),  logical = any(Lx residual),  found = BP converged

  row 0 weights_found_BP        found and not logical and w > 0      row 2 weights_found_BP_error   found and logical
  row 1 weights_found_OSD       not found, not logical and w > 0     row 3 weights_found_OSD_error  not found, logical

and the iteration histogram: bin k < max_iter the trials first satisfied in 0-based iteration k, bin max_iter those BP
did not converge on.  The row depends on ``found`` alone, never on whether OSD ran or its output is valid.
"""
import numpy as np

from oracle import oracle
from osd_order_oracle import osd_order_batch

ROWS = 4


def spectrum_of_errors(H, Lx, distance, errors, prior, max_iter, variant=0, alpha=1.0, damping=1.0, clip_llr=20.0,
                       osd=False, osd_method="cs", osd_order=0):
    """(counters int64[12], spectrum int64[4, n + 1], iter_hist int64[max_iter + 1]) of GIVEN error patterns."""
    H = np.asarray(H).astype(np.int64)
    Lx = np.asarray(Lx).astype(np.int64)
    errors = np.asarray(errors).astype(np.uint8)
    n = H.shape[1]
    syndromes = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    hard, conv, iters, llr = oracle.decode_batch(H, syndromes, prior, max_iter, variant=variant, alpha=alpha,
                                                 damping=damping, clip_llr=clip_llr)
    conv = np.asarray(conv, bool)
    detection = hard.copy()
    late = np.flatnonzero(~conv)
    if osd and len(late):
        if osd_order:
            detection[late] = osd_order_batch(H, syndromes[late], llr[late], hard[late], osd_order, osd_method)
        else:
            for i in late:
                detection[i] = oracle.osd0(H, syndromes[i], llr[i], hard[i])
    counters = oracle.classify_trials(H, Lx, distance, errors, syndromes, detection, conv, iters)
    if osd:
        counters[10] = sum(not np.array_equal((detection[i].astype(np.int64) @ H.T) % 2, syndromes[i]) for i in late)
    residual = (detection ^ errors).astype(np.int64)
    w = residual.sum(axis=1)
    logical = ((residual @ Lx.T) % 2).any(axis=1)
    spectrum = np.zeros((ROWS, n + 1), np.int64)
    for found, lg, row in ((True, False, 0), (False, False, 1), (True, True, 2), (False, True, 3)):
        sel = (conv == found) & (logical == lg) & (w > 0)
        spectrum[row] = np.bincount(w[sel], minlength=n + 1)
    iter_hist = np.bincount(np.where(conv, iters.astype(np.int64), max_iter), minlength=max_iter + 1).astype(np.int64)
    return counters, spectrum, iter_hist


def spectrum_counters(H, Lx, distance, p, prior, trial_begin, trial_end, draws=1, seed=0, max_iter=50, **kw):
    """The same for the trials [trial_begin, trial_end) of the build's own sampler at a uniform error rate p."""
    n = np.asarray(H).shape[1]
    errors = oracle.mc_errors(n, p, draws, seed, trial_begin, trial_end - trial_begin)
    return spectrum_of_errors(H, Lx, distance, errors, prior, max_iter, **kw)


def check_identities(counters, spectrum, iter_hist, max_iter, osd):
    """The identities between the tables and the counters that hold for every run."""
    c = [int(x) for x in counters]
    s = np.asarray(spectrum, np.int64).sum(axis=1)
    assert s[2] + s[3] == c[1]
    assert s[3] == c[8]
    assert s[0] + s[1] == c[0] - c[1] - c[9]
    if not osd:
        assert s[0] == c[5]
    elif c[10] == 0:
        assert s[0] + s[1] == c[5]
    assert not np.asarray(spectrum)[:, 0].any()
    h = np.asarray(iter_hist, np.int64)
    assert len(h) == max_iter + 1
    assert h.sum() == c[0] and h[max_iter] == c[6]
    assert int(np.dot(np.arange(max_iter), h[:max_iter])) + (max_iter - 1) * int(h[max_iter]) == c[7]
