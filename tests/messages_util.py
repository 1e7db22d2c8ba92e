"""Inputs shared by tests/test_messages_cpu.py (which checks on the CPU that they reach what they are meant to reach)
and tests/test_gpu_messages.py (which runs them on the device): matrices, decode modes, and the error / syndrome /
prior draws of the histogram cases."""
import numpy as np

import lsd_util
from oracle import oracle

# (variant, alpha, damping, clip_llr): oracle and device number the variants alike
MINSUM = (oracle.VARIANT_MIN_SUM, 0.8, 0.7, 25.0)
DAMPED = (oracle.VARIANT_DAMPED_SP, 0.9, 0.8, 20.0)
P = 0.08                        # error rate of every draw
GRID_STRIDE_B = 1301            # on [[144, 12, 12]] (E = 432): 562 032 messages
HIST_GRID_ITEMS = 1024 * 256    # one pass of the histogram kernels' grid (qbp_message_histograms)
CONTINUOUS_BINS = (1, 2, 3, 7, 50, 64, 1000)
# (matrix, mode, iteration) of the continuous histogram inputs
CONTINUOUS = [(name, mode, it) for name in ("[[72, 12, 6]]", "rand37")
              for mode, it in ((MINSUM, 0), (DAMPED, 0), (DAMPED, 3))]

_CACHE = {}


def matrix(name):
    """int64 H: 'steane', 'rand37' (the irregular 20 x 37 matrix of the Relay / BPGD tests), 'zeros' (a small matrix
    with an all-zero row and an all-zero column), or a name of tests/test_gpu_geometry.matrix."""
    if name not in _CACHE:
        if name == "steane":
            H = lsd_util.STEANE
        elif name == "rand37":
            H = lsd_util.irregular37()
        elif name == "zeros":
            H = (np.random.default_rng(21).random((9, 14)) < 0.3).astype(np.int64)
            H[4] = 0
            H[:, 6] = 0
            assert H.sum(1).min() == 0 and H.sum(0).min() == 0 and H.sum(1).max() >= 4
        else:
            from test_gpu_geometry import matrix as geometry_matrix
            H = geometry_matrix(name)
        _CACHE[name] = np.ascontiguousarray(H).astype(np.int64)
    return _CACHE[name]


def draw(H, B, seed, prior="nonuniform", p_prior=P):
    """(errors u8[B, n], syndromes u8[B, m], prior f64[n]).  Errors at rate P; prior L = log((1 - p_prior) / p_prior),
    'uniform', 'nonuniform' (uniform(0.5, 1.5) * L per column) or 'integers' (drawn from {1, 2, 3, 4})."""
    rng = np.random.default_rng([seed, B])
    n = H.shape[1]
    errors = (rng.random((B, n)) < P).astype(np.uint8)
    syndromes = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    L = np.log((1 - p_prior) / p_prior)
    if prior == "uniform":
        pr = np.full(n, L)
    elif prior == "nonuniform":
        pr = rng.uniform(0.5, 1.5, n) * L
    else:
        assert prior == "integers"
        pr = rng.choice([1.0, 2.0, 3.0, 4.0], n)
    return errors, syndromes, pr


def continuous_input(name):
    """300 syndromes and a non-uniform prior.  The irregular matrix has a check of weight 1, whose sum-product message
    is +-2 arctanh(0.9999999) = +-16.8 whatever the prior: its prior is scaled to an error rate of 0.005, so that the
    other messages spread over that range instead of sitting in its middle bins."""
    if name == "rand37":
        return draw(matrix(name), 300, 3, "nonuniform", 0.005)
    return draw(matrix(name), 300, 1, "nonuniform")


def edge_input():
    """[[72, 12, 6]], integer priors: with min-sum, alpha = 1, iteration 0 the messages are small integers, the range
    is [-3, 3] and np.linspace's edges are exact for 3, 6 and 12 bins."""
    return draw(matrix("[[72, 12, 6]]"), 300, 5, "integers")


INEXACT_BINS = (11, 22, 50)


def estimate_one_below(edges):
    """Interior edges k on which the bin estimate of hist_bin_kernel, int((v - first) * (bins / (last - first))),
    gives k - 1 for v == edges[k]: the kernel's upward correction (`v >= edge k`: on to bin k) decides their bin."""
    bins = len(edges) - 1
    norm = bins / (edges[-1] - edges[0])
    return [k for k in range(1, bins) if int((edges[k] - edges[0]) * norm) == k - 1]


def inexact_edge_input(bins):
    """[[72, 12, 6]], min-sum, alpha = 1, iteration 0, for `bins` bins whose width is no exact double: two thirds of
    the priors are 3.0 (so that the range is [-3, 3]), the others the magnitudes of those edges of
    np.linspace(-3, 3, bins + 1) on which the rounded bin estimate falls one short.  Messages then sit exactly on such
    edges and land in the right bin only through the correction step."""
    edges = np.linspace(-3.0, 3.0, bins + 1)
    mags = sorted({abs(edges[k]) for k in estimate_one_below(edges)})
    assert mags
    errors, syndromes, _ = draw(matrix("[[72, 12, 6]]"), 300, 8, "uniform")
    rng = np.random.default_rng([8, bins])
    prior = np.where(rng.random(72) < 2 / 3, 3.0, rng.choice(mags, 72))
    return errors, syndromes, prior


def spikes_input():
    return draw(matrix("[[72, 12, 6]]"), 300, 6, "uniform")


def grid_stride_input():
    return draw(matrix("[[144, 12, 12]]"), GRID_STRIDE_B, 7, "nonuniform")
