"""CPU: the numpy statement of qbp_message_histograms (tests/hist_oracle.py) reproduces the reference's alpha, and the
inputs of tests/test_gpu_messages.py reach what they are meant to reach (so that no GPU case there is vacuous)."""
import os

import numpy as np
import pytest

import hist_oracle
import messages_util as mu
from oracle import oracle
from qldpc_amd import alvarado

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alpha_est.npz")


def golden_draw():
    """The draw of tests/golden/alpha_est.npz: (H, errors, syndromes, prior, bins, alpha)."""
    d = np.load(GOLD)
    H = d["H"].astype(np.int64)
    trials, error_rate, bins, seed = d["alpha_fit_args"]
    assert (int(trials), float(error_rate), int(bins), int(seed)) == (400, 0.08, 50, 123)
    n = H.shape[1]
    np.random.seed(int(seed))
    errors = np.empty((int(trials), n), np.uint8)
    for t in range(int(trials)):                      # one call per trial: rework/Alvarado.py:17-21
        errors[t] = np.random.random(n) < error_rate
    syndromes = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = np.full(n, np.log((1 - error_rate) / error_rate))
    return H, errors, syndromes, prior, int(bins), float(d["alpha_fit"][0])


def test_statement_reproduces_the_golden_alpha():
    H, errors, syndromes, prior, bins, alpha = golden_draw()
    edges, h0, h1, msg = hist_oracle.message_histograms(H, syndromes, errors, prior, oracle.VARIANT_MIN_SUM, bins, 1.0,
                                                        1.0, np.inf, 0)
    assert alvarado.alpha_from_histograms(edges, h0, h1) == pytest.approx(alpha, rel=1e-12)
    assert h0.sum() + h1.sum() == msg.size
    # why that input is not enough: two message values, so only the first and the last bin are ever filled
    assert len(np.unique(msg)) == 2
    assert not h0[1:-1].any() and not h1[1:-1].any()


def test_statement_raises_on_a_range_that_is_not_finite():
    H = mu.matrix("[[72, 12, 6]]")
    errors, syndromes, prior = mu.draw(H, 8, 1)
    bad = prior.copy()
    bad[5] = np.nan
    for pr in (bad, np.full_like(prior, np.nan)):
        with pytest.raises(ValueError, match="not finite"):
            hist_oracle.message_histograms(H, syndromes, errors, pr, *mu.MINSUM[:1], 50, *mu.MINSUM[1:], 0)


def test_edge_input_puts_messages_on_the_edges():
    """On [[72, 12, 6]] with 3 bins the share of messages that equal an edge is 0.70."""
    H = mu.matrix("[[72, 12, 6]]")
    errors, syndromes, prior = mu.edge_input()
    for bins in (3, 6, 12):
        edges, h0, h1, msg = hist_oracle.message_histograms(H, syndromes, errors, prior, oracle.VARIANT_MIN_SUM, bins,
                                                            1.0, 1.0, np.inf, 0)
        assert np.array_equal(edges, np.linspace(-3.0, 3.0, bins + 1)) and (msg == np.round(msg)).all()
        assert np.isin(msg, edges).mean() >= 0.5
        assert np.isin(msg, edges[1:-1]).any() and (msg == edges[-1]).any()     # interior edges and the maximum
        # a message on interior edge k belongs to bin k (the one to its right), the maximum to the last bin
        for k in range(1, bins):
            assert h0[k] + h1[k] >= (msg == edges[k]).sum()
        assert h0[-1] + h1[-1] >= (msg == edges[-1]).sum() > 0


@pytest.mark.parametrize("bins", mu.INEXACT_BINS)
def test_inexact_edge_input_reaches_the_correction_step(bins):
    """The exact edges above are binned right by the index estimate alone (it is exact there).  Here at least a quarter
    of the messages equal an interior edge on which the estimate is one short, so the kernel's `v >= next edge` step
    decides their bin; np.histogram puts them to the right of that edge."""
    H = mu.matrix("[[72, 12, 6]]")
    errors, syndromes, prior = mu.inexact_edge_input(bins)
    edges, h0, h1, msg = hist_oracle.message_histograms(H, syndromes, errors, prior, oracle.VARIANT_MIN_SUM, bins, 1.0,
                                                        1.0, np.inf, 0)
    assert (edges[0], edges[-1]) == (-3.0, 3.0)
    short = mu.estimate_one_below(edges)
    assert short and sum((msg == edges[k]).sum() for k in short) >= msg.size // 4
    for k in short:
        assert h0[k] + h1[k] >= (msg == edges[k]).sum()


@pytest.mark.parametrize("name,mode,iteration", mu.CONTINUOUS, ids=lambda v: str(v).replace(" ", ""))
def test_continuous_inputs_fill_the_interior_bins(name, mode, iteration):
    """At least half of the 50 bins of each class are non-empty, and an interior bin is non-empty in both classes.

    Two inputs on the irregular 20 x 37 matrix cannot do that, because the matrix has a check of weight 1:
    * min-sum: that check's message is +-inf, the range is not finite and the statement raises (the device must refuse);
    * damped sum-product at iteration 0: that check's message is +-16.8 whatever the prior, the other messages
      take at most two values per edge and lie within a part of that range -- 13 of 50 bins at best (measured for
      priors from p = 0.08 down to 0.001).  The interior bins are still reached, which is asserted."""
    H = mu.matrix(name)
    errors, syndromes, prior = mu.continuous_input(name)
    args = (H, syndromes, errors, prior, mode[0], 50, *mode[1:], iteration)
    if name == "rand37" and mode is mu.MINSUM:
        assert (H.sum(1) == 1).any()
        with pytest.raises(ValueError, match="not finite"):
            hist_oracle.message_histograms(*args)
        return
    edges, h0, h1, msg = hist_oracle.message_histograms(*args)
    assert ((h0[1:-1] > 0) & (h1[1:-1] > 0)).any()
    if name == "rand37" and iteration == 0:
        assert ((h0 > 0)[1:-1].sum() >= 8) and ((h1 > 0)[1:-1].sum() >= 8)
    else:
        assert (h0 > 0).sum() >= 25 and (h1 > 0).sum() >= 25
    assert len(np.unique(msg)) > 50


def test_spikes_input_has_two_values():
    H = mu.matrix("[[72, 12, 6]]")
    errors, syndromes, prior = mu.spikes_input()
    msg = oracle.check_messages(H, syndromes, prior, oracle.VARIANT_MIN_SUM, 1.0, 1.0, np.inf, 0)
    assert len(np.unique(msg)) == 2


def test_grid_stride_batch_is_more_than_two_passes_and_ragged():
    E = int(mu.matrix("[[144, 12, 12]]").sum())
    assert E == 432
    items = mu.GRID_STRIDE_B * E
    assert items > 2 * mu.HIST_GRID_ITEMS and items % 256 != 0
