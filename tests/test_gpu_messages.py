"""GPU: the alpha_estimation message dump (qbp_check_messages: the dump_R branch of bp_generic_kernel) against
oracle.check_messages, and the two histogram kernels behind qbp_message_histograms (qbp_hist.hpp) against the numpy
statement tests/hist_oracle.py.

Every comparison is bit for bit: messages as uint64 views with NaN equal to NaN (golden_util.same_bits), edges bitwise,
counts exactly.  Both entry points are called through the C ABI into buffers filled with sentinels, so a value that was
never written, or written beyond its range, cannot hide.  tests/test_messages_cpu.py checks on the CPU that the inputs
used here reach the interior bins, the bin edges and more than two passes of the histogram grid."""
import numpy as np
import pytest

import geometry_util as gu
import golden_util
import hist_oracle
import messages_util as mu
from oracle import oracle
from qldpc_amd import _lib, alvarado, bp, rework
from test_gpu_geometry import general_option_sets

pytestmark = pytest.mark.gpu

POISON = gu.LLR_POISON
POISON_BITS = np.float64(POISON).view(np.uint64)
COUNT_POISON = -7
SMALL = ("steane", "[[72, 12, 6]]", "[[144, 12, 12]]", "rand37", "long_row", "zeros")
# (variant, alpha, damping, clip) passed to the device -> the same for the oracle.  Plain sum-product ignores the three
# numbers in the ABI: odd values go in, the bits of the damped update with (1, 1, inf) are expected.
MODES = {"minsum": (mu.MINSUM, mu.MINSUM), "damped": (mu.DAMPED, mu.DAMPED),
         "sp": ((_lib.SUM_PRODUCT, 0.37, 0.21, 3.0), (oracle.VARIANT_DAMPED_SP, 1.0, 1.0, np.inf))}
ITERATIONS = (0, 1, 10)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def decoder(name):
    """A Decoder of this module's own (options set here never reach the decoders other test files share)."""
    return cached(("dec", name), lambda: _lib.Decoder(*bp.csr_from_H(mu.matrix(name)), bp.DEVICE))


# ---- the two entry points through the C ABI, into sentinels ---------------------------------------------------------------
def dump_rc(dec, syn, prior, B, mode, iteration, buf, null=()):
    ptr = lambda nm, a: None if nm in null else a.ctypes.data
    return _lib.load().qbp_check_messages(dec._h, ptr("syn", syn), ptr("prior", prior), int(B), int(mode[0]),
                                          float(mode[1]), float(mode[2]), float(mode[3]), int(iteration), 0,
                                          ptr("messages", buf))


def dump(dec, syn, prior, B, mode, iteration, what):
    """messages float64[B, E] of the first B syndromes: no sentinel left in them, nothing but sentinels behind them."""
    E = len(dec.col_idx)
    buf = np.full((B + gu.PAD) * E, POISON)
    syn = np.ascontiguousarray(syn[:B])
    rc = dump_rc(dec, syn, prior, B, mode, iteration, buf)
    assert rc == 0, (what, rc, _lib.load().qbp_last_error().decode())
    bits = buf.view(np.uint64)
    assert (bits[B * E:] == POISON_BITS).all(), f"{what}: written beyond B * E"
    never = bits[:B * E] == POISON_BITS
    assert not never.any(), f"{what}: {int(never.sum())} messages never written (first {np.flatnonzero(never)[:8]})"
    return buf[:B * E].reshape(B, E).copy()


def assert_same_messages(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = golden_util.same_bits(got, want)
    if not ok.all():
        rows = np.flatnonzero(~ok.all(axis=1))
        b = rows[0]
        e = np.flatnonzero(~ok[b])
        raise AssertionError(f"{what}: messages differ on {len(rows)} of {len(got)} syndromes, first {b} at edges "
                             f"{e[:8]}: got {got[b, e[:4]]}, want {want[b, e[:4]]}")


def hist_rc(dec, syn, err, prior, B, mode, iteration, bins, null=()):
    """(rc, edges, hist0, hist1), the three outputs pre-filled with sentinels (one element more than `bins` asks for)."""
    nb = max(int(bins), 0)
    edges = np.full(nb + 2, POISON)
    h0 = np.full(nb + 1, COUNT_POISON, np.int64)
    h1 = np.full(nb + 1, COUNT_POISON, np.int64)
    ptr = lambda nm, a: None if nm in null else a.ctypes.data
    rc = _lib.load().qbp_message_histograms(dec._h, ptr("syn", syn), ptr("err", err), ptr("prior", prior), int(B),
                                            int(mode[0]), float(mode[1]), float(mode[2]), float(mode[3]), int(iteration),
                                            0, int(bins), ptr("edges", edges), ptr("hist0", h0), ptr("hist1", h1))
    return rc, edges, h0, h1


def untouched(edges, h0, h1):
    return bool((edges.view(np.uint64) == POISON_BITS).all() and (h0 == COUNT_POISON).all() and (h1 == COUNT_POISON).all())


def check_histograms(name, err, syn, prior, dev_mode, ora_mode, iteration, bins, what):
    """One qbp_message_histograms call against the statement.  Where the statement raises (np.histogram's range that is
    not finite) the device must answer QBP_E_INVALID and leave the outputs alone.  Returns the statement's result, or
    None where it raises."""
    H, dec = mu.matrix(name), decoder(name)
    B = len(syn)
    key, what = ("stmt", what, bins), f"{what} bins={bins}"          # (`what` names the inputs: one statement each)
    try:
        want = cached(key, lambda: hist_oracle.message_histograms(H, syn, err, prior, ora_mode[0], bins, *ora_mode[1:],
                                                                  iteration))
    except ValueError:
        want = None
    rc, edges, h0, h1 = hist_rc(dec, syn, err, prior, B, dev_mode, iteration, bins)
    if want is None:
        assert rc == _lib.E_INVALID, (what, rc)
        assert untouched(edges, h0, h1), what
        return None
    assert rc == 0, (what, rc, _lib.load().qbp_last_error().decode())
    w_edges, w0, w1, msg = want
    assert edges.view(np.uint64)[-1] == POISON_BITS and h0[-1] == COUNT_POISON and h1[-1] == COUNT_POISON, what
    edges, h0, h1 = edges[:-1], h0[:-1], h1[:-1]
    assert np.array_equal(edges.view(np.uint64), w_edges.view(np.uint64)), (what, edges, w_edges)
    assert np.array_equal(h0, w0), (what, "class 0", np.flatnonzero(h0 != w0)[:8], h0[h0 != w0][:8], w0[h0 != w0][:8])
    assert np.array_equal(h1, w1), (what, "class 1", np.flatnonzero(h1 != w1)[:8], h1[h1 != w1][:8], w1[h1 != w1][:8])
    rows, cols = np.nonzero(H)
    assert h0.sum() + h1.sum() == B * len(cols), what
    assert h1.sum() == int((err[:, cols] & 1).sum()), what
    return want


# ---- a. the dump against the oracle ---------------------------------------------------------------------------------------
def batch_sizes(name):
    if name == "st144x12":
        return (40,)
    num_cu = decoder(name).info("num_cu")
    return (1, num_cu - 1, 8 * num_cu + 37)


def dump_input(name, prior_kind):
    """(errors, syndromes, prior) of the largest batch of the matrix; a smaller batch is its first rows."""
    return cached(("in", name, prior_kind), lambda: mu.draw(mu.matrix(name), max(batch_sizes(name)), 11, prior_kind,
                                                            0.01 if name == "st144x12" else mu.P))


def oracle_dump(name, prior_kind, mode_name, iteration):
    """The oracle's messages of the largest batch, and the syndromes it had satisfied before `iteration`."""
    def make():
        H = mu.matrix(name)
        _, syn, prior = dump_input(name, prior_kind)
        v, a, d, c = MODES[mode_name][1]
        want = oracle.check_messages(H, syn, prior, v, a, d, c, iteration)
        done = np.zeros(len(syn), bool)
        if iteration > 0:
            done = oracle.decode_batch(H, syn, prior, iteration, v, a, d, c, threads=8)[1]
        return want, done
    return cached(("odump", name, prior_kind, mode_name, iteration), make)


def default_dump(name, prior_kind, mode_name, iteration, B):
    """The device's dump at the automatic geometry, compared with the oracle (once per case)."""
    def make():
        dec = decoder(name)
        _, syn, prior = dump_input(name, prior_kind)
        what = f"dump {name} {prior_kind} {mode_name} iteration={iteration} B={B}"
        got = dump(dec, syn, prior, B, MODES[mode_name][0], iteration, what)
        want, done = oracle_dump(name, prior_kind, mode_name, iteration)
        # Syndromes satisfied before the dump iteration: the reference returns their decode there and no messages
        # (rework/decoding.py:69-71, :185-187 precede the next iteration's dump), so only the others have a reference
        # value.  Oracle and device nevertheless follow ONE rule on them: both run with forced iterations
        # (ORACLE_FLAG_FORCE_FULL in oracle_bp_check_messages, QBP_FLAG_FORCE_FULL in dump_messages), under which a
        # satisfied syndrome goes on through the same check and variable updates (bp_oracle.c: `done` only guards the
        # outputs; bp_generic_kernel: `frozen` only guards the parity flips and the emission) and is dumped at
        # `iteration` like the others.  So the open syndromes are compared first, then all of them.
        open_ = ~done[:B]
        assert_same_messages(got[open_], want[:B][open_], what + " (syndromes still open)")
        assert_same_messages(got, want[:B], what + " (all syndromes)")
        print(f"DUMP {what}: grid={dec.info('grid')} threads={dec.info('threads')} open={int(open_.sum())}")
        return got
    return cached(("ddump", name, prior_kind, mode_name, iteration, B), make)


@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("name", SMALL + ("st144x12",))
def test_dump_equals_oracle(name, mode_name):
    """Iterations 0, 1 and 10 x uniform and non-uniform prior x B in {1, CUs - 1, 8 CUs + 37} (the last: every
    workgroup fetches further syndromes from the work counter after a dump); 40 syndromes on 864 x 2592."""
    for prior_kind in ("uniform", "nonuniform"):
        for iteration in ITERATIONS:
            for B in batch_sizes(name):
                default_dump(name, prior_kind, mode_name, iteration, B)
    if name in ("[[72, 12, 6]]", "[[144, 12, 12]]"):           # (the iteration-10 case is not empty of open syndromes)
        assert (~oracle_dump(name, "nonuniform", mode_name, 10)[1]).sum() > 10


@pytest.mark.parametrize("mode_name,iteration", [("minsum", 1), ("damped", 10)])
@pytest.mark.parametrize("name", ["long_row", "[[144, 12, 12]]", "st144x12"])
def test_dump_across_launch_geometries(name, mode_name, iteration):
    """Workgroup width {64, 192, 1024} x workgroups per CU {1, 8} x messages in {LDS, global memory, split}, and the
    two A/B switches: the dump of every geometry equals the automatic geometry's, which equals the oracle's."""
    dec = decoder(name)
    num_cu = dec.info("num_cu")
    _, syn, prior = dump_input(name, "nonuniform")
    for B in batch_sizes(name)[-2:]:
        ref = default_dump(name, "nonuniform", mode_name, iteration, B)
        for opts in general_option_sets():
            what = f"dump {name} {mode_name} iteration={iteration} B={B} {opts}"
            with gu.options(dec, **opts):
                got = dump(dec, syn, prior, B, MODES[mode_name][0], iteration, what)
                grid, threads = dec.info("grid"), dec.info("threads")
            if "threads" in opts:
                assert threads == opts["threads"], what
                per_cu = 1 if opts["mem"] == 2 else opts["blocks"]
                assert grid == min(B, num_cu * per_cu), (what, grid)
            assert_same_messages(got, ref, what)


def test_dump_calls_that_leave_the_buffer_untouched():
    name = "[[72, 12, 6]]"
    dec = decoder(name)
    _, syn, prior = dump_input(name, "uniform")
    E = len(dec.col_idx)
    syn = np.ascontiguousarray(syn[:5])
    for what, B, mode, iteration, rc_want in (("B = 0", 0, mu.MINSUM, 0, 0), ("iteration = -1", 5, mu.MINSUM, -1, -1),
                                              ("unknown variant", 5, (7, 1.0, 1.0, 20.0), 0, -1)):
        buf = np.full(8 * E, POISON)
        assert dump_rc(dec, syn, prior, B, mode, iteration, buf) == rc_want, what
        assert (buf.view(np.uint64) == POISON_BITS).all(), what
    for null in ("syn", "prior", "messages"):
        buf = np.full(8 * E, POISON)
        assert dump_rc(dec, syn, prior, 5, mu.MINSUM, 0, buf, null=(null,)) == _lib.E_INVALID, null
        assert (buf.view(np.uint64) == POISON_BITS).all(), null


def test_handle_reuse_between_decodes():
    """decode -> check_messages -> message_histograms -> decode on one handle (the dump lives in the handle's LLR
    buffer): both decodes return the oracle's bits."""
    name = "[[144, 12, 12]]"
    H, dec = mu.matrix(name), decoder(name)
    err, syn, prior = (x[:300] if x.ndim == 2 else x for x in dump_input(name, "nonuniform"))
    kw = dict(variant=_lib.MIN_SUM, alpha=0.8, damping=0.7, clip_llr=25.0)
    first = dec.decode(syn, prior, 50, **kw)
    dec.check_messages(syn[:77], prior, _lib.DAMPED_SP, 0.9, 0.8, 20.0, 3)
    dec.message_histograms(syn, err, prior, _lib.MIN_SUM, 0.8, 0.7, 25.0, 0, bins=50)
    second = dec.decode(syn, prior, 50, **kw)
    o = oracle.decode_batch(H, syn, prior, 50, threads=8, **kw)
    gu.assert_same(first[:4], (o[0], o[1], o[2], o[3]), "first decode vs oracle")
    gu.assert_same(second[:4], first[:4], "decode after the dump and the histograms vs the first decode")


# ---- b. the histograms against the statement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,iteration", mu.CONTINUOUS, ids=lambda v: str(v).replace(" ", ""))
def test_histograms_continuous(name, mode, iteration):
    """Messages spread over the interior bins.  (Min-sum on the irregular matrix: its check of weight 1 sends an
    infinite message, the statement raises and the device refuses, for every bin count.)"""
    err, syn, prior = mu.continuous_input(name)
    seen = []
    for bins in mu.CONTINUOUS_BINS:
        what = f"continuous {name} {mode} iteration={iteration}"
        seen.append(check_histograms(name, err, syn, prior, mode, mode, iteration, bins, what))
    assert all(s is None for s in seen) == (name == "rand37" and mode is mu.MINSUM)


def test_histograms_messages_on_the_edges():
    """Integer messages, exact edges: a message on an interior edge is counted in the bin to its right, the maximum
    in the last bin (np.histogram's rule; the counts are np.histogram's own)."""
    name = "[[72, 12, 6]]"
    err, syn, prior = mu.edge_input()
    mode = (_lib.MIN_SUM, 1.0, 1.0, np.inf)
    for bins in (3, 6, 12):
        want = check_histograms(name, err, syn, prior, mode, mode, 0, bins, "edge")
        edges, h0, h1, msg = want
        assert (msg == edges[-1]).sum() > 0 and h0[-1] + h1[-1] >= (msg == edges[-1]).sum()
    # with 6 bins every message sits on an edge: bin k holds exactly the messages equal to edge k, the last bin
    # those equal to edge 5 and to edge 6
    edges, h0, h1, msg = check_histograms(name, err, syn, prior, mode, mode, 0, 6, "edge")
    count = [(msg == x).sum() for x in edges]
    assert list(h0 + h1) == count[:5] + [count[5] + count[6]]


def test_histograms_messages_on_inexact_edges():
    """Messages equal to edges of np.linspace(-3, 3, bins + 1) on which the kernel's index estimate is one short
    (tests/messages_util.py): only the `v >= next edge` correction puts them to the right of their edge."""
    name = "[[72, 12, 6]]"
    mode = (_lib.MIN_SUM, 1.0, 1.0, np.inf)
    for bins in mu.INEXACT_BINS:
        err, syn, prior = mu.inexact_edge_input(bins)
        check_histograms(name, err, syn, prior, mode, mode, 0, bins, "inexact edges")


def test_histograms_two_spikes():
    name = "[[72, 12, 6]]"
    err, syn, prior = mu.spikes_input()
    mode = (_lib.MIN_SUM, 1.0, 1.0, np.inf)
    for bins in (1, 2, 50):
        edges, h0, h1, msg = check_histograms(name, err, syn, prior, mode, mode, 0, bins, "spikes")
        assert not (h0 + h1)[1:-1].any() and (h0 + h1)[0] > 0 and (h0 + h1)[-1] > 0


def test_histograms_degenerate_range():
    """All-zero syndromes and errors on the Steane code: every message has one value, np.histogram widens the range
    to [value - 0.5, value + 0.5]."""
    name = "steane"
    n, m = mu.matrix(name).shape[1], mu.matrix(name).shape[0]
    err, syn = np.zeros((9, n), np.uint8), np.zeros((9, m), np.uint8)
    prior = np.full(n, 2.0)
    mode = (_lib.MIN_SUM, 1.0, 1.0, np.inf)
    for bins in (1, 4, 50):
        edges, h0, h1, msg = check_histograms(name, err, syn, prior, mode, mode, 0, bins, "degenerate")
        assert len(np.unique(msg)) == 1 and edges[0] == msg[0, 0] - 0.5 and edges[-1] == msg[0, 0] + 0.5
        assert h1.sum() == 0


@pytest.mark.parametrize("mode", [mu.MINSUM, mu.DAMPED], ids=["minsum", "damped"])
def test_histograms_grid_stride(mode):
    """562 032 messages: both kernels' grid-stride loops run more than two passes and end on a ragged one."""
    err, syn, prior = mu.grid_stride_input()
    check_histograms("[[144, 12, 12]]", err, syn, prior, mode, mode, 0, 50, f"grid stride {mode}")


def test_histograms_bins_at_the_limit():
    name = "[[72, 12, 6]]"
    err, syn, prior = mu.continuous_input(name)
    for bins in (4095, 4096):
        check_histograms(name, err, syn, prior, mu.DAMPED, mu.DAMPED, 3, bins, "limit")
    for bins in (0, 4097, -1):
        rc, edges, h0, h1 = hist_rc(decoder(name), syn, err, prior, len(syn), mu.DAMPED, 3, bins)
        assert rc == _lib.E_INVALID and untouched(edges, h0, h1), bins


def test_histograms_long_rows_and_memory_modes():
    """The histograms of the dumps that test_dump_across_launch_geometries pins: a row of weight 22, and 864 x 2592
    with the messages in LDS, in global memory and split."""
    err, syn, prior = dump_input("long_row", "nonuniform")
    for mode in (mu.MINSUM, mu.DAMPED):
        check_histograms("long_row", err[:300], syn[:300], prior, mode, mode, 1, 50, f"long_row {mode}")
    err, syn, prior = dump_input("st144x12", "nonuniform")
    dec = decoder("st144x12")
    for mem in (0, 1, 2):
        with gu.options(dec, mem=mem):
            for mode in (mu.MINSUM, mu.DAMPED):
                check_histograms("st144x12", err, syn, prior, mode, mode, 1, 50, f"st144x12 {mode}")


def test_histogram_refusals():
    """A NaN message (one NaN prior entry turns the messages of its checks NaN), nothing but NaN, a null pointer,
    B = 0: QBP_E_INVALID with edges and counts untouched, where the statement raises ValueError."""
    name = "[[72, 12, 6]]"
    H, dec = mu.matrix(name), decoder(name)
    err, syn, prior = mu.continuous_input(name)
    one = prior.copy()
    one[5] = np.nan
    for what, pr in (("one NaN", one), ("all NaN", np.full_like(prior, np.nan))):
        for mode in (mu.MINSUM, mu.DAMPED):
            msg = oracle.check_messages(H, syn, pr, *mode, 0)
            assert np.isnan(msg).any() and (what == "all NaN" or not np.isnan(msg).all())
            assert check_histograms(name, err, syn, pr, mode, mode, 0, 50, f"refusal {what} {mode}") is None
    for null in ("syn", "err", "prior", "edges", "hist0", "hist1"):
        rc, edges, h0, h1 = hist_rc(dec, syn, err, prior, len(syn), mu.MINSUM, 0, 50, null=(null,))
        assert rc == _lib.E_INVALID and untouched(edges, h0, h1), null
    rc, edges, h0, h1 = hist_rc(dec, syn, err, prior, 0, mu.MINSUM, 0, 50)
    assert rc == _lib.E_INVALID and untouched(edges, h0, h1)
    # the handle still works
    check_histograms(name, err, syn, prior, mu.MINSUM, mu.MINSUM, 0, 50, f"continuous {name} {mu.MINSUM} iteration=0")


# ---- c. the Python mirrors ------------------------------------------------------------------------------------------------
def test_estimate_alpha_on_a_second_configuration(capsys):
    """[[144, 12, 12]], 700 trials, error rate 0.06, 40 bins: against the reference's own call sequence on the
    statement's messages (rework/Alvarado.py:41-62: np.histogram(density=True) per class, curve_fit of a * x)."""
    from scipy.optimize import curve_fit
    H = mu.matrix("[[144, 12, 12]]")
    trials, rate, bins, n = 700, 0.06, 40, H.shape[1]
    np.random.seed(7)
    got = alvarado.estimate_alpha_from_code(H, trials=trials, error_rate=rate, maxIter=1, bins=bins)
    assert "Estimated alpha for error rate 0.06" in capsys.readouterr().out
    np.random.seed(7)
    errors = np.empty((trials, n), np.uint8)
    for t in range(trials):
        errors[t] = np.random.random(n) < rate
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    msg = oracle.check_messages(H, syn, np.full(n, np.log((1 - rate) / rate)), oracle.VARIANT_MIN_SUM, 1.0, 1.0, np.inf, 0)
    cls = errors[:, np.nonzero(H)[1]]
    m0, m1 = msg[cls == 0], msg[cls == 1]
    rng_ = (min(m0.min(), m1.min()), max(m0.max(), m1.max()))
    h0, edges = np.histogram(m0, bins=bins, range=rng_, density=True)
    h1, _ = np.histogram(m1, bins=bins, range=rng_, density=True)
    centres = (edges[:-1] + edges[1:]) / 2
    ok = (h0 > 0) & (h1 > 0)
    want = curve_fit(lambda x, a: a * x, centres[ok], np.log(h0[ok] / h1[ok]))[0][0]
    assert got == pytest.approx(want, rel=1e-9)


@pytest.mark.parametrize("name", ["long_row", "rand37"])
def test_rework_alpha_estimation_returns_the_dense_messages(name):
    H = mu.matrix(name)
    rows, cols = np.nonzero(H)
    _, syn, prior = mu.draw(H, 4, 13)
    for b in range(len(syn)):
        for fn, args, ora in ((rework.performMinSum_Symmetric, dict(maxIter=1, alpha=0.8, damping=0.7, clip_llr=25.0),
                               (*mu.MINSUM, 0)),
                              (rework.performBeliefPropagation_Symmetric,
                               dict(maxIter=50, alpha=0.9, damping=0.8, clip_llr=20.0), (*mu.DAMPED, 10))):
            out = fn(H, syn[b], list(prior), alpha_estimation=True, **args)
            assert out[0] == 0 and out[1] == 0 and out[3] == 0 and out[2].shape == H.shape
            want = oracle.check_messages(H, syn[b:b + 1], prior, *ora, flags=oracle.colsum_flags("minsum", H))[0]
            assert golden_util.same_bits(out[2][rows, cols], want).all(), (name, fn.__name__, b)
            assert not out[2][H == 0].any()
