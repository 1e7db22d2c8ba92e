"""GPU: fixed-weight Monte-Carlo (qbp_mc_run_weight) -- the device sampler against its numpy statement
(tests/weight_oracle.py) bit for bit, the counters against the stored-errors pipeline (qbp_mc_run_errors) fed the
statement's errors, chunk / shard invariance, the _device form, the argument checks, and the weight-stratified LER of
a code small enough to enumerate against a Bernoulli run."""
import math

import numpy as np
import pytest

from qldpc_amd import _lib, bp, codes, mc
from weight_oracle import errors_weight

pytestmark = pytest.mark.gpu

OSD_CS7 = _lib.osd_flags("cs", 7)
SEEDS = (3, 0xC0FFEE123456789)            # (the second is above 2^32: both key words in use)
BEGINS = (0, 2 ** 32 - 100)               # (the second: the counter's low word wraps inside a batch of 257)


def irregular37():
    """An irregular 20 x 37 matrix (row weights 1 .. 13, column weights 1 .. 7: the general-H kernel) and three
    logical rows."""
    rng = np.random.default_rng(37)
    H = (rng.random((20, 37)) < rng.uniform(0.05, 0.3, size=(20, 1))).astype(np.uint8)
    H[np.arange(20), rng.integers(0, 37, 20)] = 1          # (no empty row)
    L = (rng.random((3, 37)) < 0.3).astype(np.uint8)
    return H, L


def matrices():
    st = codes.load_code("steane")
    c72 = codes.load_code("[[72, 12, 6]]")
    H37, L37 = irregular37()
    return {"steane": (st.Hx, np.ones((1, 7), np.uint8), 3), "72": (c72.Hx, c72.Lx, c72.distance), "rand37": (H37, L37, 4)}


def fresh(H):
    return _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)


# ---- 1. the sampler, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steane", "72", "rand37"])
def test_sampler_equals_statement(name):
    H, _, _ = matrices()[name]
    n = H.shape[1]
    dec = fresh(H)
    T = 257
    for w in sorted({0, 1, 2, 5, 9, n - 1, n} & set(range(n + 1))):
        for seed in SEEDS:
            for begin in BEGINS:
                got = dec.mc_sample_errors_weight(w, begin, T, seed=seed)
                assert np.array_equal(got.sum(axis=1), np.full(T, w)), (name, w, seed, begin)
                assert np.array_equal(got, errors_weight(n, w, seed, begin, T)), (name, w, seed, begin)


def test_sampler_clears_a_reused_buffer():
    H, _, _ = matrices()["72"]
    dec = fresh(H)
    T = 257
    first = dec.mc_sample_errors_weight(12, 0, T, seed=1)
    assert np.array_equal(first.sum(axis=1), np.full(T, 12))
    second = dec.mc_sample_errors_weight(2, 0, T, seed=1)          # (same handle, same buffer, same size)
    assert np.array_equal(second.sum(axis=1), np.full(T, 2))
    assert np.array_equal(second, errors_weight(72, 2, 1, 0, T))


# ---- 2. the counters: those of the stored-errors pipeline on the statement's errors ---------------------------------------------
def expect(dec, L, d, n, w, seed, begin, T, prior, **kw):
    return dec.mc_run_errors(L, d, errors_weight(n, w, seed, begin, T), prior, **kw)


@pytest.mark.parametrize("mode", ["on_chip", "generic", "osd0", "cs7", "min_sum"])
def test_counters_equal_stored_errors_pipeline_72(mode):
    H, L, d = matrices()["72"]
    n, T = 72, 2000
    prior = mc.prior_of(0.02, n)
    dec = fresh(H)
    kw = dict(max_iter=20)
    if mode == "generic":
        dec.set_option(_lib.OPT_FORCE_GENERIC, 1)
    elif mode == "osd0":
        kw["flags"] = _lib.FLAG_OSD0
    elif mode == "cs7":
        kw["flags"] = OSD_CS7
    elif mode == "min_sum":
        kw.update(variant=_lib.MIN_SUM, alpha=0.8)
    for w in (2, 6, 12):
        got = dec.mc_run_weight(L, d, w, prior, 0, T, seed=9, **kw)
        assert dec.info("last_kernel") == (2 if mode == "generic" else 1)
        want = expect(dec, L, d, n, w, 9, 0, T, prior, **kw)
        assert got[0] == T
        assert np.array_equal(got, want), (mode, w, got, want)
        if w == 12:
            assert got[1] > 0 or got[6] > 0          # (weight 2 d: not a run the decoder gets right throughout)
        # ew < distance / 2 is evaluated with the actual weight: every logical error goes to one side
        assert (got[3], got[4]) == ((got[1], 0) if w < d // 2 else (0, got[1]))


def test_counters_equal_stored_errors_pipeline_irregular():
    H, L, d = matrices()["rand37"]
    n, T = 37, 2000
    prior = mc.prior_of(0.05, n)
    dec = fresh(H)
    for w in (1, 3, 9):
        got = dec.mc_run_weight(L, d, w, prior, 0, T, seed=4, max_iter=20, flags=_lib.FLAG_OSD0)
        assert dec.info("last_kernel") == 2
        assert np.array_equal(got, expect(dec, L, d, n, w, 4, 0, T, prior, max_iter=20, flags=_lib.FLAG_OSD0)), w


# ---- 3. chunks and shards --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _lib.FLAG_OSD0], ids=["bp", "osd0"])
def test_chunk_and_shard_invariance(flags):
    H, L, d = matrices()["72"]
    prior = mc.prior_of(0.02, 72)
    kw = dict(seed=21, max_iter=20, flags=flags)
    whole = fresh(H).mc_run_weight(L, d, 8, prior, 0, 1000, **kw)
    chunked = fresh(H)
    chunked.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 100)             # ten chunks on one buffer
    assert np.array_equal(chunked.mc_run_weight(L, d, 8, prior, 0, 1000, **kw), whole)
    chunked.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 333)             # (a last chunk of one trial)
    assert np.array_equal(chunked.mc_run_weight(L, d, 8, prior, 0, 1000, **kw), whole)
    parts = chunked.mc_run_weight(L, d, 8, prior, 0, 337, **kw) + chunked.mc_run_weight(L, d, 8, prior, 337, 1000, **kw)
    assert np.array_equal(parts, whole)
    assert np.array_equal(whole, expect(chunked, L, d, 72, 8, 21, 0, 1000, prior, max_iter=20, flags=flags))
    with pytest.raises(_lib.QbpError):
        chunked.set_option(_lib.OPT_MC_WEIGHT_CHUNK, -1)


def test_large_trial_index_and_shard():
    H, L, d = matrices()["72"]
    prior = mc.prior_of(0.02, 72)
    dec = fresh(H)
    begin = 2 ** 32 - 100
    got = dec.mc_run_weight(L, d, 9, prior, begin, begin + 257, seed=SEEDS[1], max_iter=20)
    assert np.array_equal(got, expect(dec, L, d, 72, 9, SEEDS[1], begin, 257, prior, max_iter=20))


# ---- 4. the _device form -----------------------------------------------------------------------------------------------------
def test_device_form_adds_to_counters():
    import torch
    H, L, d = matrices()["72"]
    prior = mc.prior_of(0.02, 72)
    dec = fresh(H)
    dev = torch.device("cuda", bp.DEVICE)
    start = np.arange(100, 112, dtype=np.int64)
    d_cnt = torch.from_numpy(start.copy()).to(dev)
    d_prior = torch.from_numpy(prior).to(dev)
    stream = torch.cuda.current_stream(dev)
    for a, b in ((0, 400), (400, 1000)):
        dec.mc_run_weight_device(L, d, 7, d_prior.data_ptr(), a, b, d_cnt.data_ptr(), seed=2, max_iter=20,
                                 flags=_lib.FLAG_OSD0, stream=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    host = dec.mc_run_weight(L, d, 7, prior, 0, 1000, seed=2, max_iter=20, flags=_lib.FLAG_OSD0)
    assert np.array_equal(d_cnt.cpu().numpy(), start + host)
    # the drivers on top of it: every weight a row, the same digits
    table = mc.run_weights_matrix(H, L, [0, 7], 1000, prior=prior, distance=d, seed=2, max_iter=20, osd=True,
                                  device=bp.DEVICE)
    assert np.array_equal(table[1], host) and table[0, 0] == 1000 and table[0, 1] == 0 and table[0, 9] == 1000
    assert np.array_equal(mc.run_weights("[[72, 12, 6]]", [7], 1000, prior_p=0.02, seed=2, max_iter=20, osd=True,
                                         device=bp.DEVICE)[0], host)


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_counters_untouched():
    H, L, d = matrices()["72"]
    dec = fresh(H)
    lib = _lib.load()
    n = 72
    prior = mc.prior_of(0.02, n)
    Lc = np.ascontiguousarray(L, np.uint8)
    counters = np.full(12, 5, np.int64)

    def call(weight=3, begin=0, end=100, prior_ptr=prior.ctypes.data, flags=0, counters_ptr=counters.ctypes.data):
        return lib.qbp_mc_run_weight(dec._h, Lc.ctypes.data, Lc.shape[0], d, weight, 0, begin, end, prior_ptr, 20, 0,
                                     1.0, 1.0, 20.0, flags, counters_ptr)

    for what, kw, word in (("w = -1", dict(weight=-1), b"weight"), ("w = n + 1", dict(weight=n + 1), b"weight"),
                           ("null prior", dict(prior_ptr=None), b"null"),
                           ("negative trial_begin", dict(begin=-5), b"trial_begin"),
                           ("end < begin", dict(begin=10, end=5), b">= 0"),
                           ("a method bit without OSD0", dict(flags=_lib.FLAG_OSD_CS | (3 << 16)), b"QBP_FLAG_OSD0"),
                           ("too many trials with OSD", dict(end=_lib.MC_OSD_MAX_TRIALS + 1, flags=_lib.FLAG_OSD0),
                            b"at most")):
        assert call(**kw) == -1, what
        assert word in lib.qbp_last_error(), (what, lib.qbp_last_error())
        assert np.all(counters == 5), what
    assert call(counters_ptr=None) == -1
    errors = np.full((4, n), 9, np.uint8)
    for w in (-1, n + 1):
        assert lib.qbp_mc_sample_errors_weight(dec._h, w, 0, 0, 4, errors.ctypes.data) == -1
        assert b"weight" in lib.qbp_last_error()
    assert lib.qbp_mc_sample_errors_weight(dec._h, 3, 0, -1, 4, errors.ctypes.data) == -1
    assert lib.qbp_mc_sample_errors_weight(dec._h, 3, 0, 0, 4, None) == -1
    assert np.all(errors == 9)
    assert call(end=0) == 0 and np.all(counters == 5)        # (no trials: nothing changes)
    assert call() == 0 and counters[0] == 105                # (and a good call ADDS)


# ---- 6. end to end on a code small enough to enumerate ----------------------------------------------------------------------------
def test_stratified_ler_equals_bernoulli_ler_on_steane():
    """Steane's H with the all-ones logical, prior at p0 = 0.1, BP(20): the exact failure fraction of every weight
    from all C(7, w) patterns; the LER at p0 they give through ler_from_weights against a Bernoulli run of 10^6
    trials (5 sigma of its binomial error); and the sampled fractions of 20 000 trials per weight against the exact
    ones (5 sigma of theirs)."""
    H = codes.load_code("steane").Hx
    n, p0 = 7, 0.1
    assert H.shape[1] == n
    L = np.ones((1, n), np.uint8)
    prior = mc.prior_of(p0, n)
    dec = fresh(H)
    patterns = ((np.arange(128)[:, None] >> np.arange(n)) & 1).astype(np.uint8)
    exact = np.zeros((n + 1, mc.NUM_COUNTERS), np.int64)
    for w in range(n + 1):
        rows = patterns[patterns.sum(axis=1) == w]
        assert len(rows) == math.comb(n, w)
        exact[w] = dec.mc_run_errors(L, 3, rows, prior, max_iter=20)
        assert exact[w, 0] == len(rows)
    f = exact[:, 1] / exact[:, 0]
    print("exact f_w:", f)
    # No error is no failure.  H 1 = 0 (every check has weight 4), so an error and its complement share a syndrome and
    # a decoder output, and their residuals differ by the all-ones vector, whose parity is odd: exactly one of the two
    # is a logical error, f_w + f_(7-w) = 1.  (f_1 = 1 / 7, not 0: flooding BP at this prior answers the syndrome of
    # the weight-3 column with a weight-4 pattern in its first iteration, as the CPU oracle does.)
    assert f[0] == 0 and f[n] == 1
    assert np.array_equal(exact[:, 1] + exact[::-1, 1], exact[:, 0])
    est = mc.ler_from_weights(exact, list(range(n + 1)), n, [p0])
    assert est["unsampled_mass"][0] == 0
    ler = est["ler"][0]
    T = 1_000_000
    bern = dec.mc_run(L, 3, p0, prior, 0, T, seed=5, max_iter=20)
    sigma = math.sqrt(ler * (1 - ler) / T)
    print("stratified LER", ler, "Bernoulli", bern[1] / T, "5 sigma", 5 * sigma)
    assert bern[0] == T and abs(bern[1] / T - ler) <= 5 * sigma
    Tw = 20000
    for w in range(n + 1):
        got = dec.mc_run_weight(L, 3, w, prior, 0, Tw, seed=6, max_iter=20)
        s = math.sqrt(f[w] * (1 - f[w]) / Tw)
        print(f"w={w}: sampled {got[1] / Tw:.5f} exact {f[w]:.5f} 5 sigma {5 * s:.5f}")
        assert got[0] == Tw and abs(got[1] / Tw - f[w]) <= 5 * s
