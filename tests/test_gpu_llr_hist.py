"""GPU: posterior-LLR histograms per iteration budget (qbp_mc_run_llr_hist).  No tolerance anywhere: the table equals the
numpy statement (tests/llr_hist_oracle.py: one oracle decode per budget, np.histogram itself) digit for digit, and the
counters equal qbp_mc_run_budgets.  tests/test_llr_hist_cpu.py shows that the inputs (tests/llr_hist_cases.py) reach
interior bins, both outer columns, the NaN column and values exactly on edges."""
import os

import numpy as np
import pytest

import llr_hist_cases as cases
from llr_hist_oracle import llr_hist, llr_hist_of_errors
from qldpc_amd import _lib, bp, codes, mc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OSD_CS7 = _lib.osd_flags("cs", 7)


def decoder(c, **options):
    dec = _lib.Decoder(*bp.csr_from_H(c.H), bp.DEVICE)
    for opt, value in options.items():
        dec.set_option(getattr(_lib, opt), value)
    return dec


def run(dec, c, flags=0, bins=None, llr_range=None, budgets=None, begin=0, end=None, hist=None):
    probs = c.probs
    return dec.mc_run_llr_hist(c.L, c.distance, probs, c.prior, budgets or c.budgets, bins or c.bins, llr_range or c.range,
                               begin, c.T if end is None else end, seed=c.seed, flags=flags, hist=hist, **c.kw)


def check(dec, c, name, flags=0, kernel=None, **kw):
    """Table == statement, counters == qbp_mc_run_budgets, and the three identities."""
    cnt, hist = run(dec, c, flags, **kw)
    if kernel is not None:
        assert dec.info("last_kernel") == kernel
    want = cases.statement(name, kw.get("bins"), kw.get("llr_range"), kw.get("budgets"))
    budgets = kw.get("budgets") or c.budgets
    print(name, flags, kw, "unconverged values", hist[:, 2:].sum(axis=(1, 2)).tolist(), "NaN", int(hist[:, :, -1].sum()))
    assert hist.shape == want.shape and np.array_equal(hist, want), np.argwhere(hist != want)[:10]
    ladder = dec.mc_run_budgets(c.L, c.distance, c.probs, c.prior, budgets, 0, c.T, seed=c.seed, flags=flags, **c.kw)
    assert np.array_equal(cnt, ladder), (cnt, ladder)
    n = c.H.shape[1]
    assert (hist.sum(axis=(1, 2)) == n * cnt[:, 0]).all() and (hist[:, 2:].sum(axis=(1, 2)) == n * cnt[:, 6]).all()
    assert len(set((hist[:, 1] + hist[:, 3]).sum(axis=1).tolist())) == 1
    return cnt, hist


@pytest.mark.parametrize("name", ["steane", "72", "72_minsum", "zero_lo_hi", "zero_edge_lo", "dem72", "inf_nan"])
def test_on_chip_builds(name):
    """Steane (padded rows), [[72,12,6]] sum-product and damped min-sum on the (6, 3) build, two columns without a check
    whose priors sit exactly on edges, a three-round space-time matrix on the (8, 4) build, a +inf prior and NaN."""
    c = cases.case(name)
    dec = decoder(c)
    check(dec, c, name, kernel=1)
    dec.close()


def test_osd_bits_do_not_change_the_table():
    c = cases.case("72")
    dec = decoder(c)
    base = check(dec, c, "72")[1]
    for flags in (_lib.FLAG_OSD0, OSD_CS7):
        cnt, hist = check(dec, c, "72", flags=flags)
        assert np.array_equal(hist, base) and cnt[0, 6] > 0
    dec.close()


def test_fast_math_against_the_device_decoder():
    """QBP_FLAG_FAST_MATH: the statement fed the device's own qbp_decode_batch LLRs under the same flag."""
    c = cases.case("72")
    dec = decoder(c)
    fast = _lib.FLAG_FAST_MATH

    def decode(syndromes, max_iter):
        return dec.decode(syndromes, c.prior, max_iter, flags=fast)

    want = llr_hist(c.H, c.probs, c.prior, 0, c.T, c.budgets, c.bins, *c.range, seed=c.seed, decode=decode)
    cnt, hist = run(dec, c, flags=fast)
    assert np.array_equal(hist, want), np.argwhere(hist != want)[:10]
    assert np.array_equal(cnt, dec.mc_run_budgets(c.L, c.distance, c.probs, c.prior, c.budgets, 0, c.T, seed=c.seed, flags=fast))
    dec.close()


@pytest.mark.parametrize("mem", [0, 1, 2])
@pytest.mark.parametrize("name", ["rand37", "rand37_minsum"])
def test_general_kernel_memory_modes(name, mem):
    c = cases.case(name)
    dec = decoder(c, OPT_GENERAL_MEM=mem)
    check(dec, c, name, kernel=2)
    check(dec, c, name, flags=_lib.FLAG_OSD0, kernel=2)
    dec.close()


@pytest.mark.parametrize("bins,budgets", [(1, cases.LADDER), (128, cases.LADDER), (2045, (4,)), (679, cases.LADDER)])
def test_bin_counts_up_to_the_cap(bins, budgets):
    c = cases.case("72")
    assert bins <= 128 or bins == _lib.LLR_HIST_MAX_WORDS // (4 * len(budgets)) - 3        # (the largest the cap allows)
    dec = decoder(c)
    check(dec, c, "72", bins=bins, budgets=budgets, kernel=1)
    gen = decoder(c, OPT_FORCE_GENERIC=1)
    check(gen, c, "72", bins=bins, budgets=budgets, kernel=2)
    dec.close(), gen.close()


def test_more_trials_than_one_pass_of_the_grid_and_launch_chunks():
    """Two slots per workgroup, one workgroup per CU: every slot decodes several trials; then the launches of
    QBP_OPT_LLR_HIST_CHUNK (several per call, sampled and stored errors)."""
    c = cases.case("72")
    dec = decoder(c, OPT_SLOTS_PER_BLOCK=2, OPT_BLOCKS_PER_CU=1)
    assert dec.info("num_cu") * 2 < c.T
    base = check(dec, c, "72", kernel=1)
    dec.set_option(_lib.OPT_LLR_HIST_CHUNK, 333)
    for flags in (0, _lib.FLAG_OSD0):
        cnt, hist = run(dec, c, flags=flags)
        assert np.array_equal(hist, base[1]) and np.array_equal(cnt[:, [0, 6, 7]], base[0][:, [0, 6, 7]])
    g = np.load(os.path.join(HERE, "golden", "llr_hist.npz"))
    errors = np.unpackbits(g["errors"], axis=1)[:, :72]
    prior = mc.prior_of(float(g["p"]), 72)
    args = (c.L, c.distance, errors, prior, g["limits"], int(g["bins"]), tuple(g["range"]))
    chunked = dec.mc_run_errors_llr_hist(*args)
    dec.set_option(_lib.OPT_LLR_HIST_CHUNK, 0)
    whole = dec.mc_run_errors_llr_hist(*args)
    assert np.array_equal(chunked[0], whole[0]) and np.array_equal(chunked[1], whole[1])
    small = cases.case("rand37")
    gen = decoder(small, OPT_BLOCKS_PER_CU=1, OPT_LLR_HIST_CHUNK=701)
    assert gen.info("num_cu") < small.T
    check(gen, small, "rand37", kernel=2)
    dec.close(), gen.close()


def test_stored_errors_entry_gives_the_reference_counts():
    """The fixture of tests/golden/make_golden_llr_hist.py: the reference's own lists, binned by np.histogram."""
    g = np.load(os.path.join(HERE, "golden", "llr_hist.npz"))
    code = codes.load_code(str(g["code"]))
    errors = np.unpackbits(g["errors"], axis=1)[:, :code.n]
    bins, (lo, hi) = int(g["bins"]), (float(x) for x in g["range"])
    prior = mc.prior_of(float(g["p"]), code.n)
    dec = bp.decoder_for(code.Hx)
    for flags in (0, _lib.FLAG_OSD0):
        cnt, hist = dec.mc_run_errors_llr_hist(code.Lx, code.distance, errors, prior, g["limits"], bins, (lo, hi), flags=flags)
        sums = np.stack([hist.sum(axis=1), hist[:, 2] + hist[:, 3], hist[:, 0] + hist[:, 2], hist[:, 1] + hist[:, 3]], axis=1)
        assert np.array_equal(sums[:, :, 1:bins + 1], g["counts"])
        assert np.array_equal(sums[:, :, 0], g["outside"][:, :, 0]) and np.array_equal(sums[:, :, bins + 1], g["outside"][:, :, 1])
        assert np.array_equal(hist, llr_hist_of_errors(code.Hx, errors, prior, g["limits"], bins, lo, hi))
        assert (cnt[:, 0] == len(errors)).all() and (hist[:, 2:].sum(axis=(1, 2)) == code.n * cnt[:, 6]).all()
        for j, b in enumerate(g["limits"]):        # counters SET: those of qbp_mc_run_errors at that limit
            assert np.array_equal(cnt[j], dec.mc_run_errors(code.Lx, code.distance, errors, prior, max_iter=int(b), flags=flags))


def test_added_to_split_grid_and_stream_independence():
    import torch
    c = cases.case("72")
    dec = decoder(c)
    cnt, hist = check(dec, c, "72")
    # ADDED to a pre-filled table
    fill = np.arange(hist.size, dtype=np.int64).reshape(hist.shape) * 3 + 11
    again = run(dec, c, hist=fill.copy())[1]
    assert np.array_equal(again - fill, hist)
    # two ranges into one table
    acc = np.zeros_like(hist)
    a = 777
    parts = run(dec, c, end=a, hist=acc)[0] + run(dec, c, begin=a, hist=acc)[0]
    assert np.array_equal(acc, hist) and np.array_equal(parts, cnt)
    # another grid
    for slots, per_cu in ((1, 1), (5, 3)):
        other = decoder(c, OPT_SLOTS_PER_BLOCK=slots, OPT_BLOCKS_PER_CU=per_cu)
        got = run(other, c)
        assert np.array_equal(got[1], hist) and np.array_equal(got[0], cnt)
        other.close()
    # the _device entry on torch buffers, on a side stream, in two ranges; and the sharded driver
    dev = torch.device("cuda", bp.DEVICE)
    K = len(c.budgets)
    d_out = torch.zeros(K * 12 + hist.size, dtype=torch.int64, device=dev)
    d_prior = torch.from_numpy(c.prior).to(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for lo, hi in ((0, a), (a, c.T)):
            dec.mc_run_llr_hist_device(c.L, c.distance, c.probs, d_prior.data_ptr(), c.budgets, c.bins, c.range, lo, hi,
                                       d_out.data_ptr(), d_out.data_ptr() + 8 * K * 12, seed=c.seed,
                                       stream=side.cuda_stream)
    side.synchronize()
    got = mc._split_llr_hist(d_out.cpu().numpy(), K, c.bins)
    assert np.array_equal(got[0], cnt) and np.array_equal(got[1], hist)
    d_cnt, d_hist, edges = mc.run_llr_hist("[[72, 12, 6]]", c.probs, c.T, c.budgets, c.bins, c.range, seed=c.seed)
    assert np.array_equal(d_cnt, cnt) and np.array_equal(d_hist, hist) and np.array_equal(edges, np.linspace(*c.range, c.bins + 1))
    dist = mc.llr_distributions("[[72, 12, 6]]", c.probs, c.T, c.budgets[-1], c.bins, c.range, seed=c.seed)
    assert np.array_equal(dist["true_1"], hist[-1, 1] + hist[-1, 3]) and np.array_equal(dist["true_0"], hist[-1, 0] + hist[-1, 2])
    dec.close()


def test_every_refusal_leaves_the_outputs_untouched():
    c = cases.case("72")
    dec = decoder(c)
    lib = _lib.load()
    n = c.H.shape[1]
    Lx = np.ascontiguousarray(c.L, np.uint8)
    probs = np.full(n, 0.06)
    cfill = np.arange(16 * 12, dtype=np.int64) + 5
    hfill = np.arange(_lib.LLR_HIST_MAX_WORDS + 64, dtype=np.int64) * 7 + 3

    def call(budgets=(2, 5), bins=16, lo=-5.0, hi=5.0, flags=0, hist=True, stored=False):
        bud = np.asarray(budgets, np.int32)
        counters, table = cfill.copy(), hfill.copy()
        tail = (0, 1.0, 1.0, 20.0, flags, lo, hi, bins, counters.ctypes.data, table.ctypes.data if hist else None)
        if stored:
            errors = np.zeros((10, n), np.uint8)
            rc = lib.qbp_mc_run_errors_llr_hist(dec._h, Lx.ctypes.data, Lx.shape[0], c.distance, errors.ctypes.data, 10,
                                                c.prior.ctypes.data, bud.ctypes.data, len(bud), *tail)
        else:
            rc = lib.qbp_mc_run_llr_hist(dec._h, Lx.ctypes.data, Lx.shape[0], c.distance, probs.ctypes.data, 1, 0, 0, 500,
                                         c.prior.ctypes.data, bud.ctypes.data, len(bud), *tail)
        assert rc != 0 or np.array_equal(counters[24:], cfill[24:])
        if rc != 0:
            assert np.array_equal(counters, cfill) and np.array_equal(table, hfill)
        return rc

    assert call() == 0 and call(stored=True) == 0
    for stored in (False, True):
        assert call(hist=False, stored=stored) == -1 and b"hist" in lib.qbp_last_error()
        assert call(bins=0, stored=stored) == -1 and call(bins=-4, stored=stored) == -1
        assert call(lo=1.0, hi=1.0, stored=stored) == -1 and call(lo=2.0, hi=1.0, stored=stored) == -1
        for bad in (np.inf, -np.inf, np.nan):
            assert call(lo=bad, stored=stored) == -1 and call(hi=bad, stored=stored) == -1
        assert call(budgets=(4,), bins=2046, stored=stored) == -1 and b"QBP_LLR_HIST_MAX_WORDS" in lib.qbp_last_error()
        assert call(bins=1022, stored=stored) == -1 and call(budgets=tuple(range(1, 17)), bins=126, stored=stored) == -1
        assert call(budgets=(5, 5), stored=stored) == -1 and call(budgets=(0, 5), stored=stored) == -1   # as the ladder
        assert call(flags=_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS, stored=stored) == -1
        assert call(flags=_lib.FLAG_RELAY, stored=stored) != 0
    assert call(budgets=(4,), bins=2045) == 0
    with pytest.raises(ValueError):
        dec.mc_run_llr_hist(c.L, c.distance, 0.06, c.prior, (2, 5), 16, (3.0, 3.0), 0, 100)
    with pytest.raises(_lib.QbpError) as e:                  # the _device entry: before any launch
        dec.mc_run_llr_hist_device(c.L, c.distance, np.full(n, 1.5), 0, (5, 6), 8, (-1.0, 1.0), 0, 1000, 0, 0)
    assert e.value.code == -1
    dec.close()
