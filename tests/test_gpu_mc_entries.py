"""GPU: the Monte-Carlo entry points against each other, in one table -- every comparison exact int64 equality.

  sampled = stored   a sampled entry's counters are qbp_mc_run_errors' on what the matching qbp_mc_sample_errors*
                     returns (a ladder: row by row, with that row's max_iter)
  host = device      a _device entry adds the host entry's answer to whatever its buffers held
  add / set          sampled entries ADD to the caller's counters, stored-error entries SET them (and zero them for T = 0)
  range splitting    [0, T) = [0, a) + [a, T)
  refusals           one bad argument per entry: -1, and a poisoned counters array stays as it was, host and device form

on Steane, [[72, 12, 6]] and [[72, 12, 6]] forced onto the general-H kernel, with draws 1 and 2, without and with OSD-0;
p and max_iter leave BP trials unconverged, so the OSD rows run the second kernel."""
import types

import numpy as np
import pytest

from qldpc_amd import _lib, bp, codes, mc

pytestmark = pytest.mark.gpu

T, SPLIT, SEED = 3000, 1237, 11
ENTRIES = ("run", "probs", "spectrum", "weight", "budgets")
GRID = [(draws, flags) for draws in (1, 2) for flags in (0, _lib.FLAG_OSD0)]
CASES = {"steane": ("steane", 0.2, 3, 3, False), "72": ("[[72, 12, 6]]", 0.06, 4, 7, False),
         "72-general": ("[[72, 12, 6]]", 0.06, 4, 7, True)}          # code, p, max_iter, weight, general-H kernel


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    name, p, max_iter, weight, general = CASES[request.param]
    code = codes.load_code(name)
    c = types.SimpleNamespace(name=request.param, H=code.Hx, p=p, max_iter=max_iter, weight=weight)
    c.n = code.Hx.shape[1]
    c.L, c.d = (np.ones((1, c.n), np.uint8), 3) if name == "steane" else (np.ascontiguousarray(code.Lx, np.uint8), code.distance)
    c.dec = _lib.Decoder(*bp.csr_from_H(code.Hx), bp.DEVICE)
    if general:
        c.dec.set_option(_lib.OPT_FORCE_GENERIC, 1)
    c.kernel = 2 if general else (1 if name != "steane" else None)
    c.prior = mc.prior_of(p, c.n)
    c.probs = np.full(c.n, p)
    c.budgets = sorted({1, max_iter - 1, max_iter})
    c.cache = {}
    return c


def host(c, entry, draws, flags, begin=0, end=T):
    """The host entry's answer for trials [begin, end): (counters,) or (counters, spectrum, iter_hist)."""
    key = (entry, draws, flags, begin, end)
    if key not in c.cache:
        kw = dict(seed=SEED, flags=flags)
        d = c.dec
        if entry == "run":
            out = (d.mc_run(c.L, c.d, c.p, c.prior, begin, end, draws=draws, max_iter=c.max_iter, **kw),)
        elif entry == "probs":
            out = (d.mc_run_probs(c.L, c.d, c.probs, c.prior, begin, end, draws=draws, max_iter=c.max_iter, **kw),)
        elif entry == "spectrum":
            out = d.mc_run_spectrum(c.L, c.d, c.probs, c.prior, begin, end, draws=draws, max_iter=c.max_iter, **kw)
        elif entry == "weight":
            out = (d.mc_run_weight(c.L, c.d, c.weight, c.prior, begin, end, max_iter=c.max_iter, **kw),)
        else:
            out = (d.mc_run_budgets(c.L, c.d, c.probs, c.prior, c.budgets, begin, end, draws=draws, **kw),)
        if c.kernel is not None:
            assert d.info("last_kernel") == c.kernel, key
        rows = out[0].reshape(-1, _lib.NUM_COUNTERS)
        assert np.all(rows[:, 0] == end - begin), key
        if flags & _lib.FLAG_OSD0 and end - begin == T:
            assert np.all(rows[:, 6] > 0), (key, rows[:, 6])        # BP left trials to the second kernel
        c.cache[key] = out
    return c.cache[key]


def sampled_errors(c, entry, draws):
    if entry == "run":
        return c.dec.mc_sample_errors(c.p, 0, T, draws=draws, seed=SEED)
    if entry == "weight":
        return c.dec.mc_sample_errors_weight(c.weight, 0, T, seed=SEED)
    return c.dec.mc_sample_errors_probs(c.probs, 0, T, draws=draws, seed=SEED)


@pytest.mark.parametrize("draws,flags", GRID)
def test_sampled_equals_stored(case, draws, flags):
    c = case
    for entry in ENTRIES:
        err = sampled_errors(c, entry, draws)
        got = host(c, entry, draws, flags)
        if entry == "budgets":
            for j, b in enumerate(c.budgets):
                want = c.dec.mc_run_errors(c.L, c.d, err, c.prior, max_iter=b, flags=flags)
                assert np.array_equal(got[0][j], want), (entry, b, got[0][j], want)
            continue
        want = c.dec.mc_run_errors(c.L, c.d, err, c.prior, max_iter=c.max_iter, flags=flags)
        assert np.array_equal(got[0], want), (entry, got[0], want)
        if entry == "spectrum":
            stored = c.dec.mc_run_errors_spectrum(c.L, c.d, err, c.prior, max_iter=c.max_iter, flags=flags)
            for g, w in zip(got, stored):
                assert g.dtype == np.int64 and np.array_equal(g, w), (entry, g, w)
            assert got[2].sum() == T and got[2][c.max_iter] == got[0][6]


@pytest.mark.parametrize("draws,flags", GRID)
def test_host_form_equals_device_form(case, draws, flags):
    import torch
    c = case
    dev = torch.device("cuda", bp.DEVICE)
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_prior = torch.from_numpy(c.prior).to(dev)
    kw = dict(seed=SEED, flags=flags, stream=stream)
    for entry in ENTRIES:
        want = host(c, entry, draws, flags)
        fill = [np.arange(7, 7 + a.size, dtype=np.int64).reshape(a.shape) for a in want]
        bufs = [torch.from_numpy(f.copy()).to(dev) for f in fill]
        ptr = [b.data_ptr() for b in bufs]
        if entry == "run":
            c.dec.mc_run_device(c.L, c.d, c.p, d_prior.data_ptr(), 0, T, ptr[0], draws=draws, max_iter=c.max_iter, **kw)
        elif entry == "probs":
            c.dec.mc_run_probs_device(c.L, c.d, c.probs, d_prior.data_ptr(), 0, T, ptr[0], draws=draws,
                                      max_iter=c.max_iter, **kw)
        elif entry == "spectrum":
            c.dec.mc_run_spectrum_device(c.L, c.d, c.probs, d_prior.data_ptr(), 0, T, ptr[0], ptr[1], ptr[2], draws=draws,
                                         max_iter=c.max_iter, **kw)
        elif entry == "weight":
            c.dec.mc_run_weight_device(c.L, c.d, c.weight, d_prior.data_ptr(), 0, T, ptr[0], max_iter=c.max_iter, **kw)
        else:
            c.dec.mc_run_budgets_device(c.L, c.d, c.probs, d_prior.data_ptr(), c.budgets, 0, T, ptr[0], draws=draws, **kw)
        torch.cuda.synchronize(dev)
        for b, f, w in zip(bufs, fill, want):
            assert np.array_equal(b.cpu().numpy(), f + w), (entry, b.cpu().numpy(), f, w)


def raw_args(c, flags=0, max_iter=None):
    """The decoder tail every raw call shares: max_iter, variant, alpha, damping, clip_llr, flags."""
    return (c.max_iter if max_iter is None else max_iter, _lib.SUM_PRODUCT, 1.0, 1.0, 20.0, flags)


@pytest.mark.parametrize("flags", [0, _lib.FLAG_OSD0])
def test_add_versus_set_through_the_raw_library(case, flags):
    c = case
    lib = _lib.load()
    once = host(c, "run", 1, flags)[0]
    cnt = np.zeros(_lib.NUM_COUNTERS, np.int64)
    for _ in range(2):
        assert lib.qbp_mc_run(c.dec._h, c.L.ctypes.data, c.L.shape[0], c.d, c.p, 1, SEED, 0, T, c.prior.ctypes.data,
                              *raw_args(c, flags), cnt.ctypes.data) == 0
    assert np.array_equal(cnt, 2 * once), (cnt, once)                       # sampled: added to
    err = sampled_errors(c, "run", 1)
    cnt[:] = 99
    for _ in range(2):
        assert lib.qbp_mc_run_errors(c.dec._h, c.L.ctypes.data, c.L.shape[0], c.d, err.ctypes.data, T,
                                     c.prior.ctypes.data, *raw_args(c, flags), cnt.ctypes.data) == 0
    assert np.array_equal(cnt, once), (cnt, once)                           # stored: set
    spec0, hist0 = host(c, "spectrum", 1, flags)[1:]
    spec = np.zeros_like(spec0)
    hist = np.zeros_like(hist0)
    cnt[:] = 99
    for _ in range(2):
        assert lib.qbp_mc_run_errors_spectrum(c.dec._h, c.L.ctypes.data, c.L.shape[0], c.d, err.ctypes.data, T,
                                              c.prior.ctypes.data, *raw_args(c, flags), cnt.ctypes.data,
                                              spec.ctypes.data, hist.ctypes.data) == 0
    assert np.array_equal(cnt, once)                                        # counters set,
    assert np.array_equal(spec, 2 * spec0) and np.array_equal(hist, 2 * hist0)   # the tables added to
    # no patterns: the counters are zeroed all the same, the tables stay
    cnt[:] = 99
    assert lib.qbp_mc_run_errors(c.dec._h, c.L.ctypes.data, c.L.shape[0], c.d, err.ctypes.data, 0, c.prior.ctypes.data,
                                 *raw_args(c, flags), cnt.ctypes.data) == 0
    assert np.all(cnt == 0)
    cnt[:] = 99
    assert lib.qbp_mc_run_errors_spectrum(c.dec._h, c.L.ctypes.data, c.L.shape[0], c.d, err.ctypes.data, 0,
                                          c.prior.ctypes.data, *raw_args(c, flags), cnt.ctypes.data, spec.ctypes.data,
                                          hist.ctypes.data) == 0
    assert np.all(cnt == 0) and np.array_equal(spec, 2 * spec0) and np.array_equal(hist, 2 * hist0)
    # and an empty sampled range adds nothing
    cnt[:] = 99
    assert lib.qbp_mc_run(c.dec._h, c.L.ctypes.data, c.L.shape[0], c.d, c.p, 1, SEED, 5, 5, c.prior.ctypes.data,
                          *raw_args(c, flags), cnt.ctypes.data) == 0
    assert np.all(cnt == 99)


@pytest.mark.parametrize("draws,flags", GRID)
def test_range_splitting(case, draws, flags):
    c = case
    for entry in ENTRIES:
        whole = host(c, entry, draws, flags)
        left, right = host(c, entry, draws, flags, 0, SPLIT), host(c, entry, draws, flags, SPLIT, T)
        for w, a, b in zip(whole, left, right):
            assert np.array_equal(w, a + b), (entry, w, a, b)


def test_refusals_leave_the_counters_untouched(case):
    """Each call: (entry, what is wrong); host form on a poisoned host array, device form on a poisoned device one."""
    import torch
    c = case
    lib = _lib.load()
    dev = torch.device("cuda", bp.DEVICE)
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_prior = torch.from_numpy(c.prior).to(dev)
    h, Lp, k, pr = c.dec._h, c.L.ctypes.data, c.L.shape[0], c.prior.ctypes.data
    bad_probs = c.probs.copy()
    bad_probs[c.n // 2] = 1.5
    down = np.asarray([5, 3], np.int32)
    good = np.asarray(c.budgets, np.int32)
    width = 2 * _lib.NUM_COUNTERS + _lib.SPECTRUM_ROWS * (c.n + 1) + 1026       # room for every entry's outputs
    POISON = -7777

    def calls(cnt, prior, tail):
        """name -> the call, for counters at address `cnt` (tables behind them) and the prior at `prior`; `tail`: ()
        for the host form, (stream,) for the device form."""
        dv = "_device" if tail else ""
        spec, hist = cnt + 8 * _lib.NUM_COUNTERS, cnt + 8 * (_lib.NUM_COUNTERS + _lib.SPECTRUM_ROWS * (c.n + 1))
        run, probs = getattr(lib, "qbp_mc_run" + dv), getattr(lib, "qbp_mc_run_probs" + dv)
        weight, budgets = getattr(lib, "qbp_mc_run_weight" + dv), getattr(lib, "qbp_mc_run_budgets" + dv)
        spectrum = getattr(lib, "qbp_mc_run_spectrum" + dv)
        a = raw_args(c, _lib.FLAG_OSD0)
        return {
            "run, p = 1.5": lambda: run(h, Lp, k, c.d, 1.5, 1, SEED, 0, T, prior, *a, cnt, *tail),
            "run, draws = 3": lambda: run(h, Lp, k, c.d, c.p, 3, SEED, 0, T, prior, *a, cnt, *tail),
            "probs, a prob of 1.5": lambda: probs(h, Lp, k, c.d, bad_probs.ctypes.data, 1, SEED, 0, T, prior, *a, cnt, *tail),
            "probs, draws = 3": lambda: probs(h, Lp, k, c.d, c.probs.ctypes.data, 3, SEED, 0, T, prior, *a, cnt, *tail),
            "weight = n + 1": lambda: weight(h, Lp, k, c.d, c.n + 1, SEED, 0, T, prior, *a, cnt, *tail),
            "spectrum, max_iter = 1025": lambda: spectrum(h, Lp, k, c.d, c.probs.ctypes.data, 1, SEED, 0, T, prior,
                                                          *raw_args(c, _lib.FLAG_OSD0, 1025), cnt, spec, hist, *tail),
            "spectrum, a prob of 1.5": lambda: spectrum(h, Lp, k, c.d, bad_probs.ctypes.data, 1, SEED, 0, T, prior, *a, cnt,
                                                        spec, hist, *tail),
            "budgets, descending": lambda: budgets(h, Lp, k, c.d, c.probs.ctypes.data, 1, SEED, 0, T, prior,
                                                   down.ctypes.data, 2, *a[1:], cnt, *tail),
            "budgets, draws = 3": lambda: budgets(h, Lp, k, c.d, c.probs.ctypes.data, 3, SEED, 0, T, prior,
                                                  good.ctypes.data, len(good), *a[1:], cnt, *tail),
        }

    cnt = np.full(width, POISON, np.int64)
    for what, call in calls(cnt.ctypes.data, pr, ()).items():
        assert call() == _lib.E_INVALID, ("host", what, lib.qbp_last_error())
        assert np.all(cnt == POISON), ("host", what)
    d_cnt = torch.full((width,), POISON, dtype=torch.int64, device=dev)
    for what, call in calls(d_cnt.data_ptr(), d_prior.data_ptr(), (stream,)).items():
        assert call() == _lib.E_INVALID, ("device", what, lib.qbp_last_error())
        torch.cuda.synchronize(dev)
        assert bool((d_cnt == POISON).all()), ("device", what)
    # stored errors: nothing about the patterns can be wrong but their number
    err = np.zeros((1, c.n), np.uint8)
    assert lib.qbp_mc_run_errors(h, Lp, k, c.d, err.ctypes.data, -1, pr, *raw_args(c), cnt.ctypes.data) == _lib.E_INVALID
    assert lib.qbp_mc_run_errors_spectrum(h, Lp, k, c.d, err.ctypes.data, 1, pr, *raw_args(c, 0, 1025), cnt.ctypes.data,
                                          cnt.ctypes.data + 96, cnt.ctypes.data + 96 + 32 * (c.n + 1)) == _lib.E_INVALID
    assert np.all(cnt == POISON)
    # a good call after all the refused ones: the handle is as it was
    assert np.array_equal(c.dec.mc_run(c.L, c.d, c.p, c.prior, 0, T, seed=SEED, max_iter=c.max_iter, flags=_lib.FLAG_OSD0),
                          host(c, "run", 1, _lib.FLAG_OSD0)[0])
