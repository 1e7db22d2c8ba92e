"""GPU: exhaustive weight-w enumeration (qbp_mc_run_enum, qbp_enum_failures) -- the device filler against
itertools.combinations bit for bit (tests/enum_oracle.py), the counters against the stored-errors pipeline fed the
oracle's rows, split / chunk / stream invariance, the captured failing patterns against the numpy statement (the CPU
oracle's BP and OSD-0, then the kind rule), and the refusals."""
import functools
import math

import numpy as np
import pytest

import enum_oracle
from oracle import oracle
from qldpc_amd import _lib, bp, codes, enumerate as en, mc
from test_gpu_weight import fresh, matrices

pytestmark = pytest.mark.gpu

OSD_CS7 = _lib.osd_flags("cs", 7)
ITERS = 20
# The prior of the capture and stage tests, chosen on the CPU with the oracle (tests/enum_oracle.py: kinds_of) so that
# both kinds occur.  Weight 3, BP(20), prior of p = 0.05, patterns by kind 0 / 1 / 2 / 3:
#   [[72,12,6]] (59 640):   BP alone 57528 / 720 / 129 / 1263,  with OSD-0 57528 / 720 / 1056 / 336
#   the 20 x 37 matrix (7770): BP alone 3798 / 45 / 625 / 3302,  with OSD-0 3798 / 45 / 2403 / 1524
PRIOR_P = 0.05


@functools.lru_cache(maxsize=None)
def rows_of(name, w):
    n = matrices()[name][0].shape[1]
    rows = enum_oracle.patterns(n, w)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def statement(name, osd):
    """kinds uint8[C(n, 3)] of the whole weight-3 class by the CPU oracle."""
    H, L, _ = matrices()[name]
    kinds = enum_oracle.kinds_of(H, L, rows_of(name, 3), mc.prior_of(PRIOR_P, H.shape[1]), ITERS, osd=osd)[0]
    kinds.setflags(write=False)
    return kinds


# ---- 1. the filler, bit for bit ------------------------------------------------------------------------------------------
def test_filler_steane_every_class():
    dec = fresh(matrices()["steane"][0])
    for w in range(8):
        got = dec.mc_sample_errors_enum(w, 0, math.comb(7, w))
        assert np.array_equal(got, enum_oracle.patterns(7, w)), w


def test_filler_72():
    dec = fresh(matrices()["72"][0])
    for w in (0, 1, 2, 3, 71, 72):
        C = math.comb(72, w)
        assert C <= 59640
        got = dec.mc_sample_errors_enum(w, 0, C)
        assert np.array_equal(got.sum(axis=1), np.full(C, w))
        assert np.array_equal(got, rows_of("72", w)), w
    T = 257
    for w in (3, 69):
        C = math.comb(72, w)
        for begin in (0, 1000, C - T):
            assert np.array_equal(dec.mc_sample_errors_enum(w, begin, T), enum_oracle.patterns(72, w, begin, T)), (w, begin)


def test_filler_irregular_whole_class():
    dec = fresh(matrices()["rand37"][0])
    got = dec.mc_sample_errors_enum(3, 0, 7770)
    assert np.array_equal(got, rows_of("rand37", 3))


def test_filler_crosses_the_32_bit_boundary_of_the_rank():
    n, w, T = 288, 5, 300
    begin = 2 ** 32 - 150
    dec = fresh(codes.load_code("[[288, 12, 18]]").Hx)
    got = dec.mc_sample_errors_enum(w, begin, T)
    want = enum_oracle.rows_of(n, [enum_oracle.unrank_int(n, w, begin + b) for b in range(T)])
    assert np.array_equal(got, want)
    assert np.array_equal(got, en.patterns(n, w, range(begin, begin + T)))
    last = math.comb(n, w) - 1
    assert np.array_equal(dec.mc_sample_errors_enum(w, last, 1), enum_oracle.rows_of(n, [[283, 284, 285, 286, 287]]))


def test_filler_clears_a_reused_buffer():
    dec = fresh(matrices()["72"][0])
    T = 257
    first = dec.mc_sample_errors_enum(12, 5000, T)
    assert np.array_equal(first.sum(axis=1), np.full(T, 12))
    assert np.array_equal(first, en.patterns(72, 12, range(5000, 5000 + T)))
    second = dec.mc_sample_errors_enum(2, 0, T)          # (same handle, same buffer, same size; another table)
    assert np.array_equal(second, enum_oracle.patterns(72, 2, 0, T))


# ---- 2. the counters: those of the stored-errors pipeline on the oracle's rows ----------------------------------------------
@pytest.mark.parametrize("mode", ["on_chip", "generic", "osd0", "cs7", "min_sum"])
def test_counters_equal_stored_errors_pipeline_72(mode):
    H, L, d = matrices()["72"]
    prior = mc.prior_of(PRIOR_P, 72)
    dec = fresh(H)
    kw = dict(max_iter=ITERS)
    if mode == "generic":
        dec.set_option(_lib.OPT_FORCE_GENERIC, 1)
    elif mode == "osd0":
        kw["flags"] = _lib.FLAG_OSD0
    elif mode == "cs7":
        kw["flags"] = OSD_CS7
    elif mode == "min_sum":
        kw.update(variant=_lib.MIN_SUM, alpha=0.8)
    for w in (2, 3):
        C = math.comb(72, w)
        got = dec.mc_run_enum(L, d, w, prior, 0, C, **kw)
        assert dec.info("last_kernel") == (2 if mode == "generic" else 1)
        want = dec.mc_run_errors(L, d, rows_of("72", w), prior, **kw)
        print(mode, w, dict(zip(_lib.COUNTER_NAMES, got.tolist())))
        assert got[0] == C
        assert np.array_equal(got, want), (mode, w, got, want)
        assert (got[3], got[4]) == ((got[1], 0) if w < d // 2 else (0, got[1]))


def test_counters_equal_stored_errors_pipeline_irregular():
    H, L, d = matrices()["rand37"]
    prior = mc.prior_of(PRIOR_P, 37)
    dec = fresh(H)
    got = dec.mc_run_enum(L, d, 3, prior, 0, 7770, max_iter=ITERS, flags=_lib.FLAG_OSD0)
    assert dec.info("last_kernel") == 2
    assert got[0] == 7770 and got[6] > 0
    assert np.array_equal(got, dec.mc_run_errors(L, d, rows_of("rand37", 3), prior, max_iter=ITERS, flags=_lib.FLAG_OSD0))


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _lib.FLAG_OSD0], ids=["bp", "osd0"])
def test_split_and_chunk_invariance(flags):
    H, L, d = matrices()["72"]
    prior = mc.prior_of(PRIOR_P, 72)
    kw = dict(max_iter=ITERS, flags=flags)
    w, C = 2, 2556
    dec = fresh(H)
    whole = dec.mc_run_enum(L, d, w, prior, 0, C, **kw)
    assert whole[0] == C
    for a in (1, 1000, C - 1):
        assert np.array_equal(dec.mc_run_enum(L, d, w, prior, 0, a, **kw) + dec.mc_run_enum(L, d, w, prior, a, C, **kw), whole), a
    for chunk in (1, 97, 4096):           # (2556 chunks of one pattern; a last chunk of 34; one chunk)
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, chunk)
        assert np.array_equal(dec.mc_run_enum(L, d, w, prior, 0, C, **kw), whole), chunk
    dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)
    assert np.array_equal(dec.mc_run_enum(L, d, w, prior, 7, 7, **kw), np.zeros(12, np.int64))


def test_device_form_on_its_own_stream_adds_to_counters():
    import torch
    H, L, d = matrices()["72"]
    prior = mc.prior_of(PRIOR_P, 72)
    dec = fresh(H)
    dev = torch.device("cuda", bp.DEVICE)
    start = np.arange(100, 112, dtype=np.int64)
    d_cnt = torch.from_numpy(start.copy()).to(dev)
    d_prior = torch.from_numpy(prior).to(dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    for a, b in ((0, 20000), (20000, 59640)):
        dec.mc_run_enum_device(L, d, 3, d_prior.data_ptr(), a, b, d_cnt.data_ptr(), max_iter=ITERS, flags=_lib.FLAG_OSD0,
                               stream=stream.cuda_stream)
    stream.synchronize()
    host = dec.mc_run_enum(L, d, 3, prior, 0, 59640, max_iter=ITERS, flags=_lib.FLAG_OSD0)
    assert np.array_equal(d_cnt.cpu().numpy(), start + host)
    # the drivers on top of it: every weight a row with [0] = C(n, w), the same digits
    table = mc.run_enumerate_matrix(H, L, [0, 3], prior=prior, distance=d, max_iter=ITERS, osd=True, device=bp.DEVICE)
    assert np.array_equal(table[1], host) and table[0, 0] == 1 and table[0, 1] == 0 and table[0, 9] == 1
    assert np.array_equal(mc.run_enumerate("[[72, 12, 6]]", [3], prior_p=PRIOR_P, max_iter=ITERS, osd=True,
                                           device=bp.DEVICE)[0], host)
    est = mc.ler_from_weights(table, [0, 3], 72, [0.001], exact_weights=[0, 3])
    assert est["stderr"][0] == 0 and est["ler"][0] > 0


# ---- 4. Steane, every pattern ------------------------------------------------------------------------------------------------
def test_steane_table_equals_the_oracle():
    H, L, d = matrices()["steane"]
    n, p0 = 7, 0.1
    prior = mc.prior_of(p0, n)
    table = mc.run_enumerate_matrix(H, L, list(range(8)), prior=prior, distance=d, max_iter=ITERS, device=bp.DEVICE)
    assert [int(x) for x in table[:, 0]] == [math.comb(7, w) for w in range(8)]
    for w in range(8):
        rows = enum_oracle.patterns(7, w)
        syn = (rows.astype(np.int64) @ np.asarray(H).astype(np.int64).T % 2).astype(np.uint8)
        hard, conv, iters, _ = oracle.decode_batch(H, syn, prior, ITERS)
        want = oracle.classify_trials(H, L, d, rows, syn, hard, conv, iters)
        assert table[w, 1] == want[1] and table[w, 6] == want[6], (w, table[w], want)
    assert table[:, 0].sum() == 128
    est = mc.ler_from_weights(table, list(range(8)), n, [p0], exact_weights=list(range(8)))
    assert est["unsampled_mass"][0] == 0 and est["stderr"][0] == 0


# ---- 5. the failing patterns ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72", "rand37"])
@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
def test_capture_equals_the_statement(name, osd):
    H, L, d = matrices()[name]
    n = H.shape[1]
    C = math.comb(n, 3)
    prior = mc.prior_of(PRIOR_P, n)
    kinds = statement(name, osd)
    counts = np.bincount(kinds, minlength=4)
    print(name, "osd" if osd else "bp", "patterns by kind", counts.tolist())
    assert counts[1] + counts[3] >= 1 and counts[2] + counts[3] >= 1        # (both kinds occur)
    flags = _lib.FLAG_OSD0 if osd else 0
    dec = fresh(H)
    run = dec.mc_run_enum(L, d, 3, prior, 0, C, max_iter=ITERS, flags=flags)
    for what in (1, 2, 3):
        want = np.flatnonzero(kinds & what)
        ranks, got_kinds, found, cnt = dec.enum_failures(L, 3, prior, 0, C, what=what, cap=C, max_iter=ITERS, flags=flags)
        assert dec.info("last_kernel") == (2 if name == "rand37" else 1)
        assert found == len(want) == len(ranks)
        assert np.array_equal(ranks, want) and ranks.dtype == np.int64          # (ascending: found <= cap)
        assert np.array_equal(got_kinds, kinds[want])
        assert found == (cnt[1], cnt[6], found)[what - 1]
        assert cnt[0] == C and all(cnt[i] == run[i] for i in (0, 1, 6)), (cnt, run)
        assert all(cnt[i] == 0 for i in (2, 3, 4, 5, 9, 11))
    # (the patterns themselves, from their ranks)
    assert np.array_equal(en.patterns(n, 3, ranks[:50]), rows_of(name, 3)[ranks[:50]])


def test_capture_cap_sentinels_split_and_chunk():
    H, L, d = matrices()["72"]
    C = 59640
    prior = mc.prior_of(PRIOR_P, 72)
    kinds = statement("72", True)
    want = np.flatnonzero(kinds & 3)
    lib = _lib.load()
    dec = fresh(H)
    Lc = np.ascontiguousarray(L, np.uint8)

    def raw(begin, end, what, cap, ranks, knd, found, counters):
        return lib.qbp_enum_failures(dec._h, Lc.ctypes.data, Lc.shape[0], 3, begin, end, prior.ctypes.data, ITERS, 0, 1.0,
                                     1.0, 20.0, _lib.FLAG_OSD0, what, cap, None if ranks is None else ranks.ctypes.data,
                                     None if knd is None else knd.ctypes.data, found.ctypes.data, counters.ctypes.data)

    # cap < found: found unchanged, the kept entries distinct members of the full set with their kinds, the rest untouched
    cap = 100
    ranks, knd = np.full(cap + 50, -7, np.int64), np.full(cap + 50, 0xEE, np.uint8)
    found, counters = np.full(1, -7, np.int64), np.zeros(12, np.int64)
    assert raw(0, C, 3, cap, ranks, knd, found, counters) == 0
    assert found[0] == len(want) > cap
    assert len(set(ranks[:cap].tolist())) == cap and np.all(np.isin(ranks[:cap], want))
    assert np.array_equal(knd[:cap], kinds[ranks[:cap]])
    assert np.all(ranks[cap:] == -7) and np.all(knd[cap:] == 0xEE)
    # cap = 0 with null arrays: a count
    found[0] = -7
    assert raw(0, C, 3, 0, None, None, found, counters) == 0 and found[0] == len(want)
    assert counters[0] == 2 * C                                          # (ADDED to)
    # cap > found: nothing beyond found is written
    few = np.flatnonzero(kinds[:3000] & 1)
    ranks[:], knd[:] = -7, 0xEE
    assert raw(0, 3000, 1, len(ranks), ranks, knd, found, counters) == 0
    assert found[0] == len(few) and 0 < len(few) < len(ranks)
    assert np.array_equal(ranks[:len(few)], few) and np.all(ranks[len(few):] == -7) and np.all(knd[len(few):] == 0xEE)
    # the split of the range, and the chunk
    whole = dec.enum_failures(L, 3, prior, 0, C, what=3, cap=C, max_iter=ITERS, flags=_lib.FLAG_OSD0)
    assert np.array_equal(whole[0], want)
    a = 20001
    lo = dec.enum_failures(L, 3, prior, 0, a, what=3, cap=C, max_iter=ITERS, flags=_lib.FLAG_OSD0)
    hi = dec.enum_failures(L, 3, prior, a, C, what=3, cap=C, max_iter=ITERS, flags=_lib.FLAG_OSD0)
    assert np.array_equal(np.concatenate([lo[0], hi[0]]), whole[0]) and np.array_equal(np.concatenate([lo[1], hi[1]]), whole[1])
    assert lo[2] + hi[2] == whole[2] and np.array_equal(lo[3] + hi[3], whole[3])
    for chunk in (97, 4096):
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, chunk)
        begin, end = (30000, 33000) if chunk == 97 else (0, C)
        got = dec.enum_failures(L, 3, prior, begin, end, what=3, cap=C, max_iter=ITERS, flags=_lib.FLAG_OSD0)
        sel = want[(want >= begin) & (want < end)]
        assert np.array_equal(got[0], sel) and np.array_equal(got[1], kinds[sel]) and got[2] == len(sel), chunk
    dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 0)


def test_capture_device_form_adds_to_found():
    import torch
    H, L, d = matrices()["72"]
    C = 59640
    prior = mc.prior_of(PRIOR_P, 72)
    kinds = statement("72", False)
    want = np.flatnonzero(kinds & 2)
    dec = fresh(H)
    dev = torch.device("cuda", bp.DEVICE)
    d_prior = torch.from_numpy(prior).to(dev)
    d_ranks = torch.full((len(want) + 10,), -7, dtype=torch.int64, device=dev)
    d_kinds = torch.full((len(want) + 10,), 0xEE, dtype=torch.uint8, device=dev)
    d_found = torch.zeros(1, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    for a, b in ((0, 25000), (25000, C)):
        dec.enum_failures_device(L, 3, d_prior.data_ptr(), a, b, 2, len(d_ranks), d_ranks.data_ptr(), d_kinds.data_ptr(),
                                 d_found.data_ptr(), d_cnt.data_ptr(), max_iter=ITERS, stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_found.item()) == len(want)
    ranks, knd = d_ranks.cpu().numpy(), d_kinds.cpu().numpy()
    order = np.argsort(ranks[:len(want)])
    assert np.array_equal(ranks[:len(want)][order], want) and np.array_equal(knd[:len(want)][order], kinds[want])
    assert np.all(ranks[len(want):] == -7) and np.all(knd[len(want):] == 0xEE)
    cnt = d_cnt.cpu().numpy()
    assert cnt[0] == C and cnt[6] == len(want)


def test_failing_patterns_returns_columns():
    H, L, _ = matrices()["rand37"]
    kinds = statement("rand37", True)
    out = en.failing_patterns(H, L, 3, prior=mc.prior_of(PRIOR_P, 37), what="logical", max_iter=ITERS, osd=True,
                              device=bp.DEVICE)
    want = np.flatnonzero(kinds & 1)
    assert out["found"] == len(want) and np.array_equal(out["ranks"], want) and np.array_equal(out["kinds"], kinds[want])
    assert out["columns"].shape == (len(want), 3)
    rows = rows_of("rand37", 3)[want]
    assert all(np.array_equal(np.flatnonzero(r), c) for r, c in zip(rows, out["columns"]))
    assert out["counters"][0] == 7770 and out["counters"][1] == len(want)
    with pytest.raises(ValueError):
        en.failing_patterns(H, L, 3, prior=mc.prior_of(PRIOR_P, 37), what="neither")


# ---- 6. refusals: host only, outputs untouched --------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    H, L, d = matrices()["72"]
    dec = fresh(H)
    big = fresh(codes.load_code("[[288, 12, 18]]").Hx)
    L288 = np.ascontiguousarray(codes.load_code("[[288, 12, 18]]").Lx, np.uint8)
    lib = _lib.load()
    n, C = 72, 59640
    prior = mc.prior_of(PRIOR_P, n)
    prior288 = mc.prior_of(PRIOR_P, 288)
    Lc = np.ascontiguousarray(L, np.uint8)
    counters = np.full(12, 5, np.int64)
    ranks, kinds, found = np.full(8, 5, np.int64), np.full(8, 5, np.uint8), np.full(1, 5, np.int64)
    errors = np.full((4, n), 9, np.uint8)

    def run(weight=3, begin=0, end=100, flags=0, h=dec, Lm=Lc, pr=prior):
        return lib.qbp_mc_run_enum(h._h, Lm.ctypes.data, Lm.shape[0], d, weight, begin, end, pr.ctypes.data, ITERS, 0, 1.0,
                                   1.0, 20.0, flags, counters.ctypes.data)

    def fail(weight=3, begin=0, end=100, flags=0, what=1, cap=8, found_ptr=found.ctypes.data, ranks_ptr=ranks.ctypes.data,
             h=dec, Lm=Lc, pr=prior):
        return lib.qbp_enum_failures(h._h, Lm.ctypes.data, Lm.shape[0], weight, begin, end, pr.ctypes.data, ITERS, 0, 1.0,
                                     1.0, 20.0, flags, what, cap, ranks_ptr, kinds.ctypes.data, found_ptr,
                                     counters.ctypes.data)

    def sample(weight=3, begin=0, T=4, h=dec):
        return lib.qbp_mc_sample_errors_enum(h._h, weight, begin, T, errors.ctypes.data)

    shared = (("w = -1", dict(weight=-1)), ("w = n + 1", dict(weight=n + 1)), ("rank_end = C + 1", dict(end=C + 1)),
              ("rank_begin < 0", dict(begin=-1)), ("end < begin", dict(begin=10, end=5)),
              ("C(288, 40) beyond 2^62", dict(weight=40, h=big, Lm=L288, pr=prior288)))
    for fn in (run, fail):
        for what, kw in shared:
            assert fn(**kw) == _lib.E_INVALID, (fn.__name__, what, lib.qbp_last_error())
    assert math.comb(n, 5) > _lib.MC_OSD_MAX_TRIALS + 1
    assert run(end=_lib.MC_OSD_MAX_TRIALS + 1, weight=5, flags=_lib.FLAG_OSD0) == _lib.E_INVALID      # (as qbp_mc_run_weight)
    assert b"at most" in lib.qbp_last_error()
    assert run(flags=_lib.FLAG_OSD_CS | (3 << 16)) == _lib.E_INVALID
    for what, kw in (("what = 0", dict(what=0)), ("what = 4", dict(what=4)), ("cap < 0", dict(cap=-1)),
                     ("null found", dict(found_ptr=None)), ("null ranks with cap > 0", dict(ranks_ptr=None))):
        assert fail(**kw) == _lib.E_INVALID, (what, lib.qbp_last_error())
    assert fail(flags=_lib.FLAG_RELAY) == _lib.E_UNSUPPORTED                 # (a second stage qbp_decode_shots does not take)
    assert sample(weight=-1) == -1 and sample(weight=n + 1) == -1 and sample(begin=-1) == -1
    assert sample(begin=C - 3) == -1 and sample(T=-1) == -1 and sample(weight=40, h=big) == -1
    for a, v in ((counters, 5), (ranks, 5), (kinds, 5), (found, 5), (errors, 9)):
        assert np.all(a == v)
    with pytest.raises(_lib.QbpError):
        dec.mc_run_enum(L, d, 3, prior, 0, C + 1)
    with pytest.raises(_lib.QbpError):
        dec.enum_failures(L, 3, prior, 0, 10, what=0)
    # (good calls: counters ADDED to, an empty range finds nothing)
    assert run() == 0 and counters[0] == 105
    assert fail(begin=7, end=7) == 0 and found[0] == 0 and counters[0] == 105
