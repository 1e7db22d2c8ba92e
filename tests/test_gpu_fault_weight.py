"""GPU: fixed-weight circuit-fault sampling (qbp_mc_run_fault_weight) -- the device sampler against its numpy
statement (tests/fault_weight_oracle.py) bit for bit, linearity against the device frame simulator, the counters
against the stored-errors pipeline (qbp_mc_run_errors) fed the statement's rows, the capture of failing trials against
the CPU oracle, table replacement, the refusals, and the stratified circuit-level LER against a Bernoulli run."""
import functools
import math

import numpy as np
import pytest

import enum_oracle
import fault_weight_cases as fc
import fault_weight_oracle as fo
from qldpc_amd import _lib, bp, circuit, mc, shots

pytestmark = pytest.mark.gpu

OSD_CS7 = _lib.osd_flags("cs", 7)
SEEDS = (3, 0xC0FFEE123456789)            # (the second is above 2^32: both key words in use)
BEGINS = (0, 2 ** 32 - 100)               # (the second: the counter's low word wraps inside a batch of 257)
PRIOR_P = 0.01
CAPTURE_ITERS = 4                         # (few enough that BP leaves weight-2 trials of Steane x 2 unconverged)


@functools.lru_cache(maxsize=None)
def case(name):
    """(circuit, CircuitDem by the device frame simulator, (first_fault, K, N), prior at PRIOR_P on every class)."""
    cir = fc.circuit_of(name)
    cdem = circuit.circuit_dem(cir, device=bp.DEVICE)
    # the device's model is the numpy one (tests/test_gpu_circuit.py holds that in general): the rows below depend on it
    _, _, H, L, col = fc.oracle_dem(name)
    assert np.array_equal(cdem.fault_column, col) and np.array_equal(cdem.H.toarray(), H) and np.array_equal(cdem.L, L)
    prior = mc.dem_prior(cdem.probs(circuit.rates_array(PRIOR_P, max(cir.n_classes, 1))))
    return cir, cdem, circuit.fault_sites(cir), prior


def fresh(name, classes=None):
    cir, cdem, _, _ = case(name)
    dec = _lib.Decoder(*bp.csr_from_H(cdem.H), bp.DEVICE)
    first, K, _ = circuit.fault_sites(cir, classes)
    dec.fault_table_set(first, K, cdem.fault_column)
    return dec


def statement(name, w, seed, begin, T, classes=None):
    cir, cdem, _, _ = case(name)
    first, K, _ = circuit.fault_sites(cir, classes)
    return fo.errors_fault_weight(first, K, cdem.fault_column, cdem.H.shape[1], w, seed, begin, T)


def weights_of(N):
    return sorted({0, 1, 2, 5, 64, min(N, 256)} & set(range(N + 1)))


# ---- 1. the sampler, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CASES)
def test_rows_equal_statement(name):
    _, cdem, (_, _, N), _ = case(name)
    dec = fresh(name)
    assert name != "hand" or (N == 9 and N in weights_of(N))          # (at w = N every site fires)
    for w in weights_of(N):
        T = 257 if w <= 64 else 65
        for seed in SEEDS:
            for begin in BEGINS:
                got = dec.mc_sample_errors_fault_weight(w, begin, T, seed=seed)
                assert got.shape == (T, cdem.H.shape[1]) and np.all(got.sum(axis=1) <= w)
                assert np.array_equal(got, statement(name, w, seed, begin, T)), (name, w, seed, begin)


def test_rows_of_a_reused_buffer_carry_no_stale_toggles():
    dec = fresh("72x2")
    T = 257
    first = dec.mc_sample_errors_fault_weight(256, 0, T, seed=1)
    want = statement("72x2", 256, 1, 0, T)
    assert np.array_equal(first, want) and want.sum(axis=1).min() > 2      # (every row leaves more ones than w = 2 may)
    second = dec.mc_sample_errors_fault_weight(2, 0, T, seed=1)          # (same handle, same buffers, same size)
    assert np.array_equal(second, statement("72x2", 2, 1, 0, T))
    assert np.array_equal(dec.mc_sample_errors_fault_weight(256, 0, T, seed=1), first)


def test_rows_beyond_one_launch_of_the_pick_workspace():
    """w = 256 on Steane x 2: the workspace holds the picks of 2^26 / 256 = 262 144 trials, so a longer range takes a
    second launch on it.  The rows around the seam equal the statement and the rows of a call that starts there."""
    dec = fresh("steane2")
    seam = (1 << 26) // 256
    T = seam + 70
    rows = dec.mc_sample_errors_fault_weight(256, 5, T, seed=SEEDS[1])
    assert np.array_equal(rows[seam - 40:seam + 40], statement("steane2", 256, SEEDS[1], 5 + seam - 40, 80))
    assert np.array_equal(rows[seam - 40:], dec.mc_sample_errors_fault_weight(256, 5 + seam - 40, 110, seed=SEEDS[1]))
    assert np.array_equal(rows[:40], statement("steane2", 256, SEEDS[1], 5, 40))


# ---- 2. linearity on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CASES)
def test_rows_are_the_xor_of_the_frame_simulators_fault_rows(name):
    cir, cdem, (_, _, N), _ = case(name)
    det, masks = cir.simulator(bp.DEVICE).faults(0, cir.n_faults)
    dec = fresh(name)
    H, L = cdem.H.toarray().astype(np.int64), cdem.L.astype(np.int64)
    for w in sorted({1, 2, 5, min(N, 64)} & set(range(N + 1))):
        T = 200
        faults = circuit.fault_sets(cir, w, 17, np.arange(T))
        e = dec.mc_sample_errors_fault_weight(w, 0, T, seed=17).astype(np.int64)
        assert np.array_equal(np.bitwise_xor.reduce(det[faults], axis=1), shots.pack_bits((e @ H.T) & 1)), (name, w)
        assert np.array_equal(np.bitwise_xor.reduce(masks[faults], axis=1), shots.masks_of((e @ L.T) & 1)), (name, w)


# ---- 3. the counters: those of the stored-errors pipeline on the statement's rows ---------------------------------------
def expect(dec, L, name, w, seed, begin, T, prior, **kw):
    return dec.mc_run_errors(L, 0, statement(name, w, seed, begin, T), prior, **kw)


@pytest.mark.parametrize("mode", ["default", "generic", "osd0", "cs7", "min_sum"])
def test_counters_equal_stored_errors_pipeline_steane2(mode):
    _, cdem, _, prior = case("steane2")
    T = 2000
    dec = fresh("steane2")
    kw = dict(max_iter=20)
    if mode == "generic":
        dec.set_option(_lib.OPT_FORCE_GENERIC, 1)
    elif mode == "osd0":
        kw["flags"] = _lib.FLAG_OSD0
    elif mode == "cs7":
        kw["flags"] = OSD_CS7
    elif mode == "min_sum":
        kw.update(variant=_lib.MIN_SUM, alpha=0.8)
    for w in (1, 3, 8):
        got = dec.mc_run_fault_weight(cdem.L, 0, w, prior, 0, T, seed=9, **kw)
        if mode == "generic":
            assert dec.info("last_kernel") == 2
        want = expect(dec, cdem.L, "steane2", w, 9, 0, T, prior, **kw)
        assert got[0] == T
        assert np.array_equal(got, want), (mode, w, got, want)
    assert got[1] > 0 or got[6] > 0                  # (eight faults on Steane: not a run the decoder gets right throughout)


@pytest.mark.parametrize("name,variant", [("hand", _lib.SUM_PRODUCT), ("hand", _lib.MIN_SUM), ("72x2", _lib.SUM_PRODUCT),
                                          ("72x2", _lib.MIN_SUM)])
def test_counters_equal_stored_errors_pipeline_other_circuits(name, variant):
    _, cdem, (_, _, N), prior = case(name)
    T = 1000
    for generic in (0, 1):
        dec = fresh(name)
        dec.set_option(_lib.OPT_FORCE_GENERIC, generic)
        for w in (2, min(N, 12)):
            kw = dict(max_iter=20, variant=variant, alpha=0.8 if variant == _lib.MIN_SUM else 1.0)
            got = dec.mc_run_fault_weight(cdem.L, 0, w, prior, 0, T, seed=4, **kw)
            assert np.array_equal(got, expect(dec, cdem.L, name, w, 4, 0, T, prior, **kw)), (name, generic, w)


@pytest.mark.parametrize("flags", [0, _lib.FLAG_OSD0], ids=["bp", "osd0"])
def test_chunk_split_and_stream_invariance(flags):
    import torch
    _, cdem, _, prior = case("steane2")
    kw = dict(seed=21, max_iter=20, flags=flags)
    whole = fresh("steane2").mc_run_fault_weight(cdem.L, 0, 6, prior, 0, 1000, **kw)
    dec = fresh("steane2")
    for chunk in (100, 333, 1):                                   # (ten chunks; a last chunk of one trial; chunks of one)
        dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, chunk)
        end = 1000 if chunk > 1 else 60
        got = dec.mc_run_fault_weight(cdem.L, 0, 6, prior, 0, end, **kw)
        want = whole if chunk > 1 else expect(dec, cdem.L, "steane2", 6, 21, 0, end, prior, max_iter=20, flags=flags)
        assert np.array_equal(got, want), chunk
    dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 333)
    parts = (dec.mc_run_fault_weight(cdem.L, 0, 6, prior, 0, 337, **kw)
             + dec.mc_run_fault_weight(cdem.L, 0, 6, prior, 337, 1000, **kw))
    assert np.array_equal(parts, whole)
    assert np.array_equal(whole, expect(dec, cdem.L, "steane2", 6, 21, 0, 1000, prior, max_iter=20, flags=flags))
    # the _device form on a stream of its own: ADDED to, the same digits
    dev = torch.device("cuda", bp.DEVICE)
    start = np.arange(100, 112, dtype=np.int64)
    d_cnt = torch.from_numpy(start.copy()).to(dev)
    d_prior = torch.from_numpy(prior).to(dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    for a, b in ((0, 400), (400, 1000)):
        dec.mc_run_fault_weight_device(cdem.L, 0, 6, d_prior.data_ptr(), a, b, d_cnt.data_ptr(), stream=stream.cuda_stream,
                                       **kw)
    stream.synchronize()
    assert np.array_equal(d_cnt.cpu().numpy(), start + whole)
    begin = 2 ** 32 - 100                                           # (trial indices across 2^32, a seed above it)
    got = dec.mc_run_fault_weight(cdem.L, 0, 6, prior, begin, begin + 257, seed=SEEDS[1], max_iter=20, flags=flags)
    assert np.array_equal(got, expect(dec, cdem.L, "steane2", 6, SEEDS[1], begin, 257, prior, max_iter=20, flags=flags))


def test_driver_table_equals_the_host_entry():
    code = fc.circuit_cases.code("steane")
    _, cdem, (_, _, N), prior = case("steane2")
    dec = fresh("steane2")
    table, n_sites = mc.run_circuit_weights(code, 2, [0, 3, 7], 1000, prior_p=PRIOR_P, seed=2, max_iter=20, osd=True,
                                            device=bp.DEVICE)
    assert n_sites == N and table.shape == (3, 12)
    assert table[0, 0] == 1000 and table[0, 1] == 0 and table[0, 9] == 1000
    for row, w in zip(table[1:], (3, 7)):
        assert np.array_equal(row, dec.mc_run_fault_weight(cdem.L, 0, w, prior, 0, 1000, seed=2, max_iter=20,
                                                           flags=_lib.FLAG_OSD0))
    halves = [mc.run_circuit_weights(code, 2, [3, 7], 1000, prior_p=PRIOR_P, seed=2, max_iter=20, osd=True, rank=r, world=2,
                                     device=bp.DEVICE, reduce=False)[0] for r in (0, 1)]
    assert np.array_equal(halves[0] + halves[1], table[1:])


# ---- 4. the capture of failing trials -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capture_statement(osd):
    """kinds uint8 [4096] of trials 0 .. 4095 of weight 2 on Steane x 2 by the CPU oracle's BP (+ OSD-0)."""
    _, cdem, _, prior = case("steane2")
    rows = statement("steane2", 2, 7, 0, 4096)
    kinds = enum_oracle.kinds_of(cdem.H.toarray(), cdem.L, rows, prior, CAPTURE_ITERS, osd=osd)[0]
    kinds.setflags(write=False)
    return kinds


@pytest.mark.parametrize("osd", [False, True], ids=["bp", "osd0"])
def test_capture_equals_the_oracle(osd):
    cir, cdem, _, prior = case("steane2")
    kinds = capture_statement(osd)
    print("trials by kind", np.bincount(kinds, minlength=4).tolist())
    flags = _lib.FLAG_OSD0 if osd else 0
    dec = fresh("steane2")
    for what in (1, 2, 3):
        want = np.flatnonzero(kinds & what)
        trials, got_kinds, found, cnt = dec.fault_weight_failures(cdem.L, 2, prior, 0, 4096, seed=7, what=what, cap=4096,
                                                                  max_iter=CAPTURE_ITERS, flags=flags)
        assert found == len(want) == len(trials)
        assert np.array_equal(trials, want) and trials.dtype == np.int64          # (ascending: found <= cap)
        assert np.array_equal(got_kinds, kinds[want])
        assert cnt[0] == 4096 and found == (cnt[1], cnt[6], found)[what - 1]
    # a range that does not start at 0, in chunks: the captured int64 is the global trial index
    dec.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 97)
    trials, got_kinds, found, _ = dec.fault_weight_failures(cdem.L, 2, prior, 1000, 3000, seed=7, what=3, cap=4096,
                                                            max_iter=CAPTURE_ITERS, flags=flags)
    sel = np.flatnonzero(kinds & 3)
    sel = sel[(sel >= 1000) & (sel < 3000)]
    assert found == len(sel) and np.array_equal(trials, sel) and np.array_equal(got_kinds, kinds[sel])
    # and the driver names the faults of every captured trial
    out = mc.circuit_failing_faults(fc.circuit_cases.code("steane"), 2, 2, 4096, prior_p=PRIOR_P, what="either", seed=7,
                                    max_iter=CAPTURE_ITERS, osd=osd, device=bp.DEVICE)
    want = np.flatnonzero(kinds & 3)
    assert out["found"] == len(want) and np.array_equal(out["trials"], want) and np.array_equal(out["kinds"], kinds[want])
    assert np.array_equal(out["faults"], circuit.fault_sets(cir, 2, 7, want)) and out["faults"].shape == (len(want), 2)
    base, K = cir.sites()[5], cir.sites()[4]
    assert np.array_equal(base[out["sites"]] + out["codes"] - 1, out["faults"])
    assert np.all((out["codes"] >= 1) & (out["codes"] <= K[out["sites"]]))


def test_capture_cap_sentinels_and_device_form():
    import torch
    _, cdem, _, prior = case("steane2")
    kinds = capture_statement(True)
    want = np.flatnonzero(kinds & 3)
    assert len(want) > 20                                            # (so that a cap of 10 is below found)
    lib = _lib.load()
    dec = fresh("steane2")
    Lc = np.ascontiguousarray(cdem.L, np.uint8)

    def raw(begin, end, what, cap, trials, knd, found, counters):
        return lib.qbp_fault_weight_failures(dec._h, Lc.ctypes.data, Lc.shape[0], 2, 7, begin, end, prior.ctypes.data,
                                             CAPTURE_ITERS, 0, 1.0, 1.0, 20.0, _lib.FLAG_OSD0, what, cap,
                                             None if trials is None else trials.ctypes.data,
                                             None if knd is None else knd.ctypes.data, found.ctypes.data,
                                             counters.ctypes.data)

    cap = 10
    trials, knd = np.full(cap + 50, -7, np.int64), np.full(cap + 50, 0xEE, np.uint8)
    found, counters = np.full(1, -7, np.int64), np.zeros(12, np.int64)
    assert raw(0, 4096, 3, cap, trials, knd, found, counters) == 0
    assert found[0] == len(want) > cap
    assert len(set(trials[:cap].tolist())) == cap and np.all(np.isin(trials[:cap], want))
    assert np.array_equal(knd[:cap], kinds[trials[:cap]])
    assert np.all(trials[cap:] == -7) and np.all(knd[cap:] == 0xEE)
    found[0] = -7                                                     # cap = 0 with null arrays: a count
    assert raw(0, 4096, 3, 0, None, None, found, counters) == 0 and found[0] == len(want)
    assert counters[0] == 2 * 4096                                    # (ADDED to)
    few = np.flatnonzero(kinds[:100] & 3)                             # cap > found: nothing beyond found is written
    assert 0 < len(few) < len(trials)                                 # (37 of the first 100 trials by the oracle; 60 entries)
    trials[:], knd[:] = -7, 0xEE
    assert raw(0, 100, 3, len(trials), trials, knd, found, counters) == 0
    assert found[0] == len(few)
    assert np.array_equal(trials[:len(few)], few) and np.all(trials[len(few):] == -7) and np.all(knd[len(few):] == 0xEE)
    assert raw(9, 9, 3, 4, trials, knd, found, counters) == 0 and found[0] == 0            # (an empty range)
    # the _device form: d_found ADDED to, entries in no particular order
    dev = torch.device("cuda", bp.DEVICE)
    d_prior = torch.from_numpy(prior).to(dev)
    d_trials = torch.full((len(want) + 10,), -7, dtype=torch.int64, device=dev)
    d_kinds = torch.full((len(want) + 10,), 0xEE, dtype=torch.uint8, device=dev)
    d_found = torch.zeros(1, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    for a, b in ((0, 1500), (1500, 4096)):
        dec.fault_weight_failures_device(cdem.L, 2, d_prior.data_ptr(), a, b, 3, len(d_trials), d_trials.data_ptr(),
                                         d_kinds.data_ptr(), d_found.data_ptr(), d_cnt.data_ptr(), seed=7,
                                         max_iter=CAPTURE_ITERS, flags=_lib.FLAG_OSD0, stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_found.item()) == len(want)
    t, k = d_trials.cpu().numpy(), d_kinds.cpu().numpy()
    order = np.argsort(t[:len(want)])
    assert np.array_equal(t[:len(want)][order], want) and np.array_equal(k[:len(want)][order], kinds[want])
    assert np.all(t[len(want):] == -7) and np.all(k[len(want):] == 0xEE)
    assert d_cnt.cpu().numpy()[0] == 4096


# ---- 5. table replacement -------------------------------------------------------------------------------------------------------
def test_a_second_table_replaces_the_first_and_a_cleared_one_is_refused():
    cir, cdem, (first, K, N), prior = case("hand")
    dec = fresh("hand")
    T = 100
    assert np.array_equal(dec.mc_sample_errors_fault_weight(3, 0, T, seed=5), statement("hand", 3, 5, 0, T))
    f1, k1, n1 = circuit.fault_sites(cir, [1])                       # class 0 masked off
    assert 0 < n1 < N
    dec.fault_table_set(f1, k1, cdem.fault_column)
    masked = dec.mc_sample_errors_fault_weight(3, 0, T, seed=5)
    assert np.array_equal(masked, statement("hand", 3, 5, 0, T, classes=[1]))
    assert not np.array_equal(masked, statement("hand", 3, 5, 0, T))
    with pytest.raises(_lib.QbpError):                               # (N changed: w = N of the first table is too many now)
        dec.mc_sample_errors_fault_weight(N, 0, T)
    assert np.array_equal(dec.mc_sample_errors_fault_weight(n1, 0, T), statement("hand", n1, 0, 0, T, classes=[1]))
    dec.fault_table_set(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32))
    with pytest.raises(_lib.QbpError, match="fault table"):
        dec.mc_sample_errors_fault_weight(0, 0, T)
    with pytest.raises(_lib.QbpError, match="fault table"):
        dec.mc_run_fault_weight(cdem.L, 0, 1, prior, 0, 10)
    dec.fault_table_set(first, K, cdem.fault_column)                 # (and back)
    assert np.array_equal(dec.mc_sample_errors_fault_weight(3, 0, T, seed=5), statement("hand", 3, 5, 0, T))


# ---- 6. refusals: host only, outputs untouched -----------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    cir, cdem, (first, K, N), prior = case("steane2")
    n = cdem.H.shape[1]
    lib = _lib.load()
    bare = _lib.Decoder(*bp.csr_from_H(cdem.H), bp.DEVICE)           # (no table yet)
    dec = fresh("steane2")
    Lc = np.ascontiguousarray(cdem.L, np.uint8)
    counters = np.full(12, 5, np.int64)
    trials, kinds, found = np.full(8, 5, np.int64), np.full(8, 5, np.uint8), np.full(1, 5, np.int64)
    errors = np.full((4, n), 9, np.uint8)

    def run(weight=3, begin=0, end=100, prior_ptr=prior.ctypes.data, flags=0, counters_ptr=counters.ctypes.data, h=dec):
        return lib.qbp_mc_run_fault_weight(h._h, Lc.ctypes.data, Lc.shape[0], 0, weight, 0, begin, end, prior_ptr, 20, 0,
                                           1.0, 1.0, 20.0, flags, counters_ptr)

    def fail(weight=3, begin=0, end=100, flags=0, what=1, cap=8, found_ptr=found.ctypes.data,
             trials_ptr=trials.ctypes.data, h=dec):
        return lib.qbp_fault_weight_failures(h._h, Lc.ctypes.data, Lc.shape[0], weight, 0, begin, end, prior.ctypes.data, 20,
                                             0, 1.0, 1.0, 20.0, flags, what, cap, trials_ptr, kinds.ctypes.data, found_ptr,
                                             counters.ctypes.data)

    def sample(weight=3, begin=0, T=4, h=dec, ptr=errors.ctypes.data):
        return lib.qbp_mc_sample_errors_fault_weight(h._h, weight, 0, begin, T, ptr)

    assert N > _lib.FAULT_WEIGHT_MAX                                   # (302 sites: the cap binds on this circuit)
    shared = (("w = -1", dict(weight=-1), b"weight"), ("w = 257", dict(weight=_lib.FAULT_WEIGHT_MAX + 1), b"weight"),
              ("no table", dict(h=bare), b"fault table"), ("trial_begin < 0", dict(begin=-5), b"trial_begin"),
              ("end < begin", dict(begin=10, end=5), b">= "))
    for fn in (run, fail):
        for what, kw, word in shared:
            assert fn(**kw) == _lib.E_INVALID, (fn.__name__, what, lib.qbp_last_error())
            assert word in lib.qbp_last_error(), (fn.__name__, what, lib.qbp_last_error())
    hand = fresh("hand")                                               # (nine sites: N binds)
    assert lib.qbp_mc_sample_errors_fault_weight(hand._h, 10, 0, 0, 4, errors.ctypes.data) == _lib.E_INVALID
    for what, kw, word in (("null prior", dict(prior_ptr=None), b"null"),
                           ("a method bit without OSD0", dict(flags=_lib.FLAG_OSD_CS | (3 << 16)), b"QBP_FLAG_OSD0"),
                           ("too many trials with OSD", dict(end=_lib.MC_OSD_MAX_TRIALS + 1, flags=_lib.FLAG_OSD0),
                            b"at most"), ("null counters", dict(counters_ptr=None), b"null")):
        assert run(**kw) == _lib.E_INVALID, what
        assert word in lib.qbp_last_error(), (what, lib.qbp_last_error())
    for what, kw in (("what = 0", dict(what=0)), ("what = 4", dict(what=4)), ("cap < 0", dict(cap=-1)),
                     ("null found", dict(found_ptr=None)), ("null trials with cap > 0", dict(trials_ptr=None))):
        assert fail(**kw) == _lib.E_INVALID, (what, lib.qbp_last_error())
    assert fail(flags=_lib.FLAG_RELAY) == _lib.E_UNSUPPORTED          # (a second stage qbp_decode_shots does not take)
    assert sample(weight=-1) == -1 and sample(weight=257) == -1 and sample(begin=-1) == -1 and sample(T=-1) == -1
    assert sample(h=bare) == -1 and sample(ptr=None) == -1
    # the table itself: refused, and the handle's table stays as it was
    before = dec.mc_sample_errors_fault_weight(5, 0, 50, seed=8)
    f64, k8 = np.ascontiguousarray(first, np.int64), np.ascontiguousarray(K, np.uint8)
    col = np.ascontiguousarray(cdem.fault_column, np.int32)

    def table(n_sites=N, f=f64, k=k8, n_faults=len(col), c=col):
        return lib.qbp_fault_table_set(dec._h, n_sites, None if f is None else f.ctypes.data,
                                       None if k is None else k.ctypes.data, n_faults, None if c is None else c.ctypes.data)

    bad_k, past_end, neg_first, col_n, col_low = k8.copy(), f64.copy(), f64.copy(), col.copy(), col.copy()
    bad_k[3] = 2
    past_end[-1] = len(col) - int(k8[-1]) + 1
    neg_first[0] = -1
    col_n[7] = n
    col_low[7] = -2
    for what, kw in (("null first_fault", dict(f=None)), ("null K", dict(k=None)), ("null fault_column", dict(c=None)),
                     ("K = 2", dict(k=bad_k)), ("first_fault + K > n_faults", dict(f=past_end)),
                     ("first_fault < 0", dict(f=neg_first)), ("column = n", dict(c=col_n)), ("column = -2", dict(c=col_low)),
                     ("n_sites < 0", dict(n_sites=-1)), ("n_sites > 2^32 - 4", dict(n_sites=2 ** 32 - 3)),
                     ("fewer faults than the sites name", dict(n_faults=len(col) - 1))):
        assert table(**kw) == _lib.E_INVALID, (what, lib.qbp_last_error())
    assert np.array_equal(dec.mc_sample_errors_fault_weight(5, 0, 50, seed=8), before)
    with pytest.raises(ValueError):
        dec.fault_table_set(first, K, np.full(len(col), n))
    with pytest.raises(ValueError):
        dec.fault_table_set(first, K[:-1], col)
    for a, v in ((counters, 5), (trials, 5), (kinds, 5), (found, 5), (errors, 9)):
        assert np.all(a == v)
    with pytest.raises(_lib.QbpError):
        dec.mc_run_fault_weight(cdem.L, 0, 257, prior, 0, 10)
    with pytest.raises(_lib.QbpError):
        dec.fault_weight_failures(cdem.L, 2, prior, 0, 10, what=0)
    # (good calls: counters ADDED to, no trials change nothing)
    assert run(end=0) == 0 and np.all(counters == 5)
    assert run() == 0 and counters[0] == 105


# ---- 7. end to end: the stratified estimator against a Bernoulli run --------------------------------------------------------
def test_stratified_circuit_ler_equals_bernoulli_ler_on_steane():
    """Steane x 1 round, every class at p = 0.01, BP(20) + OSD-0.  Weights 0 .. W at 2e5 trials each and
    ler_from_weights at p against run_circuit at p with 2e5 shots: within 5 combined standard errors (the estimate's
    stderr and the binomial error of the Bernoulli run).  W = 12: the binomial mass above it is below 1e-6 for N <= 200
    (checked below), three orders under either standard error."""
    code = fc.circuit_cases.code("steane")
    p, T, W = 0.01, 200_000, 12
    N = circuit.fault_sites(fc.circuit_of("steane1"))[2]
    assert 100 <= N <= 200
    mass_above = float(mc.binomial_weights(N, p)[W + 1:].sum())
    assert mass_above < 1e-6
    weights = list(range(W + 1))
    table, n_sites = mc.run_circuit_weights(code, 1, weights, T, prior_p=p, seed=31, max_iter=20, osd=True, device=bp.DEVICE)
    assert n_sites == N and np.all(table[:, 0] == T) and table[0, 1] == 0
    est = mc.ler_from_weights(table, weights, N, [p])
    assert est["unsampled_mass"][0] == pytest.approx(mass_above, rel=1e-6)
    bern = mc.run_circuit(code, 1, [p], T, seed=32, max_iter=20, osd=True, device=bp.DEVICE)[0]
    ler_b = bern[1] / bern[0]
    sigma = math.sqrt(est["stderr"][0] ** 2 + ler_b * (1 - ler_b) / T)
    print("f_w", (table[:, 1] / T).tolist())
    print("stratified LER", est["ler"][0], "+-", est["stderr"][0], "Bernoulli", ler_b, "5 sigma", 5 * sigma)
    assert bern[0] == T and 0 < ler_b < 0.5
    assert abs(est["ler"][0] - ler_b) <= 5 * sigma
