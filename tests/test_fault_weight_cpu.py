"""CPU: the fixed-weight FAULT sampler (include/qbp.h, qbp_mc_run_fault_weight) -- its numpy statement
(tests/fault_weight_oracle.py), ``circuit.fault_sites`` / ``circuit.fault_sets``, the estimator on synthetic failure
fractions, the Python-side refusals, and linearity against the numpy frame simulator (tests/circuit_oracle.py)."""
import math

import numpy as np
import pytest
from scipy import stats

import circuit_oracle as co
import fault_weight_cases as fc
import fault_weight_oracle as fo
from qldpc_amd import circuit, mc

SEEDS = (3, 0xC0FFEE123456789)            # (the second is above 2^32: both key words in use)
BEGINS = (0, 2 ** 32 - 20)                # (the second: the counter's low word wraps inside the batch)


def table(case, classes=None):
    first, K, N = circuit.fault_sites(fc.circuit_of(case), classes)
    return first, K, N


def weights_of(N):
    return sorted({0, 1, 2, 5, 64, min(N, 256)} & set(range(N + 1)))


@pytest.mark.parametrize("case", fc.CASES)
def test_picks_are_distinct_sites_in_range(case):
    first, K, N = table(case)
    for w in weights_of(N):
        sites, faults = fo.picks(first, K, w, SEEDS[1], BEGINS[1], 40)
        assert sites.shape == faults.shape == (40, w)
        assert np.all((sites >= 0) & (sites < N))
        assert all(len(set(r)) == w for r in sites.tolist()), w
        code = faults - first[sites]
        assert np.all((code >= 0) & (code < K[sites]))
    # every site fires at w = N
    sites, _ = fo.picks(first, K, min(N, 256), 1, 0, 3)
    if N <= 256:
        assert np.array_equal(np.sort(sites, axis=1), np.tile(np.arange(N), (3, 1)))


@pytest.mark.parametrize("case", fc.CASES)
def test_row_popcount_and_parity(case):
    first, K, N = table(case)
    _, _, H, _, col = fc.oracle_dem(case)
    n = H.shape[1]
    saw_dropped = False
    for w in weights_of(N):
        _, faults = fo.picks(first, K, w, SEEDS[0], 0, 60)
        rows = fo.rows_of_faults(faults, col, n)
        live = (col[faults] >= 0).sum(axis=1)
        saw_dropped |= bool(np.any(live < w))
        assert np.all(rows.sum(axis=1) <= w)
        assert np.array_equal(rows.sum(axis=1) & 1, live & 1), w
        assert np.array_equal(rows, fo.errors_fault_weight(first, K, col, n, w, SEEDS[0], 0, 60))
    if case == "hand":
        assert saw_dropped                       # (the -1 case is exercised)


@pytest.mark.parametrize("case", fc.CASES)
def test_fault_sets_agrees_with_the_statement(case):
    cir = fc.circuit_of(case)
    first, K, N = table(case)
    _, _, H, _, col = fc.oracle_dem(case)
    for w in weights_of(N):
        for seed in SEEDS:
            for begin in BEGINS:
                T = 33 if w <= 64 else 5
                got = circuit.fault_sets(cir, w, seed, np.arange(begin, begin + T))
                assert got.dtype == np.int64 and got.shape == (T, w)
                assert np.array_equal(got, fo.picks(first, K, w, seed, begin, T)[1]), (w, seed, begin)
                assert np.array_equal(fo.rows_of_faults(got, col, H.shape[1]),
                                      fo.errors_fault_weight(first, K, col, H.shape[1], w, seed, begin, T))
    # trials in any order, one at a time
    whole = circuit.fault_sets(cir, min(N, 5), 9, np.arange(100, 130))
    pick = np.array([129, 100, 117])
    assert np.array_equal(circuit.fault_sets(cir, min(N, 5), 9, pick), whole[pick - 100])


def test_site_and_code_frequencies_are_uniform():
    """The hand circuit, N = 9, w = 3, T = 30 000 trials at seed 11.  A site is in a trial's set with probability w / N;
    with c_s the number of trials that hold site s, X = (N - 1) / N * sum_s (c_s - T w / N)^2 / (T (w / N)(1 - w / N)) is
    asymptotically chi-square with N - 1 degrees of freedom for uniform sets (the (N - 1) / N accounts for the fixed set
    size).  The codes of the DEP2 site over the trials that pick it: Pearson's statistic with 14 degrees of freedom.
    Bounds: the 1 - 1e-6 quantiles.  The multiply-shift bias is at most N / 2^32 per step, far below the resolution of
    30 000 trials."""
    first, K, N = table("hand")
    w, T = 3, 30000
    sites, faults = fo.picks(first, K, w, 11, 0, T)
    counts = np.bincount(sites.ravel(), minlength=N)
    q = w / N
    X = (N - 1) / N * float(np.sum((counts - T * q) ** 2)) / (T * q * (1 - q))
    bound = stats.chi2.isf(1e-6, N - 1)
    print("sites: chi-square", X, "bound", bound, "counts", counts.tolist())
    assert counts.sum() == T * w and X < bound
    dep2 = int(np.flatnonzero(K == 15)[0])
    codes = (faults - first[sites])[sites == dep2]
    cc = np.bincount(codes, minlength=15)
    Xc = float(np.sum((cc - cc.sum() / 15) ** 2 / (cc.sum() / 15)))
    print("codes: chi-square", Xc, "bound", stats.chi2.isf(1e-6, 14), "counts", cc.tolist())
    assert len(cc) == 15 and Xc < stats.chi2.isf(1e-6, 14)
    # and the order within a set carries no site preference either: step 0 alone is a uniform draw from N - w + 1 sites
    assert set(sites[:, 0].tolist()) == set(range(N - w + 1))


def test_fault_sites_with_a_class_left_out():
    cir = fc.hand_circuit()
    first, K, N = circuit.fault_sites(cir)
    assert N == cir.n_sites == 9 and np.array_equal(first, cir.sites()[5][:-1]) and np.array_equal(K, cir.sites()[4])
    assert first.dtype == np.int64 and K.dtype == np.int64
    for classes in ([0], [1], [0, 1]):
        f, k, n = circuit.fault_sites(cir, classes)
        wf, wk, wn = fc.masked_table(cir, set(classes))
        assert n == wn and np.array_equal(f, wf) and np.array_equal(k, wk)
    assert circuit.fault_sites(cir, [0])[2] + circuit.fault_sites(cir, [1])[2] == 9
    assert circuit.fault_sites(cir, [])[2] == 0 and circuit.fault_sites(cir, [7])[2] == 0
    # names of the memory experiment's classes; the sets differ, and so do the trials
    mem = fc.circuit_of("steane2")
    all_n = circuit.fault_sites(mem)[2]
    parts = [circuit.fault_sites(mem, [c])[2] for c in ("reset", "cnot", "idle", "meas")]
    assert sum(parts) == all_n and all(p > 0 for p in parts)
    f, k, n = circuit.fault_sites(mem, ["cnot", 3])
    assert n == parts[1] + parts[3] and set(k.tolist()) == {1, 15}
    a = circuit.fault_sets(mem, 4, 5, np.arange(20))
    b = circuit.fault_sets(mem, 4, 5, np.arange(20), classes=["cnot", "meas"])
    assert not np.array_equal(a, b)
    assert np.array_equal(b, fo.picks(f, k, 4, 5, 0, 20)[1])
    with pytest.raises(ValueError):
        circuit.fault_sites(mem, [16])
    with pytest.raises(KeyError):
        circuit.fault_sites(mem, ["gate"])


def test_ler_from_weights_is_the_binomial_sum_over_sites():
    N = 158
    weights = list(range(0, 13))
    f = np.array([0, 0, 1e-3, 4e-3, 0.01, 0.03, 0.06, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5])
    T = 1_000_000
    tab = np.zeros((len(weights), mc.NUM_COUNTERS), np.int64)
    tab[:, 0] = T
    tab[:, 1] = np.round(f * T).astype(np.int64)
    ps = [1e-4, 1e-3, 0.01]
    est = mc.ler_from_weights(tab, weights, N, ps)
    for i, p in enumerate(ps):
        B = [math.comb(N, w) * p ** w * (1 - p) ** (N - w) for w in range(N + 1)]
        want = sum(B[w] * (tab[j, 1] / T) for j, w in enumerate(weights))
        assert est["ler"][i] == pytest.approx(want, rel=1e-9)
        assert est["unsampled_mass"][i] == pytest.approx(sum(B[13:]), rel=1e-6, abs=1e-300)
        assert est["stderr"][i] == pytest.approx(math.sqrt(sum(B[w] ** 2 * f[j] * (1 - f[j]) / T
                                                               for j, w in enumerate(weights))), rel=1e-6)
    # W = 12 carries the mass at p = 0.01 for N <= 200 (the condition of the end-to-end GPU test)
    assert mc.binomial_weights(200, 0.01)[13:].sum() < 1e-6


def test_python_side_refusals():
    cir = fc.hand_circuit()
    for bad in (-1, 10):
        with pytest.raises(ValueError, match="weight"):
            circuit.fault_sets(cir, bad, 0, [0])
    with pytest.raises(ValueError, match="weight"):
        circuit.fault_sets(fc.circuit_of("72x2"), 257, 0, [0])          # (N = 3888: FAULT_WEIGHT_MAX binds)
    with pytest.raises(ValueError, match="weight"):
        circuit.fault_sets(cir, 5, 0, [0], classes=[1])                 # (four sites are left)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            circuit.fault_sets(cir, 1, seed, [0])
    code = fc.circuit_cases.code("steane")
    kw = dict(prior_p=0.01)
    for args, extra, word in (((code, 1, [1], 10), dict(prior_p=0.0), "prior_p"),
                              ((code, 1, [1], 10), dict(prior_p=1.0), "prior_p"),
                              ((code, 1, [159], 10), kw, "weights"),
                              ((code, 1, [-1], 10), kw, "weights"),
                              ((code, 1, [1.5], 10), kw, "weights"),
                              ((code, 1, [1], 10), dict(prior_p=0.01, classes=[9]), "no fault site"),
                              ((code, 1, [1], 10), dict(prior_p=0.01, classes=[]), "no fault site"),
                              ((code, 1, [40], 10), dict(prior_p=0.01, classes=["meas"]), "weights"),
                              ((code, 0, [1], 10), kw, "rounds"),
                              ((code, 1, [1], 10), dict(prior_p=0.01, osd_order=3), "osd"),
                              ((code, 1, [1], 10), dict(prior_p=0.01, quant=dict(bits=8, scale=4.0)), "min-sum")):
        with pytest.raises(ValueError, match=word):
            mc.run_circuit_weights(*args, **extra)
    with pytest.raises(ValueError, match="weights"):
        mc.run_circuit_weights(fc.circuit_cases.code("[[72, 12, 6]]"), 2, [257], 10, prior_p=0.01)
    with pytest.raises(ValueError, match="what"):
        mc.circuit_failing_faults(code, 1, 2, 10, prior_p=0.01, what="neither")
    with pytest.raises(ValueError, match="weights"):
        mc.circuit_failing_faults(code, 1, 500, 10, prior_p=0.01)
    with pytest.raises(ValueError, match="cap"):
        mc.circuit_failing_faults(code, 1, 2, 10, prior_p=0.01, cap=-1)
    for argv in (["--fault-weights", "2", "--prior-p", "0.01"],                           # (no --circuit)
                 ["--circuit", "72", "2", "--fault-weights", "2"],                         # (no --prior-p)
                 ["--circuit", "72", "2", "--fault-weights", "2", "--prior-p", "0.01", "--shots", "100"],
                 ["--circuit", "72", "2", "--fault-weights", "2", "--prior-p", "0.01", "--weights", "3"],
                 ["--circuit", "72", "2", "--fault-weights", "2", "--prior-p", "0.01", "--ler-at", "2"],
                 ["--circuit", "72", "2", "--fault-weights", "9999", "--prior-p", "0.01"],
                 ["--circuit", "72", "2", "--fault-weights", "2", "--prior-p", "0.01", "--classes", "gate"]):
        with pytest.raises(SystemExit):
            mc.main(argv)


@pytest.mark.parametrize("case", fc.CASES)
def test_linearity_against_the_frame_oracle(case):
    """The XOR of the oracle's single-fault rows of a trial's faults equals H e and L e of its row."""
    cir = fc.circuit_of(case)
    det, obs, H, L, col = fc.oracle_dem(case)
    N = circuit.fault_sites(cir)[2]
    Hi, Li = H.astype(np.int64), L.astype(np.int64)
    for w in sorted({1, 2, 5, min(N, 64)} & set(range(N + 1))):
        faults = circuit.fault_sets(cir, w, 17, np.arange(40))
        e = fo.rows_of_faults(faults, col, H.shape[1]).astype(np.int64)
        assert np.array_equal(np.bitwise_xor.reduce(det[faults], axis=1), (e @ Hi.T) & 1), w
        assert np.array_equal(np.bitwise_xor.reduce(obs[faults], axis=1), (e @ Li.T) & 1), w
    if case != "72x2":
        # and the fault set injected into ONE propagation gives the same row: the frame simulator is linear
        sites, base = co.sites_of(cir)
        faults = circuit.fault_sets(cir, min(N, 5), 23, np.arange(8))
        for f in faults:
            site = np.searchsorted(base, f, side="right") - 1
            by_site = {int(s): int(x - base[s] + 1) for s, x in zip(site, f)}
            empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
            rec = co.propagate(cir, 1, lambda j: (np.zeros(1, np.int64), np.array([by_site[j]])) if j in by_site else empty)
            d1, o1 = co.assemble(cir, rec)
            assert np.array_equal(d1[0], np.bitwise_xor.reduce(det[f], axis=0))
            assert np.array_equal(o1[0], np.bitwise_xor.reduce(obs[f], axis=0))
