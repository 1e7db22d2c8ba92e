"""Circuits, the memory experiment, the detector error model of a circuit and the numpy statement of the Pauli-frame
simulator (tests/circuit_oracle.py), on the host: physics against a state-vector simulator, wrong statements, the
builder's figures, text round trips, refusals and the sampler's marginals."""
import numpy as np
import pytest

import circuit_cases as cc
import circuit_oracle as co
import statevector_util as sv
from qldpc_amd import circuit, codes, mc
from qldpc_amd import dem as dem_mod

RATES = [0.01, 0.004, 0.002, 0.02]


def pauli_of(kind, code):
    return 1 if kind == "XERR" else 2 if kind == "ZERR" else code


def outcomes(cir, rec):
    det, obs = co.assemble(cir, rec[None, :])
    return det[0], obs[0]


# ---- physics ------------------------------------------------------------------------------------------------------
PHYSICS = [("422", 2, "Z", "basis"), ("422", 2, "X", "all"), ("steane", 2, "Z", "all"), ("steane", 2, "X", "basis")]


@pytest.mark.parametrize("key", PHYSICS, ids=str)
def test_without_a_fault_nothing_fires(key):
    cir = cc.memory(*key)
    assert cir.nq == (6 if key[0] == "422" else 13)
    for seed in range(5):
        det, obs = outcomes(cir, sv.run(cir, np.random.default_rng(seed)))
        assert not det.any() and not obs.any()


@pytest.mark.parametrize("key", PHYSICS, ids=str)
def test_a_fault_fires_its_column(key):
    """[[4,2,2]]: every fault; Steane: 200 faults drawn by a fixed seed."""
    cir = cc.memory(*key)
    det, obs, _, _ = cc.fault_rows(key)
    sites, base = co.sites_of(cir)
    faults = range(cir.n_faults) if key[0] == "422" else np.random.default_rng(11).choice(cir.n_faults, 200, replace=False)
    for f in faults:
        j = int(np.searchsorted(base, f, side="right")) - 1
        p = pauli_of(sites[j][0], int(f - base[j]) + 1)
        d, o = outcomes(cir, sv.run(cir, np.random.default_rng(int(f)), fault=(j, p)))
        assert np.array_equal(d, det[f]) and np.array_equal(o, obs[f]), f


# ---- wrong statements ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect, key", [("z_forward", ("422", 2, "X", "basis")), ("reset_keeps", "reset"),
                                         ("y_as_x", ("422", 2, "X", "basis")), ("swap_pair", ("422", 2, "Z", "basis")),
                                         ("mx_reads_x", ("422", 2, "X", "basis")),
                                         ("final_no_prev", ("422", 2, "Z", "basis"))])
def test_each_wrong_statement_changes_the_output(defect, key):
    cir = cc.reset_circuit() if key == "reset" else cc.memory(*key)
    det, obs, _, _ = cc.fault_rows(key)
    bad_det, bad_obs = co.faults(cir, defect=defect)
    assert not (np.array_equal(det, bad_det) and np.array_equal(obs, bad_obs))


def test_noise_before_a_reset_and_after_a_measurement_is_dropped():
    cir = cc.reset_circuit()
    det, obs, bits, masks = cc.fault_rows("reset")
    sites, base = co.sites_of(cir)
    assert [s[0] for s in sites] == ["XERR", "DEP2", "DEP1", "DEP1", "ZERR"] and cir.n_faults == 23
    d = circuit.dem_from_fault_rows(cir, bits, masks)
    dead = range(int(base[3]), int(base[4]))                   # DEP1 on qubit 0 between MZ 0 and RZ 0
    assert all(d.fault_column[f] == -1 for f in dead)
    assert d.fault_column[0] == 0 and det[0].tolist() == [1, 0, 0] and obs[0].tolist() == [0, 1]
    assert (d.fault_column >= 0).sum() == d.counts.sum() and d.H.shape[1] == d.fault_column.max() + 1
    H, L, col = co.merge(det, obs)
    assert np.array_equal(d.H.toarray(), H) and np.array_equal(d.L, L) and np.array_equal(d.fault_column, col)
    assert d.H.has_sorted_indices and d.H.dtype == np.uint8 and d.L.dtype == np.uint8


# ---- builder ------------------------------------------------------------------------------------------------------
def test_builder_figures_72():
    """[[72,12,6]] over 6 rounds: 144 qubits, 2592 CNOTs, 63216 faults, a 252 x 2232 model with column weight <= 9 and
    row weight <= 42, 7 layers for Hx (the greedy colouring of Hz takes 8), no undetectable logical column."""
    code = cc.code("72")
    cir = cc.memory("72", 6)
    assert (cir.nq, cir.count("CX"), cir.n_faults) == (144, 2592, 63216)
    assert (len(circuit.edge_layers(code.Hx)), len(circuit.edge_layers(code.Hz))) == (7, 8)
    det, obs, bits, masks = cc.fault_rows(("72", 6, "Z", "basis"))
    d = circuit.dem_from_fault_rows(cir, bits, masks)
    A = d.H.toarray()
    assert A.shape == (252, 2232) and d.L.shape == (12, 2232)
    assert A.sum(axis=0).max() == 9 and A.sum(axis=1).max() == 42
    assert A.sum(axis=0).min() >= 1
    H, L, col = co.merge(det, obs)
    assert np.array_equal(A, H) and np.array_equal(d.L, L) and np.array_equal(d.fault_column, col)


def test_builder_counts_144():
    """[[144,12,12]] over 12 rounds, the counts that need no propagation."""
    code = cc.code("144")
    cir = cc.memory("144", 12)
    assert (cir.nq, cir.count("CX"), cir.n_faults, len(cir.detectors)) == (288, 10368, 262944, 936)
    assert (len(circuit.edge_layers(code.Hx)), len(circuit.edge_layers(code.Hz))) == (8, 8)


def test_layers_are_a_proper_colouring():
    for name in ("72", "hgp"):
        for H in (cc.code(name).Hx, cc.code(name).Hz):
            layers = circuit.edge_layers(H)
            assert sorted(e for layer in layers for e in layer) == [tuple(e) for e in np.argwhere(np.asarray(H) % 2)]
            for layer in layers:
                assert len({i for i, _ in layer}) == len(layer) == len({j for _, j in layer})


def test_detector_counts():
    assert len(cc.memory("72", 3).detectors) == 36 * 4
    assert len(cc.memory("72", 3, "Z", "all").detectors) == 36 * 4 + 36 * 2
    assert len(cc.memory("72", 3, "X", "basis").observables) == 12
    assert cc.memory("72", 2, "Z", "basis", False).count("DEP1") == 0


# ---- text and probabilities ---------------------------------------------------------------------------------------
def small_dem():
    key = ("steane", 2, "Z", "all")
    return circuit.dem_from_fault_rows(cc.memory(*key), *cc.fault_rows(key)[2:])


def test_to_text_round_trip():
    d = small_dem()
    for rates in (RATES, 0.003):
        H, L, p = dem_mod.parse_dem(d.to_text(rates))
        assert (H != d.H).nnz == 0 and H.shape == d.H.shape and np.array_equal(L, d.L)
        assert np.allclose(p, d.probs(rates), rtol=1e-15, atol=0)


def test_probs_against_a_direct_fold():
    key = ("steane", 2, "Z", "all")
    cir, d = cc.memory(*key), small_dem()
    sites, base = co.sites_of(cir)
    for rates in (RATES, [0.3, 0.6, 0.9, 0.75]):
        want = np.zeros(d.H.shape[1])
        for s, b in zip(sites, base):
            for f in range(b, b + s[4]):
                v = d.fault_column[f]
                if v >= 0:
                    q = rates[s[3]] / s[4]
                    want[v] = want[v] + q - 2.0 * want[v] * q
        assert np.allclose(d.probs(rates), want, rtol=1e-12, atol=0)


def test_to_stim_literal():
    text = cc.memory("422", 1).to_stim(dict(reset=0.125, cnot=0.25, idle=0.0625, meas=0.5))
    assert text == """R 0 1 2 3
X_ERROR(0.125) 0 1 2 3
RX 4
Z_ERROR(0.125) 4
R 5
X_ERROR(0.125) 5
CX 4 0
DEPOLARIZE2(0.25) 4 0
DEPOLARIZE1(0.0625) 1 2 3 5
CX 4 1
DEPOLARIZE2(0.25) 4 1
DEPOLARIZE1(0.0625) 0 2 3 5
CX 4 2
DEPOLARIZE2(0.25) 4 2
DEPOLARIZE1(0.0625) 0 1 3 5
CX 4 3
DEPOLARIZE2(0.25) 4 3
DEPOLARIZE1(0.0625) 0 1 2 5
CX 0 5
DEPOLARIZE2(0.25) 0 5
DEPOLARIZE1(0.0625) 1 2 3 4
CX 1 5
DEPOLARIZE2(0.25) 1 5
DEPOLARIZE1(0.0625) 0 2 3 4
CX 2 5
DEPOLARIZE2(0.25) 2 5
DEPOLARIZE1(0.0625) 0 1 3 4
CX 3 5
DEPOLARIZE2(0.25) 3 5
DEPOLARIZE1(0.0625) 0 1 2 4
Z_ERROR(0.5) 4
MX 4
X_ERROR(0.5) 5
M 5
X_ERROR(0.5) 0 1 2 3
M 0 1 2 3
DETECTOR rec[-5]
DETECTOR rec[-4] rec[-3] rec[-2] rec[-1] rec[-5]
""" + "".join(f"OBSERVABLE_INCLUDE({l}) " + " ".join(f"rec[-{4 - q}]" for q in np.flatnonzero(row)) + "\n"
              for l, row in enumerate(cc.code("422").Lz))


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_value_errors():
    with pytest.raises(ValueError, match="no logical"):
        circuit.memory_experiment("steane", 2)
    with pytest.raises(ValueError, match="rounds"):
        circuit.memory_experiment(cc.code("422"), 0)
    with pytest.raises(ValueError, match="basis"):
        circuit.memory_experiment(cc.code("422"), 1, basis="Y")
    with pytest.raises(ValueError, match="detectors"):
        circuit.memory_experiment(cc.code("422"), 1, detectors="none")
    Z = np.zeros((0, 65), np.int64)
    big = codes.Code("k65", Z, Z, np.eye(65, dtype=np.uint8), np.eye(65, dtype=np.uint8), 1)
    with pytest.raises(ValueError, match="64"):
        circuit.memory_experiment(big, 1)
    c = circuit.Circuit(2)
    for kind, targets in (("H", [0]), ("MZ", [2]), ("MZ", [-1]), ("CX", [0]), ("CX", [1, 1]), ("DEP2", [0, 0])):
        with pytest.raises(ValueError):
            c.append(kind, targets)
    with pytest.raises(ValueError):
        c.append("XERR", [0], 16)
    with pytest.raises(ValueError):
        circuit.Circuit(0)
    for bad in (1.0, -0.1, float("nan"), [0.1, 0.2], dict(reset=2.0), {99: 0.1}):
        with pytest.raises(ValueError):
            circuit.rates_array(bad, 4)
    assert circuit.rates_array(dict(cnot=0.25), 4).tolist() == [0.0, 0.25, 0.0, 0.0]
    with pytest.raises(ValueError):
        mc.run_circuit(cc.code("422"), 1, [0.01], 10, osd_order=3)         # an order without osd: before any GPU work
    with pytest.raises(ValueError):
        mc.run_circuit(cc.code("422"), 1, [0.01, 0.02], 10, rates=[0.01])


# ---- marginals ----------------------------------------------------------------------------------------------------
def test_detector_marginals_of_the_sampler():
    """[[72,12,6]] over 3 rounds, 20 000 oracle shots at p = 0.01, seed 1: every detector's firing frequency against
    (1 - prod_j (1 - 2 p_j)) / 2 over its row of the model, within 5 binomial sigma plus R^2 p^2, R the number of faults
    that flip it (what the independent fold ignores).  The oracle alone passes this: no GPU is involved.  That term is
    vacuous at these R, so the exact marginals are asserted as well, at 5 sigma alone (below)."""
    p, T, seed = 0.01, 20000, 1
    key = ("72", 3, "Z", "basis")
    cir = cc.memory(*key)
    det_f, _, bits, masks = cc.fault_rows(key)
    d = circuit.dem_from_fault_rows(cir, bits, masks)
    det, _ = co.sample(cir, [p] * 4, seed, 0, T)
    freq = det.mean(axis=0)
    A = d.H.toarray().astype(np.float64)
    want = (1.0 - np.prod(1.0 - 2.0 * A * d.probs(p)[None, :], axis=1)) / 2.0
    R = det_f.sum(axis=0).astype(np.float64)
    sigma = np.sqrt(want * (1.0 - want) / T)
    excess = np.abs(freq - want) - (5.0 * sigma + R ** 2 * p ** 2)
    print(f"largest |freq - model| / sigma = {(np.abs(freq - want) / sigma).max():.2f}; worst margin {excess.max():.2e}")
    assert (excess <= 0).all()
    # At these R (144 .. 650) the R^2 p^2 term is 2 or more, so the bound above cannot fail.  The sharp statement: sites
    # are independent and the faults of ONE site are disjoint, so a detector fires with probability exactly
    # (1 - prod_s (1 - 2 a_s)) / 2, a_s = the sum of q = p / K over the faults of site s that flip it (the floor in
    # thr = floor(p 2^32) moves a_s by less than 2^-32 a site: below 2e-7 in all).  5 binomial sigma, no further term.
    sites, _ = co.sites_of(cir)
    K = np.asarray([s[4] for s in sites])
    a = np.zeros((len(sites), det_f.shape[1]))
    np.add.at(a, np.repeat(np.arange(len(sites)), K), det_f * np.repeat(p / K, K)[:, None])
    exact = (1.0 - np.prod(1.0 - 2.0 * a, axis=0)) / 2.0
    s_exact = np.sqrt(exact * (1.0 - exact) / T)
    print(f"largest |freq - exact| / sigma = {(np.abs(freq - exact) / s_exact).max():.2f}")
    assert (np.abs(freq - exact) <= 5.0 * s_exact + 2e-7).all()
    # ... and the independent fold differs from that by at most sum_s a_s^2 (|prod x - prod y| <= sum |x_s - y_s| for
    # factors in [-1, 1], and 0 <= prod_f (1 - 2 q_f) - (1 - 2 a_s) <= 2 a_s^2): what CircuitDem.probs ignores
    assert (np.abs(want - exact) <= (a ** 2).sum(axis=0) + 1e-12).all() and (a ** 2).sum(axis=0).max() < 0.006
