"""The circuits of the fixed-weight fault tests (tests/test_fault_weight_cpu.py, tests/test_gpu_fault_weight.py) -- TEST
INFRASTRUCTURE.  Builders are cached; the oracle tables of a case are computed once, shared and read-only."""
import functools

import numpy as np

import circuit_cases
import circuit_oracle as co
from qldpc_amd import circuit


@functools.lru_cache(maxsize=None)
def hand_circuit():
    """(a) Three qubits by hand: the four noise kinds, two rate classes (0 and 1), nine sites, and faults that flip
    nothing -- a Z on a qubit that is measured in Z and never a control (the ZERR on 1, the Z and half the Y of the DEP1
    on 1), an X directly before a reset (the XERR on 0 at the end), and the codes of the DEP2 whose Paulis are of that
    kind."""
    c = circuit.Circuit(3)
    c.append("RZ", [0, 1])
    c.append("RX", [2])
    c.append("XERR", [0, 1], 0)            # sites 0, 1
    c.append("ZERR", [2], 1)               # site 2
    c.append("CX", [0, 1])
    c.append("DEP2", [0, 1], 1)            # site 3
    c.append("CX", [2, 1])
    c.append("DEP1", [0, 2], 0)            # sites 4, 5
    c.append("ZERR", [1], 1)               # site 6: flips nothing
    r1 = c.append("MZ", [1])
    c.append("DEP1", [1], 0)               # site 7: after its measurement, nothing reads qubit 1 again
    r0 = c.append("MZ", [0])
    c.append("XERR", [0], 1)               # site 8: directly before a reset
    c.append("RZ", [0])
    r2 = c.append("MX", [2])
    r3 = c.append("MZ", [0])
    c.detector(r0)
    c.detector(r1 + r0)
    c.detector(r3)
    c.observable(r2)
    c.observable(r1)
    return c


CASES = ("hand", "steane2", "72x2")


@functools.lru_cache(maxsize=None)
def circuit_of(case):
    if case == "hand":
        return hand_circuit()
    if case == "steane1":
        return circuit_cases.memory("steane", 1)
    if case == "steane2":
        return circuit_cases.memory("steane", 2)
    if case == "72x2":
        return circuit_cases.memory("[[72, 12, 6]]", 2, "Z", "all")
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def oracle_dem(case):
    """(det [F, m], obs [F, k], H [m, n], L [k, n], fault_column [F]) by the numpy frame simulator and its merge."""
    det, obs = co.faults(circuit_of(case))
    H, L, col = co.merge(det, obs)
    for a in (det, obs, H, L, col):
        a.setflags(write=False)
    return det, obs, H, L, col


def masked_table(cir, classes):
    """(first_fault, K, N) of the sites in ``classes``, by a walk over the oracle's site list."""
    sites, base = co.sites_of(cir)
    keep = [j for j, s in enumerate(sites) if s[3] in classes]
    return base[:-1][keep].astype(np.int64), np.asarray([sites[j][4] for j in keep], np.int64), len(keep)
