"""The circuits of the circuit-level tests (tests/test_circuit_cpu.py, tests/test_gpu_circuit.py) -- TEST
INFRASTRUCTURE.  Every builder is cached; the oracle rows of a case are computed once and shared."""
import functools

import numpy as np

import circuit_oracle as co
from css_oracle import hgp_asymmetric
from qldpc_amd import circuit, codes

H422 = np.array([[1, 1, 1, 1]])


@functools.lru_cache(maxsize=None)
def code(name):
    if name == "422":
        return codes.from_matrices(H422, H422, "[[4,2,2]]", 2)
    if name == "steane":
        return codes.from_matrices(codes.STEANE_H, codes.STEANE_H, "steane-css", 3)
    if name == "hgp":                       # Hx 15 x 47, Hz 28 x 47 (tests/test_gpu_css_shapes.py): irregular layers
        Hx, Hz, Lx, Lz = hgp_asymmetric("wide_a")
        return codes.Code("hgp-wide-a", Hx.astype(np.int64), Hz.astype(np.int64), Lx, Lz, None)
    return codes.load_code(name)


@functools.lru_cache(maxsize=None)
def memory(name, rounds, basis="Z", detectors="basis", idle=True):
    return circuit.memory_experiment(code(name), rounds, basis=basis, idle=idle, detectors=detectors)


@functools.lru_cache(maxsize=None)
def reset_circuit():
    """Three qubits by hand: noise directly before a reset and directly after a measurement (those faults flip nothing
    and must be dropped), a fault that two CNOTs copy, and noise ops of all four kinds in rate classes 0 .. 4."""
    c = circuit.Circuit(3)
    c.append("RZ", [0, 1])
    c.append("RX", [2])
    c.append("XERR", [0], 0)               # flips the first MZ 0 and, through CX 0 1, MZ 1
    c.append("CX", [0, 1])
    c.append("DEP2", [0, 1], 1)
    c.append("DEP1", [2], 2)
    c.append("CX", [2, 1])
    r0 = c.append("MZ", [0])
    c.append("DEP1", [0], 3)               # directly after a measurement ...
    c.append("RZ", [0])                    # ... and directly before a reset: flips nothing
    c.append("ZERR", [2], 4)
    r1 = c.append("MZ", [1])
    r2 = c.append("MX", [2])
    r3 = c.append("MZ", [0])
    c.detector(r0)
    c.detector(r1 + r0)
    c.detector(r3)
    c.observable(r2)
    c.observable(r1)
    return c


@functools.lru_cache(maxsize=None)
def fault_rows(key):
    """Oracle rows of every fault of a case -> (det [F, m], obs [F, k], b8 rows, masks); read-only."""
    cir = reset_circuit() if key == "reset" else memory(*key)
    det, obs = co.faults(cir)
    bits, masks = co.pack(det, obs)
    for a in (det, obs, bits, masks):
        a.setflags(write=False)
    return det, obs, bits, masks
