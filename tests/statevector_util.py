"""Dense state-vector simulator for RZ / RX / CX / MZ / MX circuits with inserted Paulis -- TEST INFRASTRUCTURE.

The physics check of the frame rules, independent of them: amplitudes of 2^nq basis states (qubit q is bit q of the
index), projective measurements whose outcomes come from an rng, resets as measure-and-correct.  ``run`` returns the
measurement record; detectors and observables are XORs of its bits."""
import numpy as np


class State:
    def __init__(self, nq, rng):
        self.nq, self.rng = nq, rng
        self.a = np.zeros(1 << nq, np.complex128)
        self.a[0] = 1.0
        self.idx = np.arange(1 << nq)

    def x(self, q):
        self.a = self.a[self.idx ^ (1 << q)]

    def z(self, q):
        self.a = np.where((self.idx >> q) & 1, -self.a, self.a)

    def h(self, q):
        bit = (self.idx >> q) & 1
        self.a = (self.a[self.idx ^ (1 << q)] + np.where(bit, -self.a, self.a)) / np.sqrt(2.0)

    def cx(self, c, t):
        self.a = self.a[np.where((self.idx >> c) & 1, self.idx ^ (1 << t), self.idx)]

    def mz(self, q):
        bit = (self.idx >> q) & 1
        p1 = float((np.abs(self.a[bit == 1]) ** 2).sum())
        out = int(self.rng.random() < p1)
        self.a = np.where(bit == out, self.a, 0.0) / np.sqrt(p1 if out else 1.0 - p1)
        return out

    def pauli(self, q, p):
        """1 = X, 2 = Z, 3 = Y (X then Z: a global phase apart)."""
        if p & 1:
            self.x(q)
        if p & 2:
            self.z(q)


def run(circuit, rng, fault=None):
    """The measurement record uint8 [n_records] of one run.  ``fault`` = (site, 4-bit Pauli): that Pauli is inserted at
    that site (bits 0-1 on the site's first qubit, bits 2-3 on its second)."""
    s = State(circuit.nq, rng)
    rec, site = [], 0
    for kind, t, _ in circuit.ops:
        if kind == "RZ":
            for q in t:
                if s.mz(q):
                    s.x(q)
        elif kind == "RX":
            for q in t:
                s.h(q)
                if s.mz(q):
                    s.x(q)
                s.h(q)
        elif kind == "CX":
            for c, x in zip(t[::2], t[1::2]):
                s.cx(c, x)
        elif kind == "MZ":
            rec.extend(s.mz(q) for q in t)
        elif kind == "MX":
            for q in t:
                s.h(q)
                rec.append(s.mz(q))
                s.h(q)
        else:
            targets = list(zip(t[::2], t[1::2])) if kind == "DEP2" else [(q, -1) for q in t]
            for a, b in targets:
                if fault is not None and fault[0] == site:
                    s.pauli(a, fault[1] & 3)
                    if b >= 0:
                        s.pauli(b, fault[1] >> 2)
                site += 1
    return np.asarray(rec, np.uint8)
