"""Parity-check matrices of the codes the reference ships in ``codes/*.npz``.

``Hx``/``Hz`` of the five bivariate-bicycle (BB) codes are rebuilt from the
polynomials in the reference's ``generateCodeMatrices.py:5-46`` (closed form
``Hx = [A | B]``, ``Hz = [B^T | A^T]``); the Steane matrix
is the literal at ``generateCodeMatrices.py:64-68``.  The logical operators
``Lx`` have no closed form (they come from ``qldpc``'s ``get_logical_ops()``,
``generateCodeMatrices.py:52-57``), so they ship bit-packed in
``qldpc_amd/data/logicals.npz`` (made by ``tools/make_code_fixtures.py``).
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from . import gf2

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "logicals.npz")

# name -> (l, m, A terms, B terms); a term is (x power, y power)
BB_CODES = {
    "[[72, 12, 6]]": (6, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)]),
    "[[90, 8, 10]]": (15, 3, [(9, 0), (0, 1), (0, 2)], [(0, 0), (2, 0), (7, 0)]),
    "[[108, 8, 10]]": (9, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)]),
    "[[144, 12, 12]]": (12, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)]),
    "[[288, 12, 18]]": (12, 12, [(3, 0), (0, 2), (0, 7)], [(0, 3), (1, 0), (2, 0)]),
}
DISTANCES = {
    "[[72, 12, 6]]": 6,
    "[[90, 8, 10]]": 10,
    "[[108, 8, 10]]": 10,
    "[[144, 12, 12]]": 12,
    "[[288, 12, 18]]": 18,
}
ALIASES = {"72": "[[72, 12, 6]]", "90": "[[90, 8, 10]]", "108": "[[108, 8, 10]]",
           "144": "[[144, 12, 12]]", "288": "[[288, 12, 18]]"}

STEANE_H = np.array(
    [[1, 0, 1, 0, 1, 0, 1],
     [0, 1, 1, 0, 0, 1, 1],
     [0, 0, 0, 1, 1, 1, 1]], dtype=np.int64)


def _shift(k: int) -> np.ndarray:
    return np.roll(np.eye(k, dtype=np.int64), 1, axis=1)


def _poly(l: int, m: int, terms) -> np.ndarray:
    x = np.kron(_shift(l), np.eye(m, dtype=np.int64))
    y = np.kron(np.eye(l, dtype=np.int64), _shift(m))
    out = np.zeros((l * m, l * m), dtype=np.int64)
    for px, py in terms:
        out = out + np.linalg.matrix_power(x, px) @ np.linalg.matrix_power(y, py)
    return out % 2


def _bb_pair(l: int, m: int, a_terms, b_terms):
    A = _poly(l, m, a_terms)
    B = _poly(l, m, b_terms)
    return np.hstack([A, B]), np.hstack([B.T, A.T])


def bb_matrices(name: str):
    """Return ``(Hx, Hz)`` (int64 0/1) of a BB code by its reference name."""
    return _bb_pair(*BB_CODES[name])


@dataclass
class Code:
    name: str
    Hx: np.ndarray          # (m, n) int64 0/1
    Hz: np.ndarray
    Lx: np.ndarray | None   # (k, n) uint8, None for Steane (steane.npz has no logicals)
    Lz: np.ndarray | None
    distance: int | None

    @property
    def n(self) -> int:
        return self.Hx.shape[1]


def _bits(A, what: str) -> np.ndarray:
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError(f"{what} must be a matrix, got shape {A.shape}")
    return A.astype(np.int64) & 1


def _independent_modulo(base: np.ndarray, cand: np.ndarray) -> np.ndarray:
    """Indices of the rows of ``cand`` kept by one pass in ascending order: a row is kept when it is independent of
    the rows of ``base`` and the rows kept before it."""
    n = base.shape[1]
    R, piv = gf2.row_reduce(base)
    lead = {int(c): np.packbits(r) for c, r in zip(piv, R)}       # echelon basis: leading column -> packed row
    keep = []
    for i, row in enumerate(cand):
        v = np.packbits(row.astype(np.uint8))
        while True:
            nz = np.flatnonzero(v)
            if nz.size == 0:
                break
            b = int(nz[0])
            c = 8 * b + (8 - int(v[b]).bit_length())
            if c not in lead:
                lead[c] = v
                keep.append(i)
                break
            v = v ^ lead[c]
    assert all(c < n for c in lead)
    return np.asarray(keep, np.int64)


def css_logicals(Hx, Hz):
    """Logical operators of the CSS code ``(Hx, Hz)`` -> ``(Lx, Lz)``, uint8 ``[k][n]``, ``k = n - rank Hx - rank Hz``
    (two ``[0][n]`` arrays for ``k = 0``).  Host numpy only.

    ``Lx``: k rows of ``ker Hz``, independent modulo ``rowspace(Hx)`` -- the first such rows of ``gf2.nullspace(Hz)``
    in its order.  ``Lz``: k rows of ``ker Hx``, independent modulo ``rowspace(Hz)``, recombined so that
    ``Lx @ Lz.T % 2`` is the identity.  ``ValueError`` unless ``Hx @ Hz.T % 2 == 0``."""
    Hx, Hz = _bits(Hx, "Hx"), _bits(Hz, "Hz")
    if Hx.shape[1] != Hz.shape[1]:
        raise ValueError(f"Hx has {Hx.shape[1]} columns, Hz {Hz.shape[1]}")
    if ((Hx @ Hz.T) % 2).any():
        raise ValueError("Hx @ Hz.T % 2 is not zero: the X and Z checks do not commute")
    n = Hx.shape[1]
    Kz, Kx = gf2.nullspace(Hz), gf2.nullspace(Hx)
    Lx = Kz[_independent_modulo(Hx, Kz)]
    Lz = Kx[_independent_modulo(Hz, Kx)]
    k = n - gf2.rank(Hx) - gf2.rank(Hz)
    assert Lx.shape[0] == k and Lz.shape[0] == k
    if k == 0:
        return np.zeros((0, n), np.uint8), np.zeros((0, n), np.uint8)
    # Lx Lz^T = M is invertible (the pairing of the two quotient spaces is non-degenerate): Lz <- (M^-1)^T Lz
    M = (Lx.astype(np.int64) @ Lz.T.astype(np.int64)) % 2
    R, piv = gf2.row_reduce(np.hstack([M, np.eye(k, dtype=np.int64)]))
    assert R.shape[0] == k and np.array_equal(piv, np.arange(k))
    Minv = R[:, k:].astype(np.int64)
    Lz = ((Minv.T @ Lz.astype(np.int64)) % 2).astype(np.uint8)
    return np.ascontiguousarray(Lx, np.uint8), np.ascontiguousarray(Lz)


def from_matrices(Hx, Hz, name: str, distance: int | None = None) -> Code:
    """A ``Code`` of any commuting pair ``(Hx, Hz)`` with the logical operators of ``css_logicals``.  ``distance``
    None: not known yet -- ``distance.estimate`` sets an upper bound; the Monte-Carlo entries refuse the code until
    then."""
    Hx, Hz = _bits(Hx, "Hx"), _bits(Hz, "Hz")
    Lx, Lz = css_logicals(Hx, Hz)
    return Code(str(name), Hx, Hz, Lx, Lz, None if distance is None else int(distance))


def bb_code(l: int, m: int, a_terms, b_terms, name: str | None = None) -> Code:
    """The bivariate-bicycle code of any polynomial pair: ``bb_matrices`` for terms ``(x power, y power)`` over
    ``Z_l x Z_m``, ``Hx = [A | B]``, ``Hz = [B^T | A^T]``, logicals from ``css_logicals``, distance unknown."""
    a_terms = [(int(x), int(y)) for x, y in a_terms]
    b_terms = [(int(x), int(y)) for x, y in b_terms]
    Hx, Hz = _bb_pair(int(l), int(m), a_terms, b_terms)
    if name is None:
        name = f"bb(l={int(l)}, m={int(m)}, A={a_terms}, B={b_terms})"
    return from_matrices(Hx, Hz, name)


_BUILTIN = set(BB_CODES) | set(ALIASES) | {"steane"}
_REGISTERED: dict[str, Code] = {}


def register(code: Code) -> Code:
    """After it ``load_code(code.name)`` returns ``code`` (the object itself: a distance set later is seen by every
    later ``load_code``).  Registering a name again replaces the earlier code; a built-in name is a ``ValueError``."""
    if not isinstance(code, Code):
        raise TypeError(f"a codes.Code is needed, got {type(code).__name__}")
    if code.name in _BUILTIN:
        raise ValueError(f"{code.name!r} is a built-in code name")
    if code.name.endswith(".npz"):
        raise ValueError(f"{code.name!r} ends in .npz: load_code reads such a name as a file")
    _REGISTERED[code.name] = code
    return code


def _load_npz(path: str) -> Code:
    """The reference's ``codes/*.npz`` layout: ``Hx`` and ``Hz``, optionally ``Lx``, ``Lz`` and ``distance``."""
    with np.load(path) as d:
        if "Hx" not in d or "Hz" not in d:
            raise ValueError(f"{path} holds no Hx and Hz")
        Hx, Hz = _bits(d["Hx"], "Hx"), _bits(d["Hz"], "Hz")
        if ("Lx" in d) != ("Lz" in d):
            raise ValueError(f"{path} holds one of Lx and Lz: both or neither")
        logicals = (d["Lx"], d["Lz"]) if "Lx" in d else None
        distance = int(d["distance"]) if "distance" in d else None
    if logicals is None:
        return from_matrices(Hx, Hz, path, distance)
    if ((Hx @ Hz.T) % 2).any():
        raise ValueError(f"{path}: Hx @ Hz.T % 2 is not zero")
    Lx, Lz = ((_bits(L, w) if np.size(L) else np.zeros((0, Hx.shape[1]), np.int64)).astype(np.uint8)
              for L, w in zip(logicals, ("Lx", "Lz")))
    return Code(path, Hx, Hz, np.ascontiguousarray(Lx), np.ascontiguousarray(Lz), distance)


def load_code(name: str) -> Code:
    """The six built-in names: same content as ``np.load('codes/<name>.npz')`` in the reference.  Else a name given to
    ``register``, or a path ending in ``.npz`` (``_load_npz``)."""
    name = ALIASES.get(name, name)
    if name in _REGISTERED:
        return _REGISTERED[name]
    if name not in _BUILTIN and name.endswith(".npz"):
        return _load_npz(name)
    if name == "steane":
        return Code("steane", STEANE_H.copy(), STEANE_H.copy(), None, None, None)
    Hx, Hz = bb_matrices(name)
    # memory order as in the reference's files (Hx Fortran-ordered, Hz C-ordered): the order in which the
    # reference's dense decoders add up column sums follows it (qldpc_amd.bp.dense_colsum_flags)
    Hx = np.asfortranarray(Hx)
    n = Hx.shape[1]
    with np.load(_DATA) as d:
        k = int(d[f"{name}/k"])
        Lx = np.unpackbits(d[f"{name}/Lx"], axis=1)[:k, :n].astype(np.uint8)
        Lz = np.unpackbits(d[f"{name}/Lz"], axis=1)[:k, :n].astype(np.uint8)
    return Code(name, Hx, Hz, Lx, Lz, DISTANCES[name])


def code_names():
    return list(BB_CODES)
