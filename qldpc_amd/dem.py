"""Detector error models (DEMs) as matrices for the Monte-Carlo loop (``mc.run_dem``, ``qbp_mc_run_probs``).

A DEM lists independent error mechanisms, each with its own probability, the detectors it flips and the logical
observables it flips.  ``parse_dem`` turns its text into ``(H, L, probs)``: column v of the check matrix H and of
the observable matrix L is mechanism v, flipped with probability probs[v].  This is what
``stim``'s ``detector_error_model_to_check_matrices`` hands the reference's circuit-level study
(studies/studyComplete.py:80-103), read from the text form so that stim is not needed here.

``phenomenological`` builds the phenomenological space-time model of a code (spaceTime.py:4-18 with a separate
measurement-error rate q), the model studies/studyTT.py decodes on.
"""
from __future__ import annotations

import os
import re

import numpy as np
from scipy.sparse import csr_matrix, eye, hstack, kron

_HEAD = re.compile(r"^([A-Za-z_]+)(?:\[[^\]]*\])?(?:\(([^)]*)\))?(.*)$")


def _parse_lines(lines, pos, depth):
    """Block of (line number, text, instruction, args, targets, body) up to the matching '}'."""
    out = []
    while pos < len(lines):
        no, raw = lines[pos]
        pos += 1
        text = raw.split("#", 1)[0].strip()
        if not text:
            continue
        if text == "}":
            if depth == 0:
                raise ValueError(f"DEM line {no}: '}}' without a repeat block")
            return out, pos
        m = _HEAD.match(text)
        if not m:
            raise ValueError(f"DEM line {no}: cannot parse {raw.strip()!r}")
        name, args, rest = m.group(1).lower(), m.group(2), m.group(3).split()
        body = None
        if name == "repeat":
            if not rest or rest[-1] != "{":
                raise ValueError(f"DEM line {no}: repeat needs '{{' at the end of the line: {raw.strip()!r}")
            rest = rest[:-1]
            body, pos = _parse_lines(lines, pos, depth + 1)
        out.append((no, raw.strip(), name, args, rest, body))
    if depth:
        raise ValueError("DEM: a repeat block is not closed")
    return out, pos


def _index(tok, prefix, no, raw):
    if len(tok) < 2 or tok[0] not in prefix or not tok[1:].isdigit():
        raise ValueError(f"DEM line {no}: bad target {tok!r} in {raw!r}")
    return int(tok[1:])


def _count(rest, no, raw, what):
    if len(rest) != 1 or not rest[0].isdigit():
        raise ValueError(f"DEM line {no}: {what} needs one non-negative integer: {raw!r}")
    return int(rest[0])


def parse_dem(text):
    """DEM text -> (H: csr_matrix uint8 [m, n], L: uint8 [k, n], probs: float64 [n]).

    Understands ``error(p)`` with targets ``D#``, ``L#`` and ``^`` (the mechanism is the symmetric difference of
    its components), ``detector`` and ``logical_observable`` (coordinates ignored; the indices count toward m and
    k), ``shift_detectors``, nested ``repeat N { }`` and ``#`` comments; anything else raises ValueError naming
    the line.  Mechanisms with the same (detectors, observables) merge, p <- p + q - 2pq, and columns keep the
    order of first appearance.  A mechanism that flips observables but no detector stays in (an empty column of
    H: an undetectable logical error); one that flips nothing is dropped."""
    lines = list(enumerate(str(text).splitlines(), start=1))
    prog, _ = _parse_lines(lines, 0, 0)
    cols = {}                 # (detectors, observables) -> column index
    probs = []
    m = k = 0
    offset = 0

    def run(block):
        nonlocal m, k, offset
        for no, raw, name, args, rest, body in block:
            if name == "error":
                try:
                    p = float(args)
                except (TypeError, ValueError):
                    raise ValueError(f"DEM line {no}: error needs one probability: {raw!r}") from None
                if not 0.0 <= p <= 1.0:
                    raise ValueError(f"DEM line {no}: probability {p} out of [0, 1]: {raw!r}")
                dets, obs = set(), set()
                prev_sep = True
                for tok in rest:
                    if tok == "^":
                        if prev_sep:
                            raise ValueError(f"DEM line {no}: misplaced '^' in {raw!r}")
                        prev_sep = True
                        continue
                    prev_sep = False
                    if tok[:1] == "D":        # (an index counts toward m and k even where it cancels)
                        d = offset + _index(tok, "D", no, raw)
                        dets ^= {d}
                        m = max(m, d + 1)
                    else:
                        o = _index(tok, "L", no, raw)
                        obs ^= {o}
                        k = max(k, o + 1)
                if rest and prev_sep:
                    raise ValueError(f"DEM line {no}: misplaced '^' in {raw!r}")
                if not dets and not obs:
                    continue                                  # flips nothing
                key = (tuple(sorted(dets)), tuple(sorted(obs)))
                j = cols.get(key)
                if j is None:
                    cols[key] = len(probs)
                    probs.append(p)
                else:
                    q = probs[j]
                    probs[j] = q + p - 2.0 * q * p
            elif name == "detector":
                for tok in rest:
                    m = max(m, offset + _index(tok, "D", no, raw) + 1)
            elif name == "logical_observable":
                for tok in rest:
                    k = max(k, _index(tok, "L", no, raw) + 1)
            elif name == "shift_detectors":
                offset += _count(rest, no, raw, "shift_detectors")
            elif name == "repeat":
                for _ in range(_count(rest, no, raw, "repeat")):
                    run(body)
            else:
                raise ValueError(f"DEM line {no}: unsupported instruction {name!r}: {raw!r}")

    run(prog)
    n = len(probs)
    rows, cidx = [], []
    L = np.zeros((k, n), np.uint8)
    for (dets, obs), j in cols.items():
        rows.extend(dets)
        cidx.extend([j] * len(dets))
        L[list(obs), j] = 1
    H = csr_matrix((np.ones(len(rows), np.uint8), (np.asarray(rows, np.int64), np.asarray(cidx, np.int64))),
                   shape=(m, n), dtype=np.uint8)
    H.sort_indices()
    return H, L, np.asarray(probs, np.float64)


def load_dem(x):
    """``parse_dem`` of a path (str or os.PathLike naming an existing file), of DEM text, or of any object whose
    ``str()`` is DEM text (e.g. a ``stim.DetectorErrorModel``)."""
    if isinstance(x, os.PathLike) or (isinstance(x, str) and "\n" not in x and os.path.isfile(x)):
        with open(x) as f:
            return parse_dem(f.read())
    return parse_dem(str(x))


def phenomenological(code, rounds, p, q=None):
    """Phenomenological space-time model of ``code`` (a ``codes.Code`` or a name ``codes.load_code`` knows) over
    ``rounds`` rounds: (H csr uint8 [m T, n T + m T], L uint8 [k, n T + m T], probs float64).

    H = [I_T (x) Hx | I + shift] as spaceTime.py:4-18 builds it (the data columns of every round, then the
    measurement columns; measurement error j flips checks j and j + m); L = [Lx ... Lx | 0]; probs is p on the
    data columns and q (default p) on the measurement columns."""
    from . import codes
    c = codes.load_code(code) if isinstance(code, str) else code
    if c.Lx is None:
        raise ValueError(f"code {c.name} has no logical operators")
    T = int(rounds)
    if T < 1:
        raise ValueError("rounds must be >= 1")
    q = p if q is None else q
    Hx = csr_matrix(np.asarray(c.Hx, np.uint8))
    mx, n = Hx.shape
    spatial = kron(eye(T, dtype=np.uint8, format="csr"), Hx, format="csr")
    temporal = eye(mx * T, dtype=np.uint8, format="csr") + eye(mx * T, k=-mx, dtype=np.uint8, format="csr")
    H = hstack([spatial, temporal], format="csr").astype(np.uint8)
    H.sort_indices()
    L = np.hstack([np.tile(np.asarray(c.Lx, np.uint8), (1, T)), np.zeros((c.Lx.shape[0], mx * T), np.uint8)])
    probs = np.concatenate([np.full(n * T, float(p)), np.full(mx * T, float(q))])
    return H, L, probs
