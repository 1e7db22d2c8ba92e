"""Recorded shots of a detector error model: bit packing and stim's two plain sample formats, in pure numpy.

A shot is one row of detection events (m bits) and, if known, the observable flips that really happened (k bits).
``Decoder.decode_shots`` / ``mc.run_shots`` take the detection events bit-packed in stim's ``b8`` layout -- detector c
of a shot is bit ``c % 8`` of byte ``c // 8`` of its row, rows are ``ceil(m / 8)`` bytes, padding bits zero -- and the
observables as one uint64 mask per shot (bit l = observable l, k <= 64).  ``read_shots`` reads the files ``stim
sample_dem`` / ``stim detect`` write (``--out_format b8`` or ``01``), with the observables appended to every shot
(``--append_observables``) or in a file of their own (``--obs_out``).  stim itself is not needed.
"""
from __future__ import annotations

import numpy as np


def pack_bits(a) -> np.ndarray:
    """0/1 array [T, m] (any memory order) -> C-contiguous uint8 [T, ceil(m / 8)], bit c of a row at bit c % 8 of byte
    c // 8 (stim's b8)."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"pack_bits takes a [T, m] array, got shape {a.shape}")
    if a.dtype != np.bool_ and np.any((a != 0) & (a != 1)):
        raise ValueError("pack_bits takes 0/1 values")
    if a.shape[1] == 0:
        return np.zeros((a.shape[0], 0), np.uint8)
    # (np.packbits keeps the memory order of its input: a Fortran-ordered array would give strided rows)
    return np.ascontiguousarray(np.packbits(np.ascontiguousarray(a, np.uint8), axis=1, bitorder="little"))


def unpack_bits(packed, m) -> np.ndarray:
    """uint8 [T, ceil(m / 8)] -> uint8 0/1 [T, m] (padding bits are dropped, whatever they hold)."""
    p = np.asarray(packed)
    m = int(m)
    if p.ndim != 2 or p.dtype != np.uint8 or p.shape[1] != (m + 7) // 8:
        raise ValueError(f"unpack_bits({m} bits) takes a uint8 [T, {(m + 7) // 8}] array, got {p.dtype} {p.shape}")
    if m == 0:
        return np.zeros((p.shape[0], 0), np.uint8)
    return np.unpackbits(p, axis=1, count=m, bitorder="little")


def masks_of(obs) -> np.ndarray:
    """0/1 array [T, k], k <= 64 -> uint64 [T], bit l = observable l."""
    o = np.asarray(obs)
    if o.ndim != 2 or o.shape[1] > 64:
        raise ValueError(f"masks_of takes a [T, k <= 64] array, got shape {o.shape}")
    if o.dtype != np.bool_ and np.any((o != 0) & (o != 1)):
        raise ValueError("masks_of takes 0/1 values")
    out = np.zeros(o.shape[0], np.uint64)
    for l in range(o.shape[1]):
        out |= o[:, l].astype(np.uint64) << np.uint64(l)
    return out


def obs_of(masks, k) -> np.ndarray:
    """uint64 [T] -> uint8 0/1 [T, k]: the inverse of ``masks_of`` (bits from k on are dropped)."""
    mk = np.asarray(masks, np.uint64)
    k = int(k)
    if mk.ndim != 1 or not 0 <= k <= 64:
        raise ValueError(f"obs_of takes a uint64 [T] array and 0 <= k <= 64, got shape {mk.shape}, k = {k}")
    out = np.zeros((mk.shape[0], k), np.uint8)
    for l in range(k):
        out[:, l] = (mk >> np.uint64(l)) & np.uint64(1)
    return out


def _read_bits(path, bits, fmt):
    """One sample file -> uint8 0/1 [T, bits]."""
    with open(path, "rb") as f:
        raw = f.read()
    if fmt == "b8":
        rb = (bits + 7) // 8
        if rb == 0:
            raise ValueError(f"{path}: a b8 file of 0-bit shots does not say how many there are")
        if len(raw) % rb:
            raise ValueError(f"{path}: {len(raw)} bytes are not a whole number of {rb}-byte shots ({bits} bits each)")
        return unpack_bits(np.frombuffer(raw, np.uint8).reshape(-1, rb), bits)
    if fmt == "01":
        lines = raw.decode("ascii", "replace").split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        rows = np.zeros((len(lines), bits), np.uint8)
        for i, line in enumerate(lines):
            line = line.rstrip("\r")
            if len(line) != bits or line.strip("01"):
                raise ValueError(f"{path}: line {i + 1} is not {bits} characters of 0 / 1")
            rows[i] = np.frombuffer(line.encode("ascii"), np.uint8) - ord("0")
        return rows
    raise ValueError(f"shot format must be 'b8' or '01', got {fmt!r}")


def read_shots(path, m, k=0, fmt="b8", obs=None):
    """Shots in stim's ``b8`` or ``01`` format -> ``(det_bits uint8 [T, ceil(m / 8)], masks uint64 [T] or None)``.

    ``path``: the detection events, m bits per shot; with ``k > 0`` and no ``obs`` every shot carries its k
    observables behind them (``--append_observables``: m + k bits per shot).  ``obs``: a file of the same format with
    k bits per shot (``--obs_out``).  Without observables (k = 0 and no ``obs``) the masks are None.  ValueError for a
    file whose length does not fit, a bad character, k > 64, or files of different shot counts."""
    m, k = int(m), int(k)
    if m < 1 or not 0 <= k <= 64:
        raise ValueError(f"read_shots needs m >= 1 detectors and 0 <= k <= 64 observables, got m = {m}, k = {k}")
    if obs is not None and k < 1:
        raise ValueError("a separate observables file needs k >= 1")
    appended = k if obs is None else 0
    bits = _read_bits(path, m + appended, fmt)
    det = pack_bits(bits[:, :m])
    if obs is not None:
        ob = _read_bits(obs, k, fmt)
        if len(ob) != len(det):
            raise ValueError(f"{obs}: {len(ob)} shots, but {path} holds {len(det)}")
        return det, masks_of(ob)
    return det, (masks_of(bits[:, m:]) if k else None)


def write_shots(path, bits, fmt="b8"):
    """0/1 array [T, bits] -> a file ``read_shots`` (and stim) reads."""
    a = np.asarray(bits)
    if fmt == "b8":
        data = pack_bits(a).tobytes()
    elif fmt == "01":
        if a.ndim != 2:
            raise ValueError(f"write_shots takes a [T, bits] array, got shape {a.shape}")
        data = "".join("".join("1" if v else "0" for v in row) + "\n" for row in a).encode("ascii")
    else:
        raise ValueError(f"shot format must be 'b8' or '01', got {fmt!r}")
    with open(path, "wb") as f:
        f.write(data)
