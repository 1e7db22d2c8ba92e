"""Circuit-level noise for CSS codes: a small circuit IR, the memory experiment of a code, and its detector error model.

A ``Circuit`` holds resets, CNOTs and measurements in the Z and X bases, Pauli noise ops that carry a *rate class*
instead of a probability, and detectors and observables as lists of measurement-record indices.  The GPU Pauli-frame
simulator (``qbp_frame_*`` of include/qbp.h, which states the propagation rules in full) runs it for sampled shots
(``Circuit.sample``) or for every single fault (``circuit_dem``); rates are supplied per class when sampling or pricing,
so one circuit and one propagation serve every p.  Everything in this module but those two calls is host numpy.

Sites and faults.  A *site* is one target, or one pair, of one noise op; sites are numbered in op order, then target
order.  A site has K possible faults with codes 1 .. K: K = 1 for ``XERR`` (the Pauli X) and ``ZERR`` (the Pauli Z),
3 for ``DEP1`` (1 = X, 2 = Z, 3 = Y) and 15 for ``DEP2`` (``code & 3`` acts on the first qubit, ``code >> 2`` on the
second).  Faults are numbered by site, then by code; ``site_base[j]`` is the first fault of site j.

``Circuit.to_stim`` writes the circuit as stim text so that anyone who has stim can cross-check; stim is not installed
where this library is developed, so that text HAS NOT BEEN RUN AGAINST STIM -- it is tested as text only.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.sparse import csr_matrix

KINDS = dict(RZ=0, RX=1, CX=2, MZ=3, MX=4, XERR=5, ZERR=6, DEP1=7, DEP2=8)        # QBP_FRAME_* of include/qbp.h
PAIR_KINDS = ("CX", "DEP2")
NOISE_FAULTS = dict(XERR=1, ZERR=1, DEP1=3, DEP2=15)                              # K of a site
CLASSES = dict(reset=0, cnot=1, idle=2, meas=3)                                   # the rate classes memory_experiment uses
MAX_CLASSES = 16                                                                  # QBP_FRAME_MAX_CLASSES
_STIM = dict(RZ="R", RX="RX", CX="CX", MZ="M", MX="MX", XERR="X_ERROR", ZERR="Z_ERROR", DEP1="DEPOLARIZE1",
             DEP2="DEPOLARIZE2")


def rates_array(rates, n_classes=len(CLASSES)):
    """Rates per class as float64 [max(n_classes, 1 + largest class given)]: a number (every class), a sequence by
    class, or a dict keyed by class number or by a name of ``CLASSES`` (classes not named get 0).  ValueError for a
    rate that is negative, >= 1 or NaN."""
    if isinstance(rates, dict):
        keys = {CLASSES[c] if isinstance(c, str) else int(c): float(v) for c, v in rates.items()}
        if any(c < 0 or c >= MAX_CLASSES for c in keys):
            raise ValueError(f"rate classes are 0 .. {MAX_CLASSES - 1}")
        out = np.zeros(max([int(n_classes)] + [c + 1 for c in keys]), np.float64)
        for c, v in keys.items():
            out[c] = v
    elif np.ndim(rates) == 0:
        out = np.full(max(int(n_classes), 1), float(rates))
    else:
        out = np.ascontiguousarray(rates, np.float64).ravel()
        if out.size < n_classes:
            raise ValueError(f"{out.size} rates for {n_classes} rate classes")
    if not np.all((out >= 0.0) & (out < 1.0)):
        raise ValueError(f"rates must lie in [0, 1): {out}")
    return out


class Circuit:
    """``nq`` qubits and a list of ops ``(kind, targets, rate_class)``; ``detectors`` and ``observables`` are lists of
    lists of measurement-record indices (records are numbered in op order, then target order).  No H gates, no Y-basis
    ops, no feedback: CSS syndrome extraction needs none.  A circuit holds no probabilities."""

    def __init__(self, nq):
        self.nq = int(nq)
        if self.nq < 1:
            raise ValueError("a circuit needs at least one qubit")
        self.ops = []
        self.detectors = []
        self.observables = []
        self.n_records = 0
        self._sims = {}

    def append(self, kind, targets, rate_class=0):
        """Add one op; ``targets``: qubits, for ``CX`` and ``DEP2`` as pairs a0 b0 a1 b1 ...; ``rate_class`` is read
        for noise ops only.  Returns the record indices of a measurement op (else an empty list)."""
        if kind not in KINDS:
            raise ValueError(f"unknown op kind {kind!r} (one of {sorted(KINDS)})")
        t = [int(q) for q in np.asarray(targets, np.int64).ravel()]
        if any(q < 0 or q >= self.nq for q in t):
            raise ValueError(f"{kind}: a target outside [0, {self.nq})")
        if kind in PAIR_KINDS:
            if len(t) % 2:
                raise ValueError(f"{kind} takes pairs of qubits")
            if any(a == b for a, b in zip(t[::2], t[1::2])):
                raise ValueError(f"{kind}: a pair of equal qubits")
        cls = int(rate_class) if kind in NOISE_FAULTS else 0
        if not 0 <= cls < MAX_CLASSES:
            raise ValueError(f"rate class {cls} outside [0, {MAX_CLASSES})")
        self.ops.append((kind, tuple(t), cls))
        self._sims = {}
        if kind in ("MZ", "MX"):
            first = self.n_records
            self.n_records += len(t)
            return list(range(first, self.n_records))
        return []

    def detector(self, records):
        self.detectors.append([int(r) for r in records])
        self._sims = {}

    def observable(self, records):
        if len(self.observables) >= 64:
            raise ValueError("at most 64 observables")
        self.observables.append([int(r) for r in records])
        self._sims = {}

    # ---- tables -----------------------------------------------------------------------------------------------------
    def table(self):
        """The op table of qbp_frame_create, int32 [rows, 4]: (kind, q0, q1, rate class), one row per target or pair."""
        rows = []
        for kind, t, cls in self.ops:
            code = KINDS[kind]
            if kind in PAIR_KINDS:
                rows.extend((code, a, b, cls) for a, b in zip(t[::2], t[1::2]))
            else:
                rows.extend((code, q, 0, cls) for q in t)
        return np.asarray(rows, np.int32).reshape(-1, 4)

    def sites(self):
        """The sites as int64 arrays ``(kind, q0, q1, rate class, K, site_base)``; ``site_base`` has one entry more,
        the number of faults."""
        tab = self.table().astype(np.int64)
        s = tab[tab[:, 0] >= KINDS["XERR"]]
        K = np.choose(s[:, 0] - KINDS["XERR"], [1, 1, 3, 15]) if len(s) else np.zeros(0, np.int64)
        base = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
        return s[:, 0], s[:, 1], s[:, 2], s[:, 3], K.astype(np.int64), base

    @property
    def n_sites(self):
        return int(sum(len(t) // (2 if kind in PAIR_KINDS else 1) for kind, t, _ in self.ops if kind in NOISE_FAULTS))

    @property
    def n_faults(self):
        return int(sum(NOISE_FAULTS[kind] * (len(t) // (2 if kind in PAIR_KINDS else 1))
                       for kind, t, _ in self.ops if kind in NOISE_FAULTS))

    @property
    def n_classes(self):
        return 1 + max([cls for kind, _, cls in self.ops if kind in NOISE_FAULTS], default=-1)

    def count(self, kind):
        """Targets (pairs for ``CX`` and ``DEP2``) of the ops of one kind."""
        return sum(len(t) // (2 if kind in PAIR_KINDS else 1) for k, t, _ in self.ops if k == kind)

    def _csr(self, lists, what):
        for rec in lists:
            if any(r < 0 or r >= self.n_records for r in rec):
                raise ValueError(f"{what}: a record index outside [0, {self.n_records})")
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int32)
        idx = np.asarray([r for rec in lists for r in rec], np.int32)
        return ptr, idx

    def simulator(self, device=0):
        """The GPU Pauli-frame simulator of this circuit (``_lib.FrameSim``), built once per device."""
        from . import _lib
        if len(self.observables) > 64:
            raise ValueError("at most 64 observables")
        sim = self._sims.get(int(device))
        if sim is None:
            sim = _lib.FrameSim(self.nq, self.table(), *self._csr(self.detectors, "detector"),
                                *self._csr(self.observables, "observable"), device=device)
            self._sims[int(device)] = sim
        return sim

    def sample(self, shots, rates, seed=0, *, shot_begin=0, device=0):
        """``shots`` sampled shots on the GPU -> ``(det_bits uint8 [shots, ceil(m / 8)], masks uint64 [shots])`` on the
        host: b8 detection rows and observable masks, what ``mc.run_shots`` takes.  ``rates``: see ``rates_array``."""
        return self.simulator(device).sample(rates_array(rates, self.n_classes), int(shots), seed=seed,
                                             shot_begin=shot_begin)

    def to_stim(self, rates):
        """The circuit as stim text (``R``, ``RX``, ``CX``, ``M``, ``MX``, ``X_ERROR``, ``Z_ERROR``, ``DEPOLARIZE1``,
        ``DEPOLARIZE2``, then ``DETECTOR rec[-i]`` and ``OBSERVABLE_INCLUDE(l) rec[-i]`` lines at the end) with the
        rate of every noise op's class written in.  NOT RUN AGAINST STIM here (it is not installed): tested as text."""
        r = rates_array(rates, self.n_classes)
        lines = []
        for kind, t, cls in self.ops:
            head = f"{_STIM[kind]}({r[cls]:.17g})" if kind in NOISE_FAULTS else _STIM[kind]
            lines.append(" ".join([head] + [str(q) for q in t]))
        for rec in self.detectors:
            lines.append(" ".join(["DETECTOR"] + [f"rec[-{self.n_records - i}]" for i in rec]))
        for l, rec in enumerate(self.observables):
            lines.append(" ".join([f"OBSERVABLE_INCLUDE({l})"] + [f"rec[-{self.n_records - i}]" for i in rec]))
        return "\n".join(lines) + "\n"


def edge_layers(H):
    """CNOT layers of a check matrix: the deterministic greedy edge colouring of ``H % 2``.  Edges are visited by
    ascending check, then ascending column; each gets the smallest colour free at both its ends; layer c is the list of
    the ``(check, column)`` edges of colour c, in visiting order."""
    H = np.asarray(H, np.int64) & 1
    used_r = [set() for _ in range(H.shape[0])]
    used_c = [set() for _ in range(H.shape[1])]
    layers = []
    for i in range(H.shape[0]):
        for j in np.flatnonzero(H[i]):
            c = 0
            while c in used_r[i] or c in used_c[j]:
                c += 1
            used_r[i].add(c)
            used_c[j].add(c)
            while len(layers) <= c:
                layers.append([])
            layers[c].append((i, int(j)))
    return layers


def memory_experiment(code, rounds, basis="Z", idle=True, detectors="basis"):
    """The memory experiment of a CSS code (a ``codes.Code`` or a name ``codes.load_code`` knows) over ``rounds`` rounds
    of syndrome extraction, as a ``Circuit``.  Data qubits are 0 .. n - 1, the X-ancillas n .. n + mx - 1, the
    Z-ancillas follow.  For ``basis="Z"``:

      1. ``RZ`` on the data, then ``XERR`` (class ``reset``).
      2. Each round: ``RX`` on the X-ancillas, then ``ZERR`` (``reset``); ``RZ`` on the Z-ancillas, then ``XERR``
         (``reset``); the CNOT layers of Hx (``edge_layers``), control ancilla -> data; the CNOT layers of Hz, control
         data -> ancilla; after every layer ``DEP2`` (class ``cnot``) on its pairs and, with ``idle``, ``DEP1`` (class
         ``idle``) on every qubit of the circuit that is not in the layer; ``ZERR`` (class ``meas``) then ``MX`` on the
         X-ancillas; ``XERR`` (``meas``) then ``MZ`` on the Z-ancillas.
      3. ``XERR`` (``meas``) on the data, then ``MZ`` on the data.

    Detectors, ``"basis"``: round 0 each Z-check outcome, rounds t >= 1 ``Z_t ^ Z_{t-1}``, finally the parity of the data
    outcomes over each row of Hz ``^ Z_{T-1}`` -- ``mz (T + 1)`` of them; ``"all"`` appends ``X_t ^ X_{t-1}`` for
    t >= 1.  Observables: the rows of Lz on the data outcomes.  ``basis="X"`` is the mirror image in the data's
    preparation, measurement, detectors and observables (``RX`` / ``ZERR`` / ``MX`` on the data, X-checks, Lx); the
    rounds themselves are the same.  ValueError: a code without logicals, ``rounds < 1``, more than 64 logicals, or an
    unknown ``basis`` / ``detectors``."""
    from . import codes
    c = codes.load_code(code) if isinstance(code, str) else code
    if c.Lx is None or c.Lz is None:
        raise ValueError(f"code {c.name} has no logical operators")
    T = int(rounds)
    if T < 1:
        raise ValueError("rounds must be >= 1")
    if basis not in ("Z", "X"):
        raise ValueError(f"basis must be 'Z' or 'X', got {basis!r}")
    if detectors not in ("basis", "all"):
        raise ValueError(f"detectors must be 'basis' or 'all', got {detectors!r}")
    Hx, Hz = np.asarray(c.Hx, np.int64) & 1, np.asarray(c.Hz, np.int64) & 1
    logicals = np.asarray(c.Lz if basis == "Z" else c.Lx, np.int64) & 1
    if logicals.shape[0] > 64:
        raise ValueError(f"at most 64 observables (k = {logicals.shape[0]})")
    n, mx, mz = Hx.shape[1], Hx.shape[0], Hz.shape[0]
    data, xa, za = list(range(n)), list(range(n, n + mx)), list(range(n + mx, n + mx + mz))
    nq = n + mx + mz
    R, CN, ID, ME = (CLASSES[x] for x in ("reset", "cnot", "idle", "meas"))
    layers = [[(n + i, j) for i, j in layer] for layer in edge_layers(Hx)]              # ancilla -> data
    layers += [[(j, n + mx + i) for i, j in layer] for layer in edge_layers(Hz)]        # data -> ancilla
    cir = Circuit(nq)
    cir.append("RZ" if basis == "Z" else "RX", data)
    cir.append("XERR" if basis == "Z" else "ZERR", data, R)
    xrec, zrec = [], []
    for _ in range(T):
        cir.append("RX", xa)
        cir.append("ZERR", xa, R)
        cir.append("RZ", za)
        cir.append("XERR", za, R)
        for layer in layers:
            pairs = [q for ab in layer for q in ab]
            cir.append("CX", pairs)
            cir.append("DEP2", pairs, CN)
            if idle:
                busy = set(pairs)
                rest = [q for q in range(nq) if q not in busy]
                if rest:
                    cir.append("DEP1", rest, ID)
        cir.append("ZERR", xa, ME)
        xrec.append(cir.append("MX", xa))
        cir.append("XERR", za, ME)
        zrec.append(cir.append("MZ", za))
    cir.append("XERR" if basis == "Z" else "ZERR", data, ME)
    drec = cir.append("MZ" if basis == "Z" else "MX", data)
    own, other, Hown = (zrec, xrec, Hz) if basis == "Z" else (xrec, zrec, Hx)
    for j in range(Hown.shape[0]):
        cir.detector([own[0][j]])
    for t in range(1, T):
        for j in range(Hown.shape[0]):
            cir.detector([own[t][j], own[t - 1][j]])
    for j in range(Hown.shape[0]):
        cir.detector([drec[q] for q in np.flatnonzero(Hown[j])] + [own[T - 1][j]])
    if detectors == "all":
        for t in range(1, T):
            for j in range(len(other[0])):
                cir.detector([other[t][j], other[t - 1][j]])
    for row in logicals:
        cir.observable([drec[q] for q in np.flatnonzero(row)])
    return cir


@dataclass
class CircuitDem:
    """The detector error model of a circuit: column v of ``H`` (csr uint8 [m, n], sorted indices) and ``L`` (uint8
    [k, n]) is a set of merged single faults.  ``kinds`` int64 [n_kinds, 2] lists the (rate class, K) pairs that occur
    and ``counts`` int64 [n, n_kinds] how many faults of each went into a column; ``fault_column`` int64 [faults] is
    the column of every fault, -1 for a fault that flips nothing."""
    H: csr_matrix
    L: np.ndarray
    kinds: np.ndarray
    counts: np.ndarray
    fault_column: np.ndarray

    def probs(self, rates):
        """Probability of every column for rates per class (``rates_array``): the fold of q = rate[class] / K over
        the column's faults with p (+) q = p + q - 2 p q, i.e. 1 - 2 p = prod (1 - 2 q).  Faults are treated as
        INDEPENDENT events.  This is not stim's disjoint-channel correction, which prices the 3 (15) outcomes of a
        depolarizing channel as mutually exclusive; the two differ in O(p^2)."""
        r = rates_array(rates, 1 + int(self.kinds[:, 0].max(initial=-1)))
        q = r[self.kinds[:, 0]] / self.kinds[:, 1]
        f = 1.0 - 2.0 * q
        cnt = self.counts.astype(np.float64)
        with np.errstate(divide="ignore"):
            logf = np.log(np.abs(f))                      # (-inf where q is exactly 1/2)
        logs = (cnt * np.where(self.counts > 0, logf[None, :], 0.0)).sum(axis=1)      # (no 0 * -inf)
        odd = ((self.counts & 1) * (f < 0)[None, :]).sum(axis=1) & 1
        sign = np.where(odd, -1.0, 1.0)
        return np.where(sign > 0, -np.expm1(logs) * 0.5, (1.0 + np.exp(logs)) * 0.5)

    def to_text(self, rates):
        """DEM text that ``dem.parse_dem`` reads back to the same ``(H, L, probs(rates))``: one ``error(p)`` line per
        column (%.17g), then a ``detector`` and a ``logical_observable`` line naming the last index of each."""
        p = self.probs(rates)
        Hc = self.H.tocsc()
        Hc.sort_indices()
        lines = []
        for v in range(self.H.shape[1]):
            dets = Hc.indices[Hc.indptr[v]:Hc.indptr[v + 1]]
            tok = [f"D{d}" for d in dets] + [f"L{l}" for l in np.flatnonzero(self.L[:, v])]
            lines.append(f"error({p[v]:.17g}) " + " ".join(tok))
        if self.H.shape[0]:
            lines.append(f"detector D{self.H.shape[0] - 1}")
        if self.L.shape[0]:
            lines.append(f"logical_observable L{self.L.shape[0] - 1}")
        return "\n".join(lines) + "\n"


def dem_from_fault_rows(circuit, det_bits, masks):
    """Rows of every single fault (``det_bits`` uint8 [faults, ceil(m / 8)], ``masks`` uint64 [faults], in fault order)
    -> ``CircuitDem``.  Faults that flip nothing are dropped; faults with equal (detectors, observables) merge into one
    column; columns keep the order of first appearance in fault order -- ``dem.parse_dem``'s rule."""
    m, k = len(circuit.detectors), len(circuit.observables)
    det = np.ascontiguousarray(det_bits, np.uint8)
    masks = np.ascontiguousarray(masks, np.uint64)
    F = circuit.n_faults
    if det.shape != (F, (m + 7) // 8) or masks.shape != (F,):
        raise ValueError(f"rows of {F} faults and {m} detectors are needed, got {det.shape} and {masks.shape}")
    _, _, _, cls, K, base = circuit.sites()
    kind_id = np.repeat(cls * 16 + K, K)                                  # per fault
    key = np.ascontiguousarray(np.concatenate([det, masks.view(np.uint8).reshape(F, 8)], axis=1))
    live = np.flatnonzero(key.any(axis=1))
    kv = np.ascontiguousarray(key[live]).view(np.dtype((np.void, key.shape[1]))).ravel()
    _, first, inv = np.unique(kv, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    col = rank[np.asarray(inv).ravel()]
    head = live[first[order]]                                             # the first fault of every column
    n = head.size
    fault_column = np.full(F, -1, np.int64)
    fault_column[live] = col
    bits = np.unpackbits(det[head], axis=1, bitorder="little")[:, :m]     # [n, m]
    H = csr_matrix(bits.T.astype(np.uint8))
    H.sort_indices()
    L = ((masks[head][None, :] >> np.arange(k, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(np.uint8)
    ids = np.unique(kind_id)
    counts = np.zeros((n, ids.size), np.int64)
    np.add.at(counts, (col, np.searchsorted(ids, kind_id[live])), 1)
    kinds = np.stack([ids // 16, ids % 16], axis=1).astype(np.int64)
    return CircuitDem(H, L.reshape(k, n), kinds, counts, fault_column)


FAULT_PHILOX_STREAM = 6          # QBP_FAULT_PHILOX_STREAM
FAULT_WEIGHT_MAX = 256           # QBP_FAULT_WEIGHT_MAX
_M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words, key (lo32(seed), hi32(seed)) -> the four output words."""
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _class_set(classes):
    """Rate classes given as numbers or names of ``CLASSES`` -> a set of numbers; None stays None (every class)."""
    if classes is None:
        return None
    out = {CLASSES[c] if isinstance(c, str) else int(c) for c in classes}
    if any(c < 0 or c >= MAX_CLASSES for c in out):
        raise ValueError(f"rate classes are 0 .. {MAX_CLASSES - 1}")
    return out


def fault_sites(circuit, classes=None):
    """The ACTIVE sites of a fixed-weight fault run: ``(first_fault int64 [N], K int64 [N], N)`` of the sites whose rate
    class is in ``classes`` (numbers or names of ``CLASSES``; None: every class), in site order; ``first_fault`` is
    the site's first fault in the circuit's fault numbering.  A class left out means rate 0: its sites never fire and
    do not count towards N."""
    _, _, _, cls, K, base = circuit.sites()
    keep = _class_set(classes)
    on = np.ones(len(K), bool) if keep is None else np.isin(cls, sorted(keep))
    return np.ascontiguousarray(base[:-1][on]), np.ascontiguousarray(K[on]), int(on.sum())


def fault_sets(circuit, weight, seed, trials, classes=None):
    """The faults of the trials of a fixed-weight fault run (include/qbp.h, qbp_mc_run_fault_weight, which states the
    sampler): int64 [len(trials), weight] fault numbers, column i the fault of step i.  ``trials``: global trial
    indices.  Fault f belongs to the site j with ``site_base[j] <= f < site_base[j + 1]`` of ``circuit.sites()`` and
    has code ``f - site_base[j] + 1``.
    ValueError: a weight outside [0, min(N, FAULT_WEIGHT_MAX)]."""
    first, K, N = fault_sites(circuit, classes)
    w, seed = int(weight), int(seed)
    if not 0 <= w <= min(N, FAULT_WEIGHT_MAX):
        raise ValueError(f"weight {w} out of [0, {min(N, FAULT_WEIGHT_MAX)}] (min of {N} active sites and "
                         f"FAULT_WEIGHT_MAX)")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    t = np.asarray(trials, np.int64).ravel().astype(np.uint64)
    T = t.size
    lo, hi = t & _M32, t >> np.uint64(32)
    stream = np.full(T, FAULT_PHILOX_STREAM, np.uint64)
    sites = np.zeros((T, w), np.int64)
    out = np.zeros((T, w), np.int64)
    Ku = K.astype(np.uint64)
    for i in range(w):
        if i % 4 == 0:
            block = np.full(T, i // 4, np.uint64)
            pick = _philox4x32_10(lo, hi, block, stream, seed)
            code = _philox4x32_10(lo, hi, block | np.uint64(0x80000000), stream, seed)
        j = N - w + i
        u = ((pick[i % 4] * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        s = np.where((sites[:, :i] == u[:, None]).any(axis=1), j, u)
        sites[:, i] = s
        out[:, i] = first[s] + ((code[i % 4] * Ku[s]) >> np.uint64(32)).astype(np.int64)
    return out


def circuit_dem(circuit, device=0):
    """The detector error model of ``circuit``: every single fault is propagated on the GPU (qbp_frame_faults), then
    ``dem_from_fault_rows`` drops, merges and counts on the host."""
    det, masks = circuit.simulator(device).faults(0, circuit.n_faults)
    return dem_from_fault_rows(circuit, det, masks)
