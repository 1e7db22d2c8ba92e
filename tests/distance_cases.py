"""Cases shared by tests/test_distance_cpu.py and tests/test_gpu_distance.py: (H, G, L, seed, trial range) and the
numpy statement's output on each (tests/distance_oracle.py), computed once per name and left unchanged."""
import numpy as np

import distance_oracle as do
import lsd_util as lu
from qldpc_amd import codes, gf2


class Case:
    def __init__(self, H, G, L, seed=0, begin=0, trials=16):
        self.H = np.ascontiguousarray(np.asarray(H).astype(np.int64) & 1, np.uint8)
        self.G = np.ascontiguousarray(G, np.uint8)
        self.L = np.ascontiguousarray(L, np.uint8)
        self.n = self.H.shape[1]
        self.seed, self.begin, self.trials = int(seed), int(begin), int(trials)
        assert not (self.H.astype(np.int64) @ self.G.T % 2).any()


def _code(name, side):
    c = codes.load_code(name)
    return (c.Hx, c.Lx) if side == "x" else (c.Hz, c.Lz)


def _boundary(n, r, seed):
    """Random sparse H, 36 rows and n columns of weight 3 (the one-class matrices of tests/fuzz_records_util.py: no
    empty column, so no weight-1 vector in ker H); G: r rows of ker H -- a basis, then random sums of basis rows."""
    rng = np.random.default_rng([seed, n, r])
    H = np.zeros((36, n), np.uint8)
    for v in range(n):
        H[rng.choice(36, 3, replace=False), v] = 1
    B = gf2.nullspace(H)
    assert B.shape[0] <= r
    extra = (rng.random((r - B.shape[0], B.shape[0])) < 0.1).astype(np.int64) @ B.astype(np.int64) % 2
    return Case(H, np.vstack([B, extra]), rng.random((3, n)) < 0.3, seed=seed, trials=12)


def _make(name):
    if name == "steane":
        H = codes.STEANE_H
        return Case(H, gf2.nullspace(H), codes.css_logicals(H, H)[0], trials=64)
    if name == "72x":
        H, L = _code("[[72, 12, 6]]", "x")
        return Case(H, gf2.nullspace(H), L, trials=64)
    if name == "72z":                                    # trial indices across 2^32, a seed above 2^32
        H, L = _code("[[72, 12, 6]]", "z")
        return Case(H, gf2.nullspace(H), L, seed=(9 << 32) + 5, begin=(1 << 32) - 20, trials=48)
    if name == "144":
        H, L = _code("[[144, 12, 12]]", "x")
        return Case(H, gf2.nullspace(H), L, trials=128)
    if name == "rand37":                                 # the irregular 20 x 37 matrix of the other record tests
        H = lu.irregular37()
        rng = np.random.default_rng(37)
        return Case(H, gf2.nullspace(H), rng.random((5, 37)) < 0.4, seed=7, trials=40)
    if name == "dup":                                    # duplicated and zero rows appended
        H, L = _code("[[72, 12, 6]]", "x")
        G = gf2.nullspace(H)
        return Case(H, np.vstack([G, G[:5], np.zeros((2, 72), np.uint8), G[3] ^ G[4], G[::-1][:3]]), L, seed=3, trials=24)
    if name == "k64":                                    # k = 64, the only detecting row on bit 63
        H, L = _code("[[72, 12, 6]]", "x")
        H = np.asarray(H)
        return Case(H, gf2.nullspace(H), np.vstack([np.resize(H, (63, 72)), L[:1]]), seed=11, trials=16)
    if name == "nothing":                                # an L that detects nothing: rows of H
        H, _ = _code("[[72, 12, 6]]", "x")
        H = np.asarray(H)
        return Case(H, gf2.nullspace(H), H[:3], seed=1, trials=8)
    if name == "passes":                                 # more trials than workgroups at one per CU (256 CUs)
        H = codes.STEANE_H
        return Case(H, gf2.nullspace(H), codes.css_logicals(H, H)[0], seed=5, begin=100, trials=700)
    if name.startswith("n"):                             # n64_r64, n64_r65, n65_r64, n65_r65
        n, r = (int(x[1:]) for x in name.split("_"))
        return _boundary(n, r, 20261021)
    raise KeyError(name)


BOUNDARY = ("n64_r64", "n64_r65", "n65_r64", "n65_r65")
PARITY = ("steane", "72x", "72z", "rand37", "144", "dup", "k64") + BOUNDARY
_CASES, _STATEMENTS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _make(name)
    return _CASES[name]


def statement(name):
    """The statement's output on a case (shared: do not write to it)."""
    if name not in _STATEMENTS:
        c = case(name)
        _STATEMENTS[name] = do.search(c.G, c.L, c.seed, c.begin, c.begin + c.trials)
    return _STATEMENTS[name]
