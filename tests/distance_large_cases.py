"""Cases of the distance search at the limits of dist_search_kernel (qbp_distance.hpp), shared by
tests/test_distance_large_cpu.py and tests/test_gpu_distance_large.py: 32 rows per lane, many words per row, a sweep
that runs out of columns, equal sort keys, a state of exactly 160 KiB, n below the smallest sort width, a detector
error model.  (H, G, L, seed, trial range) and the numpy statement's output on each (tests/distance_oracle.py),
computed once per name and left unchanged.  tests/test_distance_large_cpu.py asserts what is claimed here."""
import numpy as np

import distance_oracle as do
from distance_cases import Case
from qldpc_amd import codes, gf2

LDS_LIMIT = 160 * 1024

# Two columns with the same 32-bit Philox key, found with do.column_keys on the CPU and pinned here:
# (seed, trial, n) -> (position q of the first in the sorted order, the columns a < b at q and q + 1)
TIE_512 = dict(seed=0, trial=11297, n=512, q=105, a=289, b=489)
TIE_16384 = dict(seed=0, trial=20, n=16384, q=13008, a=630, b=10382)


def lds_bytes(r, n):
    """dist_lds_bytes of qbp_distance.hpp, rounded up to 16 as the host entry does -> (bytes, W, NP)."""
    W, NP = (n + 31) // 32, max(4, 1 << (n - 1).bit_length())
    return (((max(8 * NP, 4 * r * (W + 1)) + 7) & ~7) + 2 * NP + 15) & ~15, W, NP


def two_column_H(n):
    """One check on columns 0 and 1: any G with those two columns zero lies in ker H."""
    H = np.zeros((1, n), np.uint8)
    H[0, :2] = 1
    return H


def _sparse_H(rng, m, n):
    """m x n, every column of weight 3 and no two columns equal: no vector of weight 1 or 2 in ker H."""
    H = np.zeros((m, n), np.uint8)
    seen = set()
    for v in range(n):
        while True:
            rows = tuple(sorted(rng.choice(m, 3, replace=False).tolist()))
            if rows not in seen:
                break
        seen.add(rows)
        H[list(rows), v] = 1
    return H


def _stacked(n, m, r, tail, basis_last, seed, begin, trials):
    """H = _sparse_H; G = a basis B of ker H and r - |B| sparse random sums (about 3 terms) of the basis rows but the
    last ``tail`` -- so each of those ``tail`` rows is independent of all other rows of G and is a pivot row in every
    trial.  basis_last: the sums first, then the basis (the independent rows at the highest indices); else the basis
    first, and every row behind it reduces to zero.  L: 3 random vectors orthogonal to every row of G but those
    ``tail``, so that a reduced row is a candidate only through what it holds of them -- the result row is one of them,
    or a row one of them was XORed into.  The same seed gives the same H, B, sums and L in both orders."""
    rng = np.random.default_rng([seed, n, m])
    H = _sparse_H(rng, m, n)
    B = gf2.nullspace(H).astype(np.uint8)
    nb = B.shape[0]
    assert tail < nb <= r
    coef = rng.random((2048, nb)) < 3.0 / nb
    coef[:, nb - tail:] = False
    sums = (coef[:r - nb].astype(np.int64) @ B.astype(np.int64) % 2).astype(np.uint8)
    blind = gf2.nullspace(B[:nb - tail]).astype(np.int64)              # orthogonal to the other rows (and to the sums)
    L = (rng.random((3, blind.shape[0])) < 0.5).astype(np.int64) @ blind % 2
    return Case(H, np.vstack([sums, B] if basis_last else [B, sums]), L, seed=seed, begin=begin, trials=trials)


def _tie_decides(tie, r, k, seed):
    """G [r][n] of full row rank, H = two_column_H, such that in trial tie["trial"] the sweep ends on whichever of
    the tied columns a, b comes first, and the output depends on which:
      rows 0 .. r-2   one 1 each on distinct columns among the first q of that trial's order (rank r - 1 there),
      row r-1         1 in a and in b, none among the first q,
      row 0           a 1 in a as well, and nothing else: a first (the statement) XORs row r-1 into row 0; b first
                      leaves row 0 at weight 2, where L[0] detects it,
      every row but 0 at least 3 further ones on the columns behind q + 1 in that trial's order (in any other trial
                      those columns come anywhere, and the elimination is a general one).
    L: k random rows; L[0] is 1 on row 0's pivot column and 0 on a."""
    n, t, q, a, b = tie["n"], tie["trial"], tie["q"], tie["a"], tie["b"]
    order = do.column_order(tie["seed"], t, n)
    assert order[q] == a and order[q + 1] == b and a < b
    rng = np.random.default_rng([seed, n, r])
    early = order[:q][order[:q] >= 2]
    late = order[q + 2:][order[q + 2:] >= 2]
    piv = rng.choice(early, r - 1, replace=False)
    G = np.zeros((r, n), np.uint8)
    G[np.arange(r - 1), piv] = 1
    G[r - 1, [a, b]] = 1
    G[0, a] = 1
    for i in range(1, r):
        G[i, rng.choice(late, 3 + int(rng.integers(0, 6)), replace=False)] = 1
    L = (rng.random((k, n)) < 0.3).astype(np.uint8)
    L[0, piv[0]], L[0, a] = 1, 0
    return Case(two_column_H(n), G, L, seed=tie["seed"], begin=t if n > 512 else t - 2, trials=4)


def _make(name):
    if name in ("r2048_low", "r2048_high"):              # W = 18, NP = 1024: 157 696 B, the most rows at their widest n
        return _stacked(576, 36, 2048, 96, name == "r2048_high", 1, 3, 4)      # (trial 3: the result in row 2029)
    if name in ("r1985", "r1984", "r129", "r128"):       # a lane gains its 32nd / its 3rd row; the basis last
        r = int(name[1:])
        # (trial 50: the result in the last row of r1985 and of r129)
        return _stacked(200, 100, r, 8, True, 20261021, *((50, 4) if r > 1000 else (40, 16)))
    if name == "tall":                                   # r > n, rank 60: the sweep ends on the columns, left = 240
        rng = np.random.default_rng(300)
        basis = rng.random((60, 96)) < 0.3
        basis[:, :2] = False
        G = (rng.random((300, 60)) < 0.2).astype(np.int64) @ basis.astype(np.int64) % 2
        G[-60:] = basis                                  # (the rank is that of the basis)
        return Case(two_column_H(96), G, rng.random((3, 96)) < 0.3, seed=2, trials=16)
    if name in ("288x", "288z"):
        c = codes.load_code("[[288, 12, 18]]")
        H, L = (c.Hx, c.Lx) if name == "288x" else (c.Hz, c.Lz)
        return Case(H, gf2.nullspace(H), L, trials=16)
    if name == "wide8192":                               # W = 256: a real elimination over 256 words
        rng = np.random.default_rng(8192)
        G = rng.random((120, 8192)) < 0.01
        G[:, :2] = False
        L = np.vstack([np.ones((1, 8192), bool), rng.random((2, 8192)) < 0.3])
        return Case(two_column_H(8192), G, L, seed=4, trials=4)
    if name == "at_limit":                               # max(8 * 16384, 63 * 513 * 4) + 2 * 16384 = 163 840 B
        return _tie_decides(TIE_16384, 63, 3, 16384)     # trials 20 .. 23, the tie in 20
    if name == "tie":                                    # trials 11295 .. 11298, the tie in 11297
        return _tie_decides(TIE_512, 40, 2, 512)
    if name == "n1":                                     # one empty check: ker H is everything
        return Case(np.zeros((1, 1), np.uint8), [[1]], [[1]], seed=6, trials=4)
    if name == "n2":
        return Case(two_column_H(2), [[1, 1]], [[1, 0]], seed=6, trials=4)
    if name == "n3":
        return Case(two_column_H(3), [[1, 1, 0], [0, 0, 1]], [[0, 0, 1]], seed=6, trials=4)
    if name == "dem72":                                  # the phenomenological model of [[72,12,6]] over 3 rounds
        from qldpc_amd import dem
        H, L, _ = dem.phenomenological(codes.load_code("[[72, 12, 6]]"), 3, 0.01)
        H = np.asarray(H.toarray() if hasattr(H, "toarray") else H)
        return Case(H, gf2.nullspace(H.astype(np.int64)), L, trials=8)
    if name == "r129_passes":                            # more trials than workgroups at one or two per CU
        c = case("r129")
        return Case(c.H, c.G, c.L, seed=c.seed, begin=0, trials=600)
    if name == "wide8192_queue":                         # more trials than CUs at a state only one of which fits a CU
        c = case("wide8192")
        return Case(c.H, c.G, c.L, seed=c.seed, begin=0, trials=300)
    raise KeyError(name)


ROWS = ("r2048_low", "r2048_high", "r1985", "r1984", "r129", "r128")
TINY = ("n1", "n2", "n3")
PARITY = ROWS + ("tall", "288x", "288z", "wide8192", "at_limit", "tie") + TINY + ("dem72",)
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
