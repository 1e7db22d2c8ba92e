"""CPU: the variable-major layout of the on-chip kernel's check->variable messages (qbp_plan_r_layout, host only).

A slot holds one record of DV doubles per variable with a check; edge (c, j) of variable v gathers the whole record
off one address (tab_gather) and stores its own message at word lead + k of it (tab_store), k = the position of check
c in v's column in summation order; the other words of a record are zeros nobody writes, which records of short
columns may share.  Checked on every parity-check matrix under tests/golden/ and on a random irregular one:
message words disjoint, k ascending with the check, store = gather + lead + k, no foreign message inside a record,
padding edges on the zero record, no more words than one record per variable, and the LDS arithmetic
of the host (slot stride, one copy, two copies around FUSED_R2_OFF_BYTES) against a restatement of the kernel's carve."""
import glob
import os

import numpy as np
import pytest

from qldpc_amd import _lib, bp

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_LIMIT = 160 * 1024
NUM_COUNTERS = 12
E_UNSUPPORTED = -4


def _matrices():
    out = []
    for f in sorted(glob.glob(os.path.join(HERE, "golden", "*.npz"))):
        z = np.load(f, allow_pickle=True)
        if "H" in z.files and z["H"].ndim == 2:
            out.append((os.path.basename(f)[:-4], np.asarray(z["H"]).astype(np.int64) & 1))
    rng = np.random.default_rng(20)
    H = (rng.random((50, 131)) < 0.03).astype(np.int64)
    H[7] = 0                                         # a check without an edge, columns of degree 0 .. 3
    H = H[H.sum(1) <= 6]
    out.append(("random_irregular", H[:, H.sum(0) <= 3]))
    return out


MATRICES = _matrices()


def _layout(lib, H, S, col_order=0):
    rp, ci, m, n = bp.csr_from_H(H)
    info = np.zeros(8, np.int32)
    plan = np.zeros(8, np.int32)
    assert lib.qbp_plan(rp.ctypes.data, ci.ctypes.data, m, n, plan.ctypes.data, None, None, None) == 0
    if plan[0] != 1:
        assert lib.qbp_plan_r_layout(rp.ctypes.data, ci.ctypes.data, m, n, col_order, S, info.ctypes.data, None,
                                     None) == E_UNSUPPORTED
        return None
    dc, dv = int(plan[1]), int(plan[2])
    tg = np.zeros((dc, m), np.uint16)
    ts = np.zeros((dc, m), np.uint16)
    tv = np.zeros((dc, m), np.int32)
    assert lib.qbp_plan(rp.ctypes.data, ci.ctypes.data, m, n, plan.ctypes.data, tv.ctypes.data, None, None) == 0
    assert lib.qbp_plan_r_layout(rp.ctypes.data, ci.ctypes.data, m, n, col_order, S, info.ctypes.data, tg.ctypes.data,
                                 ts.ctypes.data) == 0
    return dc, dv, tv, tg.astype(np.int64), ts.astype(np.int64), info, (rp, ci, m, n)


def carve_bytes(dc, dv, m, n, S, stride, np_bytes, r2_off, two_copies):
    """The kernel's LDS carve (qbp_kernels.hpp), decode launch without the first-check-step table: function tables,
    [second-copy offset], one copy of R = S slots of `stride` doubles + zero record + dump word, priors [dc][m], three
    64-bit words per slot, 6 S + 1 + S NUM_COUNTERS 32-bit words, var_lds [dc][m], error bytes [2][S][n4]."""
    r_doubles = S * stride + dv + 1
    b = np_bytes + (r2_off if two_copies else 0) + (r_doubles + dc * m + 3 * S) * 8
    b += (6 * S + 1 + S * NUM_COUNTERS + dc * m) * 4 + 2 * S * ((n + 3) // 4) * 4
    return -(-b // 16) * 16, r_doubles


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name,H", MATRICES, ids=[x[0] for x in MATRICES])
def test_records_and_offsets(lib, name, H):
    got = _layout(lib, H, 1)
    if got is None:                                  # (not an on-chip matrix: refused, checked in _layout)
        return
    dc, dv, tv, tg, ts, info, (rp, ci, m, n) = got
    stride = int(info[1])
    deg = H.sum(0)
    assert info[0] == dv and stride <= dv * int((deg > 0).sum())
    if (deg[deg > 0] == dv).all():
        assert stride == dv * int((deg > 0).sum())                       # full columns: nothing to share
    written = np.zeros(stride + dv + 1, int)
    base = np.full(n, -1)
    for v in range(n):
        checks = np.flatnonzero(H[:, v])                                 # ascending check order
        assert len(checks) <= dv
        for k, c in enumerate(checks):
            j = int(np.searchsorted(ci[rp[c]:rp[c + 1]], v))
            assert tv[j, c] == v
            if k == 0:
                base[v], first = tg[j, c], ts[j, c]
            assert tg[j, c] == base[v], (name, v, c)                     # one gather address per variable
            assert ts[j, c] == first + k, (name, v, c, k)                # k ascends with the check
            assert base[v] <= ts[j, c] < base[v] + dv
            written[ts[j, c]] += 1
    assert (written[:stride] <= 1).all() and not written[stride:].any()  # message words disjoint, zero record clean
    for v in np.flatnonzero(deg):                                        # nobody else's message inside the record
        assert 0 <= base[v] and base[v] + dv <= stride and written[base[v]:base[v] + dv].sum() == deg[v], (name, v)
    pad = tv < 0
    assert (tg[pad] == stride).all() and (ts[pad] == stride + dv).all()  # the zero record, the dump word


@pytest.mark.parametrize("name,H", MATRICES, ids=[x[0] for x in MATRICES])
def test_lds_arithmetic(lib, name, H):
    m, n = H.shape
    for S in sorted({1, 2, max(1, 512 // m), max(1, 1024 // m)}):
        got = _layout(lib, H, S)
        if got is None:
            return
        dc, dv, tv, tg, ts, info, _ = got
        r2_off, np_bytes = int(info[5]), int(info[6])
        stride = int(info[1])
        assert np_bytes % 16 == 0 and r2_off % 16 == 0
        one, r_doubles = carve_bytes(dc, dv, m, n, S, stride, np_bytes, r2_off, False)
        two, _ = carve_bytes(dc, dv, m, n, S, stride, np_bytes, r2_off, True)
        assert info[2] == r_doubles
        assert info[3] == (one if one <= LDS_LIMIT else 0)
        # two copies: the first below the constant offset of the second, the second and the rest below the limit
        fits = dc == 6 and r_doubles * 8 <= r2_off and two <= LDS_LIMIT
        assert info[4] == (two if fits else 0), (name, S)
        # the highest word any lane addresses lies inside its copy (table entries past a slot's records are taken
        # relative to the last slot): the dump word, the copy's last, when the matrix has padding edges
        top = (S - 1) * stride + int(max(tg.max() + dv - 1, ts.max()))
        assert top == (r_doubles - 1 if (tv < 0).any() else S * stride - 1)


def test_headline_and_small_codes_keep_their_geometry(lib):
    """[[288,12,18]] keeps S = 7 with two copies (n DV = DC m); the Steane code keeps its 341 slots with two copies,
    the padded matrix of tests/test_gpu_geometry.py its 36 (shared zero words: 3 n would not fit)."""
    rng = np.random.default_rng(5)
    irr = (rng.random((40, 90)) < 0.05).astype(np.int64)
    irr[:, 0] = 0
    irr[3] = 0
    irr[3, :2] = 1
    irr = irr[(irr.sum(1) <= 6)]
    irr = irr[:, irr.sum(0) <= 3]
    for name, S in (("bp_288", 7), ("bp_72", 28), ("bp_144", 14), ("bp_steane", 341), ("irregular", 1024 // len(irr))):
        H = irr if name == "irregular" else dict(MATRICES)[name]
        info = _layout(lib, H, S)[5]
        assert info[4] > 0, (name, info.tolist())
    assert _layout(lib, dict(MATRICES)["bp_288"], 7)[5][2] == 7 * 864 + 4
    # the 864 x 2592 space-time matrix of [[144,12,12]] ((8, 4) build, column weights 3 and 2) stays on chip
    c144 = dict(MATRICES)["bp_144"]
    st = np.hstack([np.kron(np.eye(12, dtype=np.int64), c144),
                    (np.eye(864, dtype=np.int64) + np.eye(864, k=-72, dtype=np.int64)) % 2])
    info = _layout(lib, st, 1)[5]
    # 1728 columns of weight 3 take at most 3.5 words each, 864 of weight 2 at most 3; 1 KiB stays free for the
    # counter rows of a budget ladder and the iteration histogram (4 n doubles, 32-byte records, would not fit)
    assert info[0] == 4 and info[1] <= 1728 * 7 // 2 + 864 * 3 and 0 < info[3] <= LDS_LIMIT - 1024


def test_fortran_column_order_permutes_the_record(lib):
    """col_order 1 (QBP_FLAG_DENSE_F_COLSUM): word k follows the summation order of qbp_column_order."""
    H = dict(MATRICES)["bp_72"]
    rp, ci, m, n = bp.csr_from_H(H)
    cp = np.zeros(n + 1, np.int32)
    ce = np.zeros(len(ci), np.int32)
    assert lib.qbp_column_order(rp.ctypes.data, ci.ctypes.data, m, n, 1, cp.ctypes.data, ce.ctypes.data) == 0
    dc, dv, tv, tg, ts, info, _ = _layout(lib, H, 1, col_order=1)
    row_of = np.repeat(np.arange(m), np.diff(rp))
    for v in range(n):
        for k, e in enumerate(ce[cp[v]:cp[v + 1]]):
            c, j = int(row_of[e]), int(e - rp[row_of[e]])
            assert tg[j, c] == v * dv and ts[j, c] == v * dv + k        # (full columns: record v at v * dv)
