"""No GPU: the host surface of the large build of localized statistics decoding (QBP_OPT_LSD_MEM, ``large=``,
``lsd_large=``, ``--lsd-large``), the launch arithmetic of lsd_large_kernel restated in Python (lsd_large_layout of
qbp_lsd_large.hpp, the grid of lsd_launch in qbp.hip; tests/test_gpu_lsd_large.py compares the library's report with
it), and the invariant the kernel rests on, shown on the numpy statement (tests/lsd_oracle.py) itself."""
import os
import re
import sys

import numpy as np
import pytest

import lsd_oracle as lo
import lsd_util as lu
from qldpc_amd import _lib, codes, mc, paper_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM_LDS, MEM_LARGE, MEM_AUTO = 0, 1, 2
LDS_LIMIT = 160 * 1024
THREADS = 256


# ---- the launch arithmetic of lsd_large_kernel ---------------------------------------------------------------------------
def np_of(n):
    NP = 1
    while NP < n:
        NP <<= 1
    return NP


def lsd_large_layout(m, n):
    """lsd_large_layout of qbp_lsd_large.hpp -> (keys_in_lds, region0, bytes): a head of 64 bytes; region 0, the sort
    keys u64[NP] over the per-check tables int pivcol / label / alist and u32 pick / prev [m] while the whole fits
    160 KiB, else the tables alone; u16 idx[NP] and rank[n], u8 sol / act [n], u8 bad[m]; rounded up to 16."""
    NP = np_of(n)
    tables, keys = 20 * m, 8 * NP
    rest = 64 + 2 * NP + 4 * n + m
    up = lambda x, a: -(-x // a) * a
    region0 = up(max(keys, tables), 8)
    keys_in_lds = up(region0 + rest, 16) <= LDS_LIMIT
    if not keys_in_lds:
        region0 = up(tables, 8)
    return keys_in_lds, region0, up(region0 + rest, 16)


def lsd_large_lds_bytes(m, n):
    return lsd_large_layout(m, n)[2]


def lsd_large_grid(m, n, B, num_cu, blocks_per_cu=0):
    """The grid of lsd_launch's large branch: four wavefronts per workgroup; workgroups per CU: the least of two (the
    workspace), what the LDS holds, and QBP_OPT_BLOCKS_PER_CU where it is set."""
    per_cu = max(1, min(2, LDS_LIMIT // lsd_large_lds_bytes(m, n)))
    if blocks_per_cu > 0:
        per_cu = min(per_cu, blocks_per_cu)
    return max(1, min(B, num_cu * per_cu))


def lds_kernel_refuses(m, n):
    return lu.lsd_lds_bytes(m, n) > LDS_LIMIT or m > lu.MAX_ROWS or n > lu.MAX_COLS


def test_lds_formula_of_the_matrices_the_build_is_for():
    # 20 m of tables, m of `bad`, 2 NP + 4 n per variable, the head: about 85 KB and 60 KB before the sort keys
    assert 21 * 2592 + 4 * 7776 == 85536 and 21 * 1008 + 4 * 8991 == 57132
    # 2592 x 7776: NP = 8192, the keys (64 KiB) overlay the tables and everything fits
    assert lsd_large_layout(2592, 7776) == (True, 65536, 64 + 65536 + 16384 + 31104 + 2592) == (True, 65536, 115680)
    # 1008 x 8991: NP = 16384, the keys (128 KiB) go to the workspace
    assert lsd_large_layout(1008, 8991) == (False, 20160, 89968)
    assert lsd_large_layout(864, 2592)[0] and lsd_large_lds_bytes(864, 2592) == 64 + 32768 + 8192 + 10368 + 864
    for m, n in ((2592, 7776), (1008, 8991), (864, 2592), (612, 1836), (2049, 384)):
        assert lsd_large_lds_bytes(m, n) <= LDS_LIMIT and lds_kernel_refuses(m, n), (m, n)
    assert not lds_kernel_refuses(576, 1728)
    # the small cases: the tables win over the keys on a tall matrix
    assert lsd_large_layout(3, 7) == (True, 64, 64 + 64 + 16 + 28 + 3 + 1)
    assert lsd_large_layout(2049, 384)[:2] == (True, 40984)
    # the limits: columns by bytes long before 65535, rows by bytes alone
    assert lsd_large_lds_bytes(1, 65535) > LDS_LIMIT and lsd_large_lds_bytes(1, 65536) > LDS_LIMIT
    assert lsd_large_lds_bytes(1, 40000) > LDS_LIMIT >= lsd_large_lds_bytes(1, 16384)
    assert lsd_large_lds_bytes(7000, 64) <= LDS_LIMIT < lsd_large_lds_bytes(8000, 64)
    # the grid: two workgroups per CU at most, one where the LDS holds one
    assert lsd_large_grid(36, 72, 1 << 30, 256) == 512 and lsd_large_grid(36, 72, 1 << 30, 256, 1) == 256
    assert lsd_large_grid(36, 72, 1 << 30, 256, 32) == 512 and lsd_large_grid(36, 72, 5, 256) == 5
    assert lsd_large_grid(2592, 7776, 1 << 30, 256) == 256 and lsd_large_grid(1008, 8991, 1 << 30, 256) == 256
    assert lsd_large_grid(2592, 7776, 1 << 30, 256, 2) == 256                      # (the option does not pass the LDS)
    # the rows of the workspace at that grid, 32-bit words: about 650 MB on 2592 x 7776
    assert 256 * 2592 * (7776 // 32 + 1) * 4 == 647_626_752


def test_formula_is_the_headers():
    text = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp_lsd_large.hpp")).read()
    assert "constexpr int LSD_LARGE_THREADS = 256;" in text and "constexpr size_t LSD_LARGE_HEAD = 64;" in text
    assert "(size_t)m * 20" in text and "LSD_LARGE_HEAD + (size_t)NP * 2 + (size_t)n * 4 + (size_t)m" in text


# ---- the host surface -----------------------------------------------------------------------------------------------------
def test_option_constant_and_spellings():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    assert int(re.search(r"QBP_OPT_LSD_MEM = (\d+)", header).group(1)) == _lib.OPT_LSD_MEM == 19
    taken = [int(x) for x in re.findall(r"QBP_OPT_\w+ = (\d+)", header)]
    assert taken.count(19) == 1 and max(x for x in taken if x < 99) == 19          # the next free number
    assert _lib.MSG_MEM["lsd"][:2] == (_lib.OPT_LSD_MEM, {False: MEM_LDS, True: MEM_AUTO, "force": MEM_LARGE})
    assert _lib.MSG_MEM["lsd"][1] == _lib.MSG_MEM["relay"][1]                      # spelled as Relay-BP spells them
    for large, value in ((False, 0), (True, 2), ("force", 1)):
        assert _lib.msg_mem_value("lsd", large) == value
    for bad in (None, 1, 0, 2, "auto", "large", "True"):
        with pytest.raises(ValueError):
            _lib.msg_mem_value("lsd", bad)


def _never(*a, **k):
    raise AssertionError("the runner must not be reached")


def test_lsd_large_reaches_the_run_functions():
    code = codes.load_code("[[72, 12, 6]]")
    assert mc.lsd_run_flags(0, 1, True) == mc.lsd_run_flags(0, 1, "force") == mc.lsd_run_flags(0, 1) == _lib.FLAG_LSD
    got = mc.run_dem(code.Hx, code.Lx, np.full(72, 0.05), 100, lsd=1, lsd_large=True,
                     runner=lambda H, L, probs, prior, a, b: np.arange(12))
    assert np.array_equal(got, np.arange(12))
    got = mc.run_sweep("[[72, 12, 6]]", [0.05], 100, lsd=1, lsd_large="force", runner=lambda code, p, a, b: np.arange(12))
    assert np.array_equal(got[0], np.arange(12))
    got = mc.run_weights("[[72, 12, 6]]", [3], 100, prior_p=0.01, lsd=0, lsd_large=True,
                         runner=lambda code, w, a, b: np.arange(12))
    assert np.array_equal(got[0], np.arange(12))
    got = mc.run_weights_matrix(code.Hx, code.Lx, [3], 100, prior=mc.prior_of(0.01, 72), lsd=1, lsd_large=True,
                                runner=lambda H, L, w, prior, a, b: np.arange(12))
    assert np.array_equal(got[0], np.arange(12))
    # a spelling the table does not hold, and lsd_large without lsd: ValueError before the runner
    for kw in (dict(lsd=1, lsd_large="auto"), dict(lsd=1, lsd_large=1), dict(lsd=None, lsd_large=True)):
        with pytest.raises(ValueError):
            mc.run_dem(code.Hx, code.Lx, np.full(72, 0.05), 100, runner=_never, **kw)
        with pytest.raises(ValueError):
            mc.run_sweep("[[72, 12, 6]]", [0.05], 100, runner=_never, **kw)
        with pytest.raises(ValueError):
            mc.run_weights("[[72, 12, 6]]", [3], 100, prior_p=0.01, runner=_never, **kw)
        with pytest.raises(ValueError):
            mc.run_weights_matrix(code.Hx, code.Lx, [3], 100, prior=mc.prior_of(0.01, 72), runner=_never, **kw)
    with pytest.raises(ValueError):
        mc.run_weights_matrix(code.Hx, code.Lx, [3], 100, prior=mc.prior_of(0.01, 72), lsd=1, osd=True, runner=_never)


def test_cli_lsd_large_needs_lsd(capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05", "--lsd-large"])
    assert e.value.code == 2 and "--lsd-large needs --lsd" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        paper_results.main(["--lsd-large"])
    assert e.value.code == 2 and "--lsd-large needs --lsd" in capsys.readouterr().err


# ---- the invariant, on the statement ----------------------------------------------------------------------------------------
class Tracked(np.ndarray):
    """The statement's matrix A = [H | r] with every access noted: (row, whether it wrote, whether the check was active
    at that moment, what an element read returned).  The active checks of the moment -- the seeds and every check next
    to an active variable, rule 4 -- are read from the frame of lsd_decode that holds `active`."""
    log = None

    def _note(self, key, wrote, value=None):
        if self.ndim != 2 or Tracked.log is None:
            return
        f = sys._getframe(2)
        while f.f_code.co_name != "lsd_decode":
            f = f.f_back
        loc = f.f_locals
        count = int(loc["active"].sum())
        cache = Tracked.log["masks"]
        if count not in cache:
            cache.clear()
            cache[count] = loc["seeds"] | loc["H"][:, loc["active"]].any(1)
        row = int(key[0] if isinstance(key, tuple) else key)
        Tracked.log["notes"].append((row, wrote, bool(cache[count][row]), value))

    def __getitem__(self, key):
        out = super().__getitem__(key)
        self._note(key, False, int(out) if np.ndim(out) == 0 else None)
        return out

    def __setitem__(self, key, value):
        self._note(key, True)
        super().__setitem__(key, value)


class _Numpy:
    """numpy, but for concatenate, which hands the statement its matrix as a Tracked array."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def concatenate(*a, **k):
        return np.concatenate(*a, **k).view(Tracked)


@pytest.mark.parametrize("g", [0, 1, 3])
@pytest.mark.parametrize("name,p", [("72", 0.08), ("rand37", 0.08), ("steane", 0.2)])
def test_the_statement_touches_the_rows_of_active_checks_only(name, p, g, monkeypatch):
    """The statement scans all m rows of a column for its pivot and its XOR targets.  Instrumented: every row it
    writes, every row it reads as a whole (the two sides of an XOR) and every element read that returns a 1 belongs to a
    check that is active at that moment; the element reads on inactive checks all return 0 -- they decide nothing, and
    those rows need not exist.  At the end the rows of the never-active checks are still their rows of [H | r]."""
    H = lu.matrix(name)
    syn, llr, hard, conv = lu.bp_outputs(H, p, 3, 48, 50)
    f = np.flatnonzero(~conv)[:12]
    assert len(f) >= 6
    syn, llr, hard = syn[f].copy(), llr[f], hard[f]
    syn[0, 0] ^= 1                                           # (a syndrome that may lie outside the column space)
    want = lo.lsd_decode_batch(H, syn, llr, hard, g)
    monkeypatch.setattr(lo, "np", _Numpy())
    ones_inactive = zeros_inactive = touched = 0
    for b in range(len(syn)):
        Tracked.log = dict(notes=[], masks={})
        try:
            got = lo.lsd_decode(H, syn[b], llr[b], hard[b], g)
            notes = Tracked.log["notes"]
        finally:
            Tracked.log = None
        assert np.array_equal(got["solution"], want["solution"][b]) and np.array_equal(got["stats"], want["stats"][b])
        assert notes or got["stats"][1] == 0
        for row, wrote, active, value in notes:
            if active:
                touched += 1
            elif wrote or value is None or value != 0:
                ones_inactive += 1
            else:
                zeros_inactive += 1
    print(name, g, "accesses on active checks", touched, "zero element reads on inactive checks", zeros_inactive)
    assert ones_inactive == 0 and touched > 0
    assert zeros_inactive > 0 or name == "steane"       # (three checks: every record activates all of them)


def test_rows_of_inactive_checks_stay_original():
    """The same from the other side, without instrumenting: run the elimination of the statement on a copy of A whose
    inactive rows hold garbage until their check turns active -- rows materialised on activation -- and get the
    statement's output."""
    H = lu.matrix("72")
    syn, llr, hard, conv = lu.bp_outputs(H, 0.08, 3, 48, 50)
    f = np.flatnonzero(~conv)[:10]
    for g in (0, 1, 3):
        want = lo.lsd_decode_batch(H, syn[f], llr[f], hard[f], g)
        for i, b in enumerate(f):
            sol, stats = lazy_rows_decode(H, syn[b], llr[b], hard[b], g)
            assert np.array_equal(sol, want["solution"][i]) and np.array_equal(stats, want["stats"][i]), (g, i)


def lazy_rows_decode(H, syndrome, llr, hard, g):
    """Rules 1-8 with the rows of [H | r] written when their check turns active (garbage before), pivot search and XOR
    over the active checks alone: what lsd_large_kernel does, in numpy."""
    H = np.asarray(H, np.uint8) & 1
    m, n = H.shape
    rank = lo.ranks(llr)
    r = ((np.asarray(syndrome, np.int64) & 1) + H.astype(np.int64) @ hard) % 2
    A = np.full((m, n + 1), 0x55, np.uint8)                  # garbage: never read before it is written
    exists = np.zeros(m, bool)
    seeds = r.astype(bool)
    active = np.zeros(n, bool)
    pivcol = -np.ones(m, np.int64)

    def materialise():
        act_c = seeds | H[:, active].any(1)
        for c in np.flatnonzero(act_c & ~exists):
            A[c, :n], A[c, n], exists[c] = H[c], r[c], True
        return np.flatnonzero(act_c)

    rounds = 0
    checks = materialise()
    cl = lo.clusters_of(H, seeds, active)
    for _ in range(n):
        new = set()
        for c in cl:
            if not any(A[x, n] and pivcol[x] < 0 for x in c[0]):
                continue
            cand = sorted({int(v) for chk in c[0] for v in np.flatnonzero(H[chk]) if not active[v]}, key=lambda v: rank[v])
            new.update(cand if g == 0 else cand[:g])
        if not new:
            break
        rounds += 1
        active[list(new)] = True
        checks = materialise()
        for col in sorted(new, key=lambda v: rank[v]):
            has = [int(i) for i in checks if A[i, col]]
            free = [i for i in has if pivcol[i] < 0]
            if not free:
                continue
            for i in has:
                if i != free[0]:
                    A[i] ^= A[free[0]]
            pivcol[free[0]] = col
        cl = lo.clusters_of(H, seeds, active)
    e = np.zeros(n, np.uint8)
    for i in checks:
        if pivcol[i] >= 0:
            e[pivcol[i]] = A[i, n]
    valid = not any(A[x, n] and pivcol[x] < 0 for c in cl for x in c[0])
    return hard ^ e, np.array([rounds, int(active.sum()), len(cl), int(valid)], np.int32)
