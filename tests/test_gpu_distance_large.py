"""qbp_distance_search (dist_search_kernel, qbp_distance.hpp) against its numpy statement (tests/distance_oracle.py), bit
for bit, at the limits of the kernel: 32 rows per lane (r = 2048, pivots and the result row in bit 31 of the lanes'
masks), the row counts where a lane gains a row, a sweep that runs out of columns (r > n), 256 and 512 words per row,
a state of exactly 160 KiB and the refusals one step beyond it, equal sort keys that decide the output, n below the
smallest sort width, a detector error model; other grids and more than one pass at a large state; a small launch
between two launches at the limit.  The cases: tests/distance_large_cases.py; that each tells its defect from the
statement: tests/test_distance_large_cpu.py.  Every call writes into poisoned buffers."""
import numpy as np
import pytest

import distance_large_cases as dlc
import distance_oracle as do
from qldpc_amd import _lib, bp, distance

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
MASK_POISON = 0xDEADBEEFDEADBEEF


def fresh(H):
    """A Decoder of its own (options set on it stay on it)."""
    return _lib.Decoder(*bp.csr_from_H(np.asarray(H)))


def poisoned(n):
    return (np.full(4, -77, np.int64), np.full(n + 1, 1000, np.int64), np.full(n, SENTINEL, np.uint8),
            np.full(1, MASK_POISON, np.uint64))


def raw_call(dec, G, L, seed, begin, end, bufs):
    result, hist, codeword, mask = bufs
    return _lib.load().qbp_distance_search(dec._h, G.ctypes.data, G.shape[0], L.ctypes.data, L.shape[0], seed, begin, end,
                                           result.ctypes.data, hist.ctypes.data, codeword.ctypes.data, mask.ctypes.data)


def untouched(bufs):
    result, hist, codeword, mask = bufs
    return bool(np.all(result == -77) and np.all(hist == 1000) and np.all(codeword == SENTINEL) and mask[0] == MASK_POISON)


def run(dec, c, rows=None):
    """The case (``rows``: its first rows only) on poisoned buffers -> what Decoder.distance_search returns (hist: what
    the call added)."""
    bufs = poisoned(c.n)
    rc = raw_call(dec, c.G if rows is None else np.ascontiguousarray(c.G[:rows]), c.L, c.seed, c.begin,
                  c.begin + c.trials, bufs)
    assert rc == 0, (rc, _lib.load().qbp_last_error())
    result, hist, codeword, mask = bufs
    if result[1] < 0:
        assert np.all(codeword == SENTINEL) and mask[0] == MASK_POISON
        return result, hist - 1000, None, None
    return result, hist - 1000, codeword, int(mask[0])


def check_against_statement(want, got):
    result, hist, codeword, mask = got
    assert np.array_equal(result, want["result"]), (result, want["result"])
    assert np.array_equal(hist, want["hist"])
    if want["codeword"] is None:
        assert codeword is None and mask is None
    else:
        assert np.array_equal(codeword, want["codeword"]) and mask == want["logical_mask"]


def check_launch(dec, c, name):
    """lds_bytes against dist_lds_bytes of qbp_distance.hpp, computed here; the launch is printed (pytest -s)."""
    r, n = c.G.shape
    W, NP = (n + 31) // 32, max(4, 1 << (n - 1).bit_length())
    lds = ((max(8 * NP, 4 * r * (W + 1)) + 7) & ~7) + 2 * NP
    print(f"{name}: r={r} n={n} lds_bytes={dec.info('lds_bytes')} grid={dec.info('grid')}")
    assert dec.info("lds_bytes") == (lds + 15) & ~15 <= 160 * 1024
    assert dec.info("threads") == 64 and 1 <= dec.info("grid") <= c.trials


@pytest.mark.parametrize("name", dlc.PARITY)
def test_equals_the_statement(name):
    """n1: the constructor accepts a matrix of one empty check on one column (ker H is everything), so the case runs."""
    c = dlc.case(name)
    dec = fresh(c.H)
    got = run(dec, c)
    check_launch(dec, c, name)
    check_against_statement(dlc.statement(name), got)


def test_at_the_limit_then_a_small_launch_then_the_limit_again():
    """A handle is bound to its H, so n3 runs on a handle of its own between the two at_limit calls of one handle: the
    kernel's dynamic-LDS attribute, raised to 160 KiB by the first call, belongs to the process."""
    c, want = dlc.case("at_limit"), dlc.statement("at_limit")
    s, want_s = dlc.case("n3"), dlc.statement("n3")
    dec = fresh(c.H)
    first = run(dec, c)
    assert dec.info("lds_bytes") == 160 * 1024
    check_against_statement(want, first)
    small = fresh(s.H)
    check_against_statement(want_s, run(small, s))
    assert small.info("lds_bytes") == 48
    again = run(dec, c)
    check_against_statement(want, again)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)) and dec.info("lds_bytes") == 160 * 1024
    # one row of it: the state is the sort keys' 160 KiB whatever r <= 63
    check_against_statement(do.search(c.G[:1], c.L, c.seed, c.begin, c.begin + c.trials), run(dec, c, rows=1))
    assert dec.info("lds_bytes") == 160 * 1024


def test_one_step_beyond_160_KiB_is_refused():
    c = dlc.case("at_limit")
    dec = fresh(c.H)
    launches = (dec.info("threads"), dec.info("grid"), dec.info("lds_bytes"))
    G64 = np.ascontiguousarray(np.vstack([c.G, c.G[:1] ^ c.G[1:2]]))           # r = 64: 64 * 513 * 4 + 32768 = 164 096 B
    bufs = poisoned(c.n)
    assert raw_call(dec, G64, c.L, c.seed, c.begin, c.begin + c.trials, bufs) == _lib.E_UNSUPPORTED
    assert b"160 KiB" in _lib.load().qbp_last_error() and b"164096" in _lib.load().qbp_last_error()
    assert untouched(bufs)
    assert launches == (dec.info("threads"), dec.info("grid"), dec.info("lds_bytes"))      # no launch was recorded
    # n = 16385, r = 1: NP = 32768, the sort alone needs 320 KiB -- refused by bytes, long before 65535 columns
    n = 16385
    wide = fresh(dlc.two_column_H(n))
    G = np.zeros((1, n), np.uint8)
    G[0, 2] = 1
    bufs = poisoned(n)
    assert raw_call(wide, G, np.ones((1, n), np.uint8), 0, 0, 4, bufs) == _lib.E_UNSUPPORTED
    assert b"160 KiB" in _lib.load().qbp_last_error() and untouched(bufs)


def test_other_grids_at_the_largest_state():
    """r2048_low at QBP_OPT_BLOCKS_PER_CU 0, 1 and 3 on a fresh handle: one workgroup of 157 696 B fits a CU, and 3 asks
    for more than the LDS allows.  (The grid is the 4 trials each time -- the statement costs too much at r = 2048 for
    more; workgroups that really wait for the LDS: test_workgroups_that_wait_for_the_LDS.)"""
    c, want = dlc.case("r2048_low"), dlc.statement("r2048_low")
    dec = fresh(c.H)
    for per_cu in (0, 1, 3):
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
        check_against_statement(want, run(dec, c))
        check_launch(dec, c, f"r2048_low per_cu={per_cu}")


def test_workgroups_that_wait_for_the_LDS():
    """300 trials of wide8192 (139 744 B: one workgroup per CU): at QBP_OPT_BLOCKS_PER_CU = 3 the grid is all 300, more
    than the CUs hold at once, so the last ones start when an earlier one ends; at 1 the grid makes a second pass."""
    c, want = dlc.case("wide8192_queue"), dlc.statement("wide8192_queue")
    dec = fresh(c.H)
    for per_cu in (3, 1):
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
        check_against_statement(want, run(dec, c))
        check_launch(dec, c, f"wide8192_queue per_cu={per_cu}")
        assert dec.info("grid") == min(c.trials, per_cu * dec.info("num_cu")) and dec.info("num_cu") < c.trials


def test_more_trials_than_one_pass_of_the_grid_at_three_rows_per_lane():
    """600 trials of r129: at one and at two workgroups per CU the grid makes a second and a third pass, a slot's next
    trial sorting its keys over the last trial's rows; at three all 600 are resident or queued at once."""
    c, want = dlc.case("r129_passes"), dlc.statement("r129_passes")
    dec = fresh(c.H)
    grids = []
    for per_cu in (1, 2, 3, 0):
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
        check_against_statement(want, run(dec, c))
        check_launch(dec, c, f"r129_passes per_cu={per_cu}")
        grids.append(dec.info("grid"))
    assert grids[0] == dec.info("num_cu") < c.trials and grids[0] < grids[1] and grids[3] == c.trials


def test_a_detector_error_model_through_bound():
    c, want = dlc.case("dem72"), dlc.statement("dem72")
    out = distance.bound(c.H, c.L, trials=c.trials, seed=c.seed)
    raw = run(fresh(c.H), c)
    check_against_statement(want, raw)
    assert out["weight"] == raw[0][1] == want["result"][1] > 0 and out["trial"] == raw[0][2] and out["trials"] == c.trials
    assert np.array_equal(out["hist"], raw[1]) and np.array_equal(out["codeword"], raw[2]) and out["logical"] == raw[3]
    assert not (c.H.astype(np.int64) @ out["codeword"] % 2).any() and (c.L.astype(np.int64) @ out["codeword"] % 2).any()
