"""CPU: the ladder of BP iteration budgets (qbp_mc_run_budgets, mc.run_budgets) -- argument checks without a device,
the prefix rule and the b_j - 1 iteration count in numpy against the oracle, and sharding over two gloo ranks."""
import os
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from budget_oracle import ladder_counters
from oracle import oracle
from qldpc_amd import _lib, codes, dem, mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_BUDGETS = ([], [0, 5], [10, 10], [20, 10], list(range(1, _lib.MC_MAX_BUDGETS + 2)))


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    return _lib.load()


def test_null_handle_is_invalid(lib):
    budgets = np.array([10, 20], np.int32)
    probs = np.full(4, 0.1)
    counters = np.zeros((2, 12), np.int64)
    prior = np.zeros(4)
    # (h, Lx, k, distance, probs, draws, seed, trial_begin, trial_end, prior, budgets, n_budgets, variant, alpha,
    #  damping, clip_llr, flags, counters[, stream])
    args = (None, None, 0, 0, probs.ctypes.data, 1, 0, 0, 100, prior.ctypes.data, budgets.ctypes.data, 2, 0, 1.0, 1.0,
            20.0, 0, counters.ctypes.data)
    assert lib.qbp_mc_run_budgets(*args) == -1
    assert b"null handle" in lib.qbp_last_error()
    assert lib.qbp_mc_run_budgets_device(*args, None) == -1
    assert not counters.any()
    assert _lib.MC_MAX_BUDGETS >= 16


def _never(*a):
    raise AssertionError("the runner must not be reached")


@pytest.mark.parametrize("bad", BAD_BUDGETS, ids=["empty", "zero", "repeat", "descending", "too_many"])
def test_bad_budgets_raise_before_any_device_work(bad):
    # (no runner: the default path would need a GPU, and must not get that far either)
    for runner in (_never, None):
        with pytest.raises(ValueError):
            mc.run_budgets("[[72, 12, 6]]", 0.05, 100, bad, runner=runner)
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.01)
    for runner in (_never, None):
        with pytest.raises(ValueError):
            mc.run_dem_budgets(H, L, probs, 100, bad, runner=runner)
    with pytest.raises(ValueError):
        _lib.check_budgets(bad)


def test_osd_order_without_osd_raises():
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.01)
    for runner in (_never, None):
        with pytest.raises(ValueError):
            mc.run_budgets("[[72, 12, 6]]", 0.05, 100, [10, 20], osd_order=3, runner=runner)
        with pytest.raises(ValueError):
            mc.run_dem_budgets(H, L, probs, 100, [10, 20], osd_order=3, runner=runner)
    with pytest.raises(ValueError):
        mc.run_budgets("[[72, 12, 6]]", 0.05, 100, [10.5, 20], runner=_never)
    assert _lib.check_budgets((1, 2, 50)).dtype == np.int32


@pytest.mark.parametrize("osd", [False, True])
def test_prefix_rule_equals_one_oracle_run_per_budget(osd):
    code = codes.load_code("[[72, 12, 6]]")
    p, T, budgets = 0.06, 2000, (1, 2, 3, 10, 11, 50)
    prior = mc.prior_of(p, code.n)
    got = ladder_counters(code.Hx, code.Lx, code.distance, p, prior, 0, T, budgets, osd=osd)
    want = np.stack([oracle.mc_counters(code.Hx, code.Lx, code.distance, p, prior, 0, T, max_iter=b, osd=osd)
                     for b in budgets])
    print(got[:, [0, 1, 5, 6, 7]])
    assert np.array_equal(got, want)
    assert (got[:, 0] == T).all()
    assert (np.diff(got[:, 6]) <= 0).all() and got[0, 6] > got[-1, 6]


PS, TRIALS, BUDGETS = 0.06, 301, (2, 5, 30)


def _oracle_runner(code, p, budgets, begin, end):
    return ladder_counters(code.Hx, code.Lx, code.distance, p, mc.prior_of(p, code.n), begin, end, budgets,
                           draws=2, seed=11, osd=True)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def all_reduce(table):
        t = torch.from_numpy(table.copy())
        dist.all_reduce(t)
        return t.numpy()

    table = mc.run_budgets("[[72, 12, 6]]", PS, TRIALS, BUDGETS, osd=True, rank=rank, world=world,
                           runner=_oracle_runner, all_reduce=all_reduce)
    if rank == 0:
        np.save(out, table)
    dist.destroy_process_group()


def test_two_ranks_equal_one_rank(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "table.npy")
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    two = np.load(out)
    one = mc.run_budgets("[[72, 12, 6]]", PS, TRIALS, BUDGETS, osd=True, runner=_oracle_runner)
    assert one.shape == (3, 12) and np.array_equal(one, two)
    assert (one[:, 0] == TRIALS).all() and one[0, 6] > one[-1, 6]


def test_bp_per_iteration_dictionary(monkeypatch):
    """The reference script's result dictionary (BP_per_Iteration.py:85-88), from an injected runner."""
    res = mc.bp_per_iteration(["[[72, 12, 6]]"], PS, BUDGETS, TRIALS, runner=_oracle_runner)
    table = mc.run_budgets("[[72, 12, 6]]", PS, TRIALS, BUDGETS, osd=True, runner=_oracle_runner)
    r = res["[[72, 12, 6]]"]
    assert set(r) == {"logicalErrors", "degeneracies", "OSD_invocations", "iterations"}
    assert r["iterations"] == list(BUDGETS)
    assert np.allclose(r["logicalErrors"], table[:, 1] / TRIALS)
    assert np.allclose(r["degeneracies"], table[:, 5] / TRIALS)
    assert np.allclose(r["OSD_invocations"], table[:, 6] / TRIALS)
