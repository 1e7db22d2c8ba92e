"""CPU: the residual-weight spectra and the iteration histogram of qbp_mc_run_spectrum, without a GPU -- the numpy
statement of the rule (tests/spectrum_oracle.py) against the fixture the reference's own rework/main.py loop made
(tests/golden/spectrum.npz), the identities between tables and counters, the Python layer on an injected runner (two
gloo ranks), and the prototypes of the three C entry points."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from qldpc_amd import _lib, codes, mc
from spectrum_oracle import check_identities, spectrum_counters, spectrum_of_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spectrum.npz")


def test_oracle_reproduces_the_reference_fixture():
    z = np.load(GOLDEN)
    assert len(z["names"]) >= 2
    seen_osd = set()
    for name in z["names"]:
        code = codes.load_code(str(z[f"{name}/code"]))
        p, max_iter, osd = float(z[f"{name}/meta"][0]), int(z[f"{name}/meta"][1]), bool(z[f"{name}/meta"][2])
        seen_osd.add(osd)
        errors = np.unpackbits(z[f"{name}/errors"], axis=1)[:, :code.n]
        assert len(errors) >= 1000 and int(z[f"{name}/replaced"]) <= 0.02 * len(errors)
        cnt, spec, hist = spectrum_of_errors(code.Hx, code.Lx, code.distance, errors, mc.prior_of(p, code.n), max_iter,
                                             osd=osd)
        assert np.array_equal(spec, z[f"{name}/weights"]), name
        its = z[f"{name}/iterations"].astype(np.int64)
        ref_hist = np.bincount(its, minlength=max_iter + 1)
        ref_hist[max_iter - 1] -= cnt[6]                      # the reference reports max_iter - 1 for unconverged trials
        ref_hist[max_iter] += cnt[6]
        assert np.array_equal(hist, ref_hist) and cnt[7] == its.sum()
        assert spec.sum(axis=1).min() > 0 or not osd          # every list is populated in the OSD case
        check_identities(cnt, spec, hist, max_iter, osd)
    assert seen_osd == {False, True}


@pytest.mark.parametrize("kw", [dict(osd=False), dict(osd=True), dict(osd=True, osd_method="cs", osd_order=3),
                                dict(osd=False, variant=2, alpha=0.8, damping=0.7)])
def test_identities_on_oracle_output(kw):
    code = codes.load_code("[[72, 12, 6]]")
    p, T, max_iter = 0.07, 600, 15
    cnt, spec, hist = spectrum_counters(code.Hx, code.Lx, code.distance, p, mc.prior_of(p, code.n), 5, 5 + T, draws=2,
                                        seed=3, max_iter=max_iter, **kw)
    check_identities(cnt, spec, hist, max_iter, kw["osd"])
    assert cnt[0] == T and cnt[6] > 0 and spec.sum() > 0
    if kw["osd"]:
        assert spec[1].sum() + spec[3].sum() > 0
    else:                                      # without OSD an unconverged trial is classified on BP's own output
        assert 0 < spec[1].sum() + spec[3].sum() <= cnt[6]
    with pytest.raises(AssertionError):                        # the identities do notice a moved count
        bad = spec.copy()
        bad[0, 1] += 1
        check_identities(cnt, bad, hist, max_iter, kw["osd"])


def test_rework_point_expansion():
    n, max_iter = 10, 6
    weights = np.zeros((4, n + 1), np.int64)
    weights[0, [2, 4]] = [3, 1]
    weights[1, 6] = 2
    weights[3, [5, 9]] = [1, 2]
    its = np.array([10, 5, 0, 0, 1, 0, 4], np.int64)          # 4 trials BP did not converge on
    cnt = np.zeros(12, np.int64)
    cnt[0], cnt[1], cnt[5], cnt[6], cnt[8] = 20, 3, 6, 4, 3
    cnt[7] = 5 * 1 + 1 * 4 + 4 * (max_iter - 1)
    pt = mc.rework_point(cnt, weights, its)
    assert pt["weights_found_BP"] == [2, 2, 2, 4] and pt["weights_found_OSD"] == [6, 6]
    assert pt["weights_found_BP_error"] == [] and pt["weights_found_OSD_error"] == [5, 9, 9]
    assert pt["logical"] == 3 / 20 and pt["osd"] == 4 / 20 and pt["degeneracies"] == 6 / 20
    assert pt["OSD_invocation_AND_logicalError"] == 3 / 20 and pt["average_iterations"] == cnt[7] / 20
    assert set(pt) == {"logical", "osd", "degeneracies", "average_iterations", "OSD_invocation_AND_logicalError",
                       *mc.REWORK_WEIGHT_LISTS}


PS = [0.07, 0.03]
TRIALS = 301          # odd on purpose: ragged shards
MAX_ITER = 12


def _oracle_runner(code, p, begin, end):
    return spectrum_counters(code.Hx, code.Lx, code.distance, p, mc.prior_of(p, code.n), begin, end, draws=1, seed=5,
                             max_iter=MAX_ITER, osd=True)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []

    def all_reduce(table):
        calls.append(table.shape)
        t = torch.from_numpy(table.copy())
        dist.all_reduce(t)
        return t.numpy()

    cnt, weights, its = mc.run_spectrum("[[72, 12, 6]]", PS, TRIALS, max_iter=MAX_ITER, osd=True, rank=rank, world=world,
                                        runner=_oracle_runner, all_reduce=all_reduce)
    assert len(calls) == 1                                     # counters and both tables in ONE reduce
    if rank == 0:
        np.savez(out, counters=cnt, weights=weights, iterations=its)
    dist.destroy_process_group()


def test_two_ranks_equal_one_rank(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "spectrum.npz")
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    two = np.load(out)
    cnt, weights, its = mc.run_spectrum("[[72, 12, 6]]", PS, TRIALS, max_iter=MAX_ITER, osd=True, runner=_oracle_runner)
    assert cnt.shape == (2, 12) and weights.shape == (2, 4, 73) and its.shape == (2, MAX_ITER + 1)
    assert np.array_equal(two["counters"], cnt) and np.array_equal(two["weights"], weights)
    assert np.array_equal(two["iterations"], its)
    assert (cnt[:, 0] == TRIALS).all() and weights.sum() > 0
    for i in range(2):
        check_identities(cnt[i], weights[i], its[i], MAX_ITER, True)
    # stabilizer_spectrum is rows 0 + 1 of the same run; rework_results expands the same tables
    spectra = mc.stabilizer_spectrum(["[[72, 12, 6]]"], p=PS[0], trials=TRIALS, max_iter=MAX_ITER, runner=_oracle_runner)
    assert np.array_equal(spectra["[[72, 12, 6]]"], weights[0, 0] + weights[0, 1]) and spectra["[[72, 12, 6]]"][0] == 0
    res = mc.rework_results([{"code": "[[72, 12, 6]]", "name": "72", "physicalErrorRates": PS}], trials=TRIALS,
                            max_iter=MAX_ITER, runner=_oracle_runner)
    for i, p in enumerate(PS):
        for r, key in enumerate(mc.REWORK_WEIGHT_LISTS):
            assert np.array_equal(np.bincount(res["72"][p][key], minlength=73), weights[i, r])
        assert res["72"][p]["average_iterations"] == cnt[i, 7] / TRIALS


def test_python_layer_refuses_bad_arguments_before_any_gpu_work():
    with pytest.raises(ValueError):
        mc.run_spectrum("[[72, 12, 6]]", [0.05], 100, max_iter=_lib.MC_SPECTRUM_MAX_ITER + 1, runner=_oracle_runner)
    with pytest.raises(ValueError):
        mc.run_spectrum("[[72, 12, 6]]", [0.05], 100, osd=False, osd_order=3, runner=_oracle_runner)
    with pytest.raises(ValueError):
        mc.run_dem_spectrum(np.eye(3, dtype=np.uint8), np.ones((1, 4), np.uint8), np.full(3, 0.1), 10)
    with pytest.raises(SystemExit):
        mc.main(["--spectrum", "x.npz", "--budgets", "3", "5", "--p", "0.05"])
    with pytest.raises(SystemExit):
        mc.main(["--spectrum", "x.npz", "--max-iter", "2000"])


def test_lib_exposes_the_three_symbols():
    want = {"qbp_mc_run_spectrum": 19, "qbp_mc_run_spectrum_device": 20, "qbp_mc_run_errors_spectrum": 16}
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for sym, nargs in want.items():
        restype, argtypes = _lib.SIGNATURES[sym]
        assert restype is C.c_int and len(argtypes) == nargs
        decl = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None and decl.group(1).count(",") + 1 == nargs, sym       # the header agrees
    assert _lib.SPECTRUM_ROWS == 4 and _lib.MC_SPECTRUM_MAX_ITER == 1024
    assert "#define QBP_SPECTRUM_ROWS 4" in header and "#define QBP_MC_SPECTRUM_MAX_ITER 1024" in header
    for method in ("mc_run_spectrum", "mc_run_spectrum_device", "mc_run_errors_spectrum"):
        assert callable(getattr(_lib.Decoder, method))
    so = os.path.join(ROOT, "qldpc_amd", "csrc", "libqbp.so")
    if os.path.exists(so):                                     # (built: the symbols are exported)
        data = open(so, "rb").read()
        for sym in want:
            assert sym.encode() in data
