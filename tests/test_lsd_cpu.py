"""CPU: the statement of localized statistics decoding (tests/lsd_oracle.py) on hand-checked cases and its properties on
BP failures, the Python argument checks and the C ABI without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import lsd_oracle as lo
import lsd_util as lu
from qldpc_amd import _lib, codes, lsd, mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = np.zeros((4, 5), np.uint8)
for _i in range(4):
    CHAIN[_i, _i] = CHAIN[_i, _i + 1] = 1
G = (0, 1, 3)


def decode(H, s, llr, g, hard=None):
    n = H.shape[1]
    return lo.lsd_decode(H, np.array(s, np.uint8), np.array(llr, np.float64),
                         np.zeros(n, np.uint8) if hard is None else np.array(hard, np.uint8), g)


# ---- 1. hand-checked, on the statement --------------------------------------------------------------------------------------
def test_chain_all_candidates_both_pivot_orders():
    """Chain H[i] = {v_i, v_i+1}, s = (1,0,0,0), g = 0: round 1 activates v0 and v1 (the neighbours of check 0); checks 0
    and 1 form the cluster.  v0 first: pivot v0 on row 0, then v1 on row 1 (row 0 ^= row 1): e = v0.  v1 first: pivot v1
    on row 0 (row 1 ^= row 0 = {v0, v2 | 1}), then v0 on row 1 -- the lowest row that is no pivot yet -- and
    row 0 ^= row 1 = {v1, v2 | 0}: e = v0 again."""
    for llr in ([1, 2, 9, 9, 9], [2, 1, 9, 9, 9]):
        r = decode(CHAIN, [1, 0, 0, 0], llr, 0)
        assert r["solution"].tolist() == [1, 0, 0, 0, 0]
        assert r["stats"].tolist() == [1, 2, 1, 1]
        assert r["active"].tolist() == [True, True, False, False, False]


def test_chain_one_bit_per_step_both_outcomes():
    """g = 1, v1 less reliable than v0.  Round 1 activates v1 only: pivot on row 0, row 1 = {v0, v2 | 1} has no pivot and
    a syndrome bit: the cluster {0, 1} stays invalid.  Round 2 takes the lower rank of {v0, v2}.
    v0: pivot on row 1, row 0 = {v1, v2 | 0}: e = v0, stats {2, 2, 1, 1}.
    v2: pivot on row 1, row 2 ^= row 1 = {v0, v3 | 1}: cluster {0, 1, 2} invalid; round 3 takes v0 (before v3): pivot on
    row 2, rows 0 and 1 lose their syndrome bits: e = v0, stats {3, 3, 1, 1}."""
    r = decode(CHAIN, [1, 0, 0, 0], [2, 1, 9, 9, 9], 1)
    assert r["solution"].tolist() == [1, 0, 0, 0, 0] and r["stats"].tolist() == [2, 2, 1, 1]
    assert r["active"].tolist() == [True, True, False, False, False]
    r = decode(CHAIN, [1, 0, 0, 0], [3, 1, 2, 9, 9], 1)
    assert r["solution"].tolist() == [1, 0, 0, 0, 0] and r["stats"].tolist() == [3, 3, 1, 1]
    assert r["active"].tolist() == [True, True, True, False, False]
    # the hard decision is added back: with hard = v0 the residual is zero
    r = decode(CHAIN, [1, 0, 0, 0], [3, 1, 2, 9, 9], 1, hard=[1, 0, 0, 0, 0])
    assert r["solution"].tolist() == [1, 0, 0, 0, 0] and r["stats"].tolist() == [0, 0, 0, 1]


def test_two_seeds_merge():
    """s = (1,0,0,1) on the chain, g = 1, order v1 < v3 < v2 < rest.  Round 1: cluster {0} takes v1, cluster {3} takes
    v3; pivots on rows 0 and 3, rows 1 = {v0, v2 | 1} and 2 = {v2, v4 | 1} carry the bits: clusters {0, 1} and {2, 3},
    both invalid.  Round 2: both claim v2 (activated once), the clusters merge; pivot on row 1, row 2 ^= row 1 =
    {v0, v4 | 0}: valid.  e: row 0 = {v0, v1 | 1} -> v1; row 1 -> v2 = 1; row 3 = {v3, v4 | 1} -> v3."""
    r = decode(CHAIN, [1, 0, 0, 1], [9, 1, 3, 2, 9], 1)
    assert r["merged"] and r["stats"].tolist() == [2, 3, 1, 1]
    assert r["solution"].tolist() == [0, 1, 1, 1, 0]
    assert (CHAIN.astype(int) @ r["solution"] % 2).tolist() == [1, 0, 0, 1]
    # g = 0 on the same input: two clusters {0, 1} (v0, v1) and {2, 3} (v3, v4) that never touch
    r0 = decode(CHAIN, [1, 0, 0, 1], [9, 1, 3, 2, 9], 0)
    assert r0["stats"].tolist() == [1, 4, 2, 1] and not r0["merged"]
    assert (CHAIN.astype(int) @ r0["solution"] % 2).tolist() == [1, 0, 0, 1]


def test_seed_of_weight_zero_is_invalid():
    H = np.concatenate([CHAIN, np.zeros((1, 5), np.uint8)])
    for g in G:
        r = decode(H, [1, 0, 0, 0, 1], [1, 2, 9, 9, 9], g)
        assert r["stats"][3] == 0 and r["stats"][2] == 2           # the chain's cluster, and the lone check
        assert r["solution"].tolist() == [1, 0, 0, 0, 0]           # still the readout of the pivots
        r = decode(H, [0, 0, 0, 0, 1], [1, 2, 9, 9, 9], g)
        assert r["stats"].tolist() == [0, 0, 1, 0] and not r["solution"].any()


def test_order_ties_and_nan():
    assert lo.ranks([0.5, -0.5, np.nan, 0.25, np.inf, np.nan]).tolist() == [1, 2, 4, 0, 3, 5]


# ---- 2. properties on BP failures ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def failures():
    out = {}
    for name in ("72", "rand37"):
        H = lu.matrix(name)
        syn, llr, hard = lu.bp_failures(H, 0.08, 1, 300, 30)
        out[name] = (H, syn, llr, hard, {g: lo.lsd_decode_batch(H, syn, llr, hard, g) for g in G})
    return out


def test_inputs_cover_every_situation(failures):
    pooled = {}
    for _, _, _, _, res in failures.values():
        for r in res.values():
            for k, v in lo.presence(r).items():
                pooled[k] = pooled.get(k, 0) + v
    print(pooled)
    assert pooled["two_clusters"] >= 1 and pooled["merged"] >= 1 and pooled["three_rounds"] >= 1 and pooled["skipped"] >= 1


@pytest.mark.parametrize("g", G)
@pytest.mark.parametrize("name", ["72", "rand37"])
def test_properties_on_bp_failures(failures, name, g):
    H, syn, llr, hard, res = failures[name]
    r = res[g]
    n = H.shape[1]
    ok = ((r["solution"].astype(np.int64) @ H.T % 2) == syn).all(1)
    valid = r["stats"][:, 3] == 1
    assert np.all(ok[valid]) and valid.sum() >= 250
    assert not (r["e"].astype(bool) & ~r["active"]).any()
    assert np.array_equal(r["stats"][:, 1], r["active"].sum(1)) and np.all(r["stats"][:, 1] <= n)
    assert np.all(r["stats"][:, 0] <= r["stats"][:, 1])
    assert np.array_equal(r["solution"], hard ^ r["e"])


@pytest.mark.parametrize("g", G)
def test_converged_records_come_back_unchanged(g):
    H = lu.matrix("72")
    syn, llr, hard, conv = lu.bp_outputs(H, 0.05, 2, 200, 30)
    assert 20 < conv.sum() < 200
    r = lo.lsd_decode_batch(H, syn[conv], llr[conv], hard[conv], g)
    assert np.array_equal(r["solution"], hard[conv]) and np.all(r["stats"] == [0, 0, 0, 1])


@pytest.mark.parametrize("g", G)
def test_block_diagonal_is_the_concatenation(failures, g):
    H2, syn2, llr2, hard2, res = failures["72"]
    H1 = lu.STEANE
    B = 60
    rng = np.random.default_rng(5)
    syn1 = rng.integers(0, 2, (B, 3)).astype(np.uint8)
    llr1 = rng.normal(0, 3, (B, 7))
    hard1 = (llr1 < 0).astype(np.uint8)
    one = lo.lsd_decode_batch(H1, syn1, llr1, hard1, g)
    both = lo.lsd_decode_batch(lu.diag(H1, H2), np.concatenate([syn1, syn2[:B]], 1), np.concatenate([llr1, llr2[:B]], 1),
                               np.concatenate([hard1, hard2[:B]], 1), g)
    assert np.array_equal(both["solution"], np.concatenate([one["solution"], res[g]["solution"][:B]], 1))
    assert np.array_equal(both["stats"][:, 1], one["stats"][:, 1] + res[g]["stats"][:B, 1])
    assert np.array_equal(both["stats"][:, 2], one["stats"][:, 2] + res[g]["stats"][:B, 2])
    assert np.array_equal(both["stats"][:, 3], one["stats"][:, 3] & res[g]["stats"][:B, 3])
    assert one["stats"][:, 1].max() > 0


# ---- 3. the Python argument checks ----------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("the runner must not be reached")


def test_python_argument_checks():
    assert lsd.check_bits_per_step(0) == 0 and lsd.check_bits_per_step(np.int64(3)) == 3
    for bad in (-1, 1.5, True, None, "1", 1 << 31):
        with pytest.raises(ValueError):
            lsd.check_bits_per_step(bad)
    H = lu.STEANE
    z = np.zeros
    for args in ((H, z((2, 4)), z((2, 7)), z((2, 7))), (H, z((2, 3)), z((2, 6)), z((2, 7))),
                 (H, z((2, 3)), z((2, 7)), z((3, 7))), (H, z(3), z((1, 7)), z((1, 7))), (H[0], z((2, 3)), z((2, 7)), z((2, 7)))):
        with pytest.raises(ValueError):
            lsd.performLSDBatch(*args)
    with pytest.raises(ValueError):
        lsd.performLSDBatch(H, z((2, 3)), z((2, 7)), z((2, 7)), bits_per_step=-1)
    with pytest.raises(ValueError):
        lsd.performLSD(H, z((1, 3)), z(7), z(7))


def test_lsd_excludes_the_other_second_stages_before_any_device_work():
    assert _lib.FLAG_LSD == 4096
    assert mc.lsd_run_flags(0, None) == 0 and mc.lsd_run_flags(_lib.FLAG_LAYERED, 0) == _lib.FLAG_LAYERED | _lib.FLAG_LSD
    rel = dict(legs=2, iters=3, gamma0=0.1, interval=(0, 1))
    gd = dict(iters_per_round=8, max_rounds=6)
    code = codes.load_code("[[72, 12, 6]]")
    for extra in (dict(osd=True), dict(osd=True, osd_order=3), dict(relay=rel), dict(gd=gd)):
        with pytest.raises(ValueError):
            mc.run_sweep("[[72, 12, 6]]", [0.05], 100, lsd=1, runner=_never, **extra)
        with pytest.raises(ValueError):
            mc.run_dem(code.Hx, code.Lx, np.full(72, 0.05), 100, lsd=1, runner=_never, **extra)
        with pytest.raises(ValueError):
            mc.run_weights("[[72, 12, 6]]", [3], 100, prior_p=0.01, lsd=1, runner=_never, **extra)
    with pytest.raises(ValueError):
        mc.run_sweep("[[72, 12, 6]]", [0.05], 100, lsd=-1, runner=_never)
    with pytest.raises(ValueError):
        mc.run_dem(code.Hx, code.Lx, np.full(72, 0.05), 100, lsd=1, runner=_never, window=(2, 1),
                   check_round=np.zeros(36, np.int32))
    got = mc.run_sweep("[[72, 12, 6]]", [0.05], 100, lsd=1, runner=lambda code, p, a, b: np.arange(12))
    assert np.array_equal(got[0], np.arange(12))


@pytest.mark.parametrize("argv", [["--lsd", "1", "--osd"], ["--lsd", "1", "--relay", "5", "12"], ["--lsd", "1", "--gd", "8", "6"],
                                  ["--lsd", "1", "--budgets", "10", "20"], ["--lsd", "1", "--spectrum", "x.npz"],
                                  ["--lsd", "1", "--shots", "x.npz"], ["--lsd", "-1"]])
def test_cli_refuses_bad_lsd_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05"] + argv)
    assert e.value.code == 2
    assert "--lsd" in capsys.readouterr().err


def test_paper_results_cli_refuses_lsd_with_osd(capsys):
    from qldpc_amd import paper_results
    for argv in (["--lsd", "1", "--osd", "0"], ["--lsd", "1", "--osd-order", "3"], ["--lsd", "-2"]):
        with pytest.raises(SystemExit) as e:
            paper_results.main(argv)
        assert e.value.code == 2


# ---- 4. the C ABI without a device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    return _lib.load()


def test_null_handle_is_invalid(lib):
    syn = np.zeros((2, 3), np.uint8)
    llr = np.zeros((2, 7))
    hard = np.zeros((2, 7), np.uint8)
    sol = np.full((2, 7), 7, np.uint8)
    assert lib.qbp_lsd_configure(None, 1) == -1
    assert b"null handle" in lib.qbp_last_error()
    args = (None, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data, 2, sol.ctypes.data, None)
    assert lib.qbp_lsd_batch(*args) == -1
    assert lib.qbp_lsd_batch_device(*args, None) == -1
    assert np.all(sol == 7)


def test_header_binding_and_library_agree(lib):
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for name, nargs in (("qbp_lsd_configure", 2), ("qbp_lsd_batch", 7), ("qbp_lsd_batch_device", 8)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is not None
        assert hasattr(lib, name), name
    m = re.search(r"\bQBP_FLAG_LSD\s*=\s*(\d+)u", header)
    assert m and int(m.group(1)) == _lib.FLAG_LSD == 4096
    src = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp.hip")).read()
    for name in ("qbp_lsd_configure", "qbp_lsd_batch", "qbp_lsd_batch_device"):
        assert re.search(rf"^int {name}\([^)]*\)\ntry \{{", src, re.M), name      # (no exception crosses the ABI)
    # one second stage per call, and no such stage in the other entries: the codes of check_lsd_flags
    body = src[src.index("static int check_lsd_flags"):]
    body = body[:body.index("\n}\n")]
    assert "QBP_FLAG_OSD0 | OSD_ALL_BITS | QBP_FLAG_RELAY | QBP_FLAG_GD" in body
    assert body.count("QBP_E_INVALID") == 2 and body.count("QBP_E_UNSUPPORTED") == 1
    assert re.search(r"SECOND_BP_BITS = [^;]*QBP_FLAG_LSD", src)
