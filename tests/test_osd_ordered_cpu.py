"""CPU: OSD in a caller-supplied column order -- the numpy statement (tests/osd_ordered_oracle.py) against the
reference's recorded solutions on tied reliabilities (tests/golden/osd_ties.npz), against the sorted-order oracles,
and the host-side pieces (ABI surface, numpy_order, the drop-in's switch)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import osd_order_oracle as ordo
import osd_ordered_oracle as ordg
from oracle import oracle
from qldpc_amd import _lib, codes, osd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "osd_ties.npz")
CODE_OF = {"steane": "steane", "72": "[[72, 12, 6]]", "144": "[[144, 12, 12]]", "288": "[[288, 12, 18]]"}
GROUPS = ("steane", "72", "144", "288", "st144")
_CACHE = {}


def space_time(H, T):
    """spaceTime.py:4-18."""
    mm = H.shape[0]
    return np.hstack([np.kron(np.eye(T, dtype=np.int64), H),
                      (np.eye(mm * T, dtype=np.int64) + np.eye(mm * T, k=-mm, dtype=np.int64)) % 2])


def load_ties(tag):
    """H (from codes.load_code / the space-time formula) and the recorded arrays of one group."""
    if tag not in _CACHE:
        d = np.load(GOLDEN)
        H = (space_time(codes.load_code("[[144, 12, 12]]").Hx.astype(np.int64), 12) if tag == "st144"
             else codes.load_code(CODE_OF[tag]).Hx.astype(np.int64))
        g = {k: d[f"{tag}/{k}"] for k in ("syndromes", "llr", "hard", "ordering", "solution", "kind")}
        g["H"] = H
        g["ordering"] = g["ordering"].astype(np.int32)
        for a in g.values():
            a.setflags(write=False)
        _CACHE[tag] = g
    return _CACHE[tag]


def numpy_is_the_references():
    """The known-answer vectors of the fixture sort to their recorded orders on this host: then np.argsort breaks
    ties as the numpy build that made the fixture does.  (Else: the reason, for the skip message.)"""
    d = np.load(GOLDEN)
    for key in d.files:
        if key.startswith("ka/llr"):
            n = key[len("ka/llr"):]
            if not np.array_equal(np.argsort(np.abs(d[key])), d[f"ka/order{n}"].astype(np.int64)):
                return False, (f"np.argsort of this numpy build ({np.__version__}) orders the equal values of the "
                               f"known-answer vector of length {n} differently from the fixture's")
    return True, ""


_COLUMN_RULE = {}


def column_rule_solutions(tag):
    """oracle.osd0 (ties by column index) on every record of kinds 1 and 2: (record indices, solutions)."""
    if tag not in _COLUMN_RULE:
        g = load_ties(tag)
        pick = np.flatnonzero((g["kind"] == 1) | (g["kind"] == 2))
        _COLUMN_RULE[tag] = (pick, np.stack([oracle.osd0(g["H"], g["syndromes"][i], g["llr"][i], g["hard"][i])
                                             for i in pick]))
    return _COLUMN_RULE[tag]


@pytest.mark.parametrize("tag", GROUPS)
def test_fixture_shape_and_orders_are_the_references_argsort(tag):
    g = load_ties(tag)
    m, n = g["H"].shape
    B = len(g["kind"])
    assert g["syndromes"].shape == (B, m) and g["llr"].shape == g["hard"].shape == g["solution"].shape == (B, n)
    assert np.array_equal(np.sort(g["ordering"], axis=1), np.tile(np.arange(n), (B, 1)))
    # every recorded order sorts |llr| ascending, NaN last: it differs from any other argsort only inside ties
    for l, o in zip(g["llr"], g["ordering"]):
        a = np.abs(l)[o]
        k = ordo.order_key(a)
        assert (np.diff(k.astype(np.int64)) >= 0).all()
    want = {"steane": {0: 24, 1: 24, 2: 24, 3: 24, 4: 24, 5: 6}, "st144": {1: 8}}.get(
        tag, {0: 24, 1: 24, 2: 24, 3: 24, 4: 24, 5: 6, 6: 8})
    assert {int(k): int((g["kind"] == k).sum()) for k in np.unique(g["kind"])} == want
    # kind 6: outside the column space -- the recorded solution misses the syndrome; every other one meets it
    meets = ((g["solution"].astype(np.int64) @ g["H"].T) % 2 == g["syndromes"]).all(1)
    assert np.array_equal(meets, g["kind"] != 6)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "wide.npz")) // 2


@pytest.mark.parametrize("tag", GROUPS)
def test_oracle_in_the_recorded_order_is_the_reference(tag):
    g = load_ties(tag)
    for i in range(len(g["kind"])):
        got = ordg.osd0(g["H"], g["syndromes"][i], g["llr"][i], g["hard"][i], g["ordering"][i])
        assert np.array_equal(got, g["solution"][i]), (tag, i, int(g["kind"][i]))


@pytest.mark.parametrize("tag", ("steane", "72", "144", "288"))
def test_oracle_in_sorted_order_is_the_sorted_oracles(tag):
    g = load_ties(tag)
    H = g["H"]
    for i in range(0, len(g["kind"]), 3):
        s, l, h = g["syndromes"][i], g["llr"][i], g["hard"][i]
        so = ordg.sort_order(l)
        assert np.array_equal(ordg.osd0(H, s, l, h, so), oracle.osd0(H, s, l, h)), (tag, i)
        red = ordg.reduce(H, s, l, h, so)
        base = ordo.reduce(H, s, l, h)
        for method, w in (("cs", 7), ("e", 4)):
            assert np.array_equal(ordg.osd_order(H, s, l, h, so, w, method, red=red),
                                  ordo.osd_order(H, s, l, h, w, method, red=base)), (tag, i, method, w)


@pytest.mark.parametrize("tag", ("72", "144", "288", "st144"))
def test_reference_differs_from_the_column_index_rule_on_ties(tag):
    """The condition the generator asserts: without it the GPU test could pass on a build without the feature."""
    g = load_ties(tag)
    pick, sols = column_rule_solutions(tag)
    differ = int((sols != g["solution"][pick]).any(1).sum())
    print(f"{tag}: the reference differs from the column-index rule on {differ} of {len(pick)} tied records")
    assert 2 * differ >= len(pick)


def test_numpy_order_is_the_references_expression():
    rng = np.random.default_rng(1)
    l = np.round(2.0 * rng.standard_normal((5, 90)))
    got = osd.numpy_order(l)
    assert got.dtype == np.int32 and got.shape == l.shape
    for row, o in zip(l, got):
        assert np.array_equal(o, np.argsort(np.abs(row)))
    assert np.array_equal(osd.numpy_order(l[2]), got[2])
    assert osd.numpy_order(np.zeros((0, 7))).shape == (0, 7)
    ok, why = numpy_is_the_references()
    if not ok:
        print("not compared with the recorded orders:", why)
        return
    for tag in GROUPS:
        g = load_ties(tag)
        assert np.array_equal(osd.numpy_order(g["llr"]), g["ordering"]), tag


def test_column_order_argument_forms(monkeypatch):
    """osd._column_order and the keyword through performOSD / performOSD_batch, on a stub decoder."""
    calls = []

    class FakeDec:
        m, n = 3, 7

        def osd0(self, syn, llr, hard):
            calls.append(("osd0", None))
            return np.zeros_like(hard)

        def osd(self, syn, llr, hard, method="cs", order=7, column_order=None):
            calls.append((method, order, None if column_order is None else np.array(column_order)))
            return np.zeros_like(hard)

    monkeypatch.setattr(osd, "decoder_for", lambda H: FakeDec())
    monkeypatch.setattr(osd, "NUMPY_ORDER", False)
    s, h = np.zeros(3, int), np.zeros(7, int)
    l = np.array([1.0, -1.0, 2.0, 1.0, 0.5, -0.5, 2.0])
    osd.performOSD(None, s, l, h)
    assert calls[-1] == ("osd0", None)
    osd.performOSD(None, s, l, h, column_order="numpy")
    assert calls[-1][1] == 0 and np.array_equal(calls[-1][2], np.argsort(np.abs(l))[None, :])
    rev = np.arange(7)[::-1]
    osd.performOSD_enhanced(None, s, l, h, column_order=rev)
    assert np.array_equal(calls[-1][2], rev[None, :])
    osd.performOSD_order(None, s, l, h, 4, "e", column_order=rev)
    assert calls[-1][:2] == ("e", 4) and np.array_equal(calls[-1][2], rev[None, :])
    osd.performOSD_order_batch(None, s[None], l[None], h[None], 7, column_order="numpy")
    assert calls[-1][:2] == ("cs", 7) and np.array_equal(calls[-1][2], np.argsort(np.abs(l))[None, :])
    osd.performOSD_batch(None, s[None], l[None], h[None], column_order=rev[None])
    assert calls[-1][1] == 0 and np.array_equal(calls[-1][2], rev[None])
    osd.performOSD_order(None, s, l, h, 4)
    assert calls[-1][2] is None
    with pytest.raises(TypeError):
        osd.performOSD(None, s, l, h, rev)                    # keyword-only: the reference's positional signature
    for bad in ("stable", rev[:5], rev.astype(float)):
        with pytest.raises(ValueError):
            osd.performOSD(None, s, l, h, column_order=bad)
    # the environment switch makes "numpy" the default
    monkeypatch.setattr(osd, "NUMPY_ORDER", True)
    osd.performOSD(None, s, l, h)
    assert np.array_equal(calls[-1][2], np.argsort(np.abs(l))[None, :])
    osd.performOSD_order(None, s, l, h, 4)
    assert np.array_equal(calls[-1][2], np.argsort(np.abs(l))[None, :])


def test_switch_is_read_from_the_environment():
    script = "from qldpc_amd import osd; print(int(osd.NUMPY_ORDER))"
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "QBP_OSD_NUMPY_ORDER"}
        if value is not None:
            env["QBP_OSD_NUMPY_ORDER"] = value
        env["PYTHONPATH"] = ROOT
        assert subprocess.check_output([sys.executable, "-c", script], env=env, text=True).strip() == want


def test_last_batch_record_in_numpy_order(monkeypatch):
    """osd._from_last_batch under the switch: the driver's loop is still served from one launch, which then runs in
    numpy_order of every failing row; a call in an order of its own takes the one-syndrome path."""
    from qldpc_amd import bp
    m, n, B = 4, 9, 12
    calls = []

    class FakeDec:
        def __init__(self):
            self.m, self.n = m, n

        def osd0(self, syn, llr, hard):
            calls.append(("osd0", len(syn)))
            return hard.copy()

        def osd(self, syn, llr, hard, method="cs", order=7, column_order=None):
            calls.append(("osd", len(syn)))
            if len(syn) > 1:                                  # the record's launch: numpy_order of every failing row
                assert np.array_equal(column_order, np.stack([np.argsort(np.abs(r)) for r in llr]))
            return (hard ^ (np.asarray(column_order)[:, :1] == np.arange(n))).astype(np.uint8)   # depends on the order

    dec = FakeDec()
    monkeypatch.setattr(osd, "decoder_for", lambda H: dec)
    monkeypatch.setattr(osd, "NUMPY_ORDER", True)
    rng = np.random.default_rng(0)
    syn = rng.integers(0, 2, (B, m)).astype(np.int8)
    llr = np.round(rng.normal(size=(B, n)) * 2)
    hard = rng.integers(0, 2, (B, n)).astype(np.int8)
    conv = np.arange(B) % 3 == 0
    bp._set_last_batch(bp._LastBatch(dec, syn, llr, hard, conv))
    try:
        fails = np.flatnonzero(~conv)
        served = [osd.performOSD(None, syn[i], llr[i], hard[i]) for i in fails[:3]]
        assert calls == [("osd", len(fails))]
        for i, sol in zip(fails[:3], served):
            own = osd.performOSD(None, syn[i], llr[i].copy(), hard[i])       # a copy: the one-syndrome path
            assert np.array_equal(sol, own)
        assert calls[1:] == [("osd", 1)] * 3
        i = int(fails[4])
        osd.performOSD(None, syn[i], llr[i], hard[i], column_order=np.arange(n))  # an order of the caller's own
        assert calls[-1] == ("osd", 1) and len(calls) == 5
    finally:
        bp._set_last_batch(None)


def test_abi_surface_has_the_ordered_entries():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    declared = set(re.findall(r"\b(qbp_[a-z0-9_]+)\s*\(", header))
    for name in ("qbp_osd_batch_ordered", "qbp_osd_batch_ordered_device"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qbp_osd_batch_ordered"][1]) == len(_lib.SIGNATURES["qbp_osd_batch"][1]) + 1
    assert (len(_lib.SIGNATURES["qbp_osd_batch_ordered_device"][1])
            == len(_lib.SIGNATURES["qbp_osd_batch_device"][1]) + 1)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qldpc_amd", "csrc"), "libqbp.so"])
    lib = _lib.load()
    assert hasattr(lib, "qbp_osd_batch_ordered") and hasattr(lib, "qbp_osd_batch_ordered_device")
    src = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp.hip")).read()
    for name in ("qbp_osd_batch_ordered", "qbp_osd_batch_ordered_device"):
        assert re.search(rf"^int {name}\([^)]*\)\ntry \{{", src, re.M), name


def test_decoder_osd_rejects_bad_orders_before_the_library():
    class D(_lib.Decoder):
        def __init__(self):
            self.m, self.n, self._h = 3, 7, None
            import threading
            self._lock = threading.RLock()

        def __del__(self):
            pass

    d = D()
    s, l, h = np.zeros((2, 3), np.uint8), np.zeros((2, 7)), np.zeros((2, 7), np.uint8)
    for bad in (np.zeros((2, 6), int), np.zeros((2, 7)), np.full((2, 7), 2**32, np.int64),
                np.tile(np.arange(7) + 2**32, (2, 1))):           # (would wrap into a valid permutation as int32)
        with pytest.raises(ValueError):
            d.osd(s, l, h, order=0, column_order=bad)
