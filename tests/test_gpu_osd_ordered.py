"""GPU: OSD in a caller-supplied column order (qbp_osd_batch_ordered, the osd*_ordered_kernel builds).

With the reference's recorded `ordering` the device returns the reference's recorded solution on tied reliabilities
(tests/golden/osd_ties.npz) -- exactly, through every kernel; with the (|llr|, column) sort as the order it is the
unordered call bit for bit; with any permutation it is the numpy statement tests/osd_ordered_oracle.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import osd_order_oracle as ordo
import osd_ordered_oracle as ordg
from qldpc_amd import _lib, bp, codes, osd
from test_gpu_osd_order import _bp_failures, _fresh_decoder
from test_osd_ordered_cpu import GOLDEN, GROUPS, ROOT, load_ties, numpy_is_the_references

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _decoder(tag):
    return bp.decoder_for(load_ties(tag)["H"])


def _raw_ordered(dec, flags, syn, llr, hard, order):
    """qbp_osd_batch_ordered with raw arguments: (return code, the solution buffer, prefilled with 0xAA)."""
    syn = np.ascontiguousarray(syn, np.uint8)
    llr = np.ascontiguousarray(llr, np.float64)
    hard = np.ascontiguousarray(hard, np.uint8)
    out = np.full_like(hard, 0xAA)
    rc = _lib.load().qbp_osd_batch_ordered(dec._h, flags, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data,
                                           None if order is None else order.ctypes.data, len(syn), out.ctypes.data)
    return rc, out


# ---- 1. the recorded order gives the recorded reference solution ---------------------------------------------------

@pytest.mark.parametrize("tag", GROUPS)
def test_recorded_order_gives_the_reference_solution(tag):
    g = load_ties(tag)
    dec = _decoder(tag)
    got = dec.osd(g["syndromes"], g["llr"], g["hard"], order=0, column_order=g["ordering"])
    bad = np.flatnonzero((got != g["solution"]).any(1))
    assert len(bad) == 0, (tag, bad[:10], g["kind"][bad[:10]])
    if tag == "steane":
        return
    # not vacuous: WITHOUT the order the same tied records come out differently on at least half of them
    pick = np.flatnonzero((g["kind"] == 1) | (g["kind"] == 2))
    plain = dec.osd(g["syndromes"][pick], g["llr"][pick], g["hard"][pick], order=0)
    differ = int((plain != g["solution"][pick]).any(1).sum())
    print(f"{tag}: unordered OSD-0 differs from the reference on {differ} of {len(pick)} tied records")
    assert 2 * differ >= len(pick)


@pytest.mark.parametrize("tag", ("72", "144"))
def test_recorded_order_through_the_workgroup_kernels(tag):
    """QBP_OPT_OSD_BIG as tests/test_gpu_osd.py uses it: eight pivots at a time (1), one pivot at a time (2), eight at
    a time with a first sweep of K = 24 columns that runs out (3) -- kind 6 (outside the column space) included."""
    g = load_ties(tag)
    dec = _fresh_decoder(g["H"])
    for kind in (1, 2, 3):
        dec.set_option(_lib.OPT_OSD_BIG, kind)
        got = dec.osd(g["syndromes"], g["llr"], g["hard"], order=0, column_order=g["ordering"])
        bad = np.flatnonzero((got != g["solution"]).any(1))
        assert len(bad) == 0, (tag, kind, bad[:10], g["kind"][bad[:10]])


def test_device_entry_on_torch_buffers():
    import torch
    g = load_ties("144")
    dec = _decoder("144")
    dev = torch.device("cuda", bp.DEVICE)
    d_syn, d_llr, d_hard, d_ord = (torch.from_numpy(np.ascontiguousarray(g[k])).to(dev)
                                   for k in ("syndromes", "llr", "hard", "ordering"))
    assert d_ord.dtype == torch.int32
    d_sol = torch.empty_like(d_hard)
    stream = torch.cuda.current_stream(dev)
    dec.osd_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(g["kind"]), d_sol.data_ptr(), order=0,
                   stream=stream.cuda_stream, d_order=d_ord.data_ptr())
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_sol.cpu().numpy(), g["solution"])
    for method, w in (("cs", 7), ("e", 8)):
        dec.osd_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(g["kind"]), d_sol.data_ptr(),
                       method=method, order=w, stream=stream.cuda_stream, d_order=d_ord.data_ptr())
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_sol.cpu().numpy(),
                              dec.osd(g["syndromes"], g["llr"], g["hard"], method=method, order=w,
                                      column_order=g["ordering"]))
    lib = _lib.load()
    rc = lib.qbp_osd_batch_ordered_device(dec._h, 0, d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), None, 4,
                                          d_sol.data_ptr(), None)
    assert rc == E_INVALID and b"order" in lib.qbp_last_error()


# ---- 2. the device's own sort as the order: the unordered call bit for bit -----------------------------------------

_FAILURES = {}


def _failures(name):
    if name not in _FAILURES:
        code = codes.load_code(name)
        syn, llr, hard = _bp_failures(code, per_p=50)
        assert len(syn) >= 80, len(syn)
        so = np.stack([ordo.sort_order(l) for l in llr]).astype(np.int32)
        _FAILURES[name] = (code.Hx.astype(np.int64), syn, llr, hard, so)
    return _FAILURES[name]


@pytest.mark.parametrize("name", ("[[72, 12, 6]]", "[[288, 12, 18]]"))
def test_sorted_order_reproduces_the_unordered_call(name):
    H, syn, llr, hard, so = _failures(name)
    dec = bp.decoder_for(H)
    for method, w in (("cs", 0), ("cs", 1), ("cs", 7), ("cs", 64), ("e", 4), ("e", 12)):
        a = dec.osd(syn, llr, hard, method=method, order=w)
        b = dec.osd(syn, llr, hard, method=method, order=w, column_order=so)
        assert np.array_equal(a, b), (method, w, np.flatnonzero((a != b).any(1))[:10])
    want = dec.osd0(syn, llr, hard)
    big = _fresh_decoder(H)
    for kind in (1, 2, 3):
        big.set_option(_lib.OPT_OSD_BIG, kind)
        assert np.array_equal(big.osd(syn, llr, hard, order=0, column_order=so), want), kind


# ---- 3. arbitrary permutations against the numpy statement ---------------------------------------------------------

@pytest.mark.parametrize("name", ("[[72, 12, 6]]", "[[144, 12, 12]]"))
def test_arbitrary_permutations_equal_the_oracle(name):
    code = codes.load_code(name)
    H = code.Hx.astype(np.int64)
    syn, llr, hard = _bp_failures(code, ps=(0.07,), per_p=24, seed=7)
    assert len(syn) >= 12
    rng = np.random.default_rng(8)
    so = np.stack([ordo.sort_order(l) for l in llr])
    orders = {"reversed": so[:, ::-1], "random": np.stack([rng.permutation(code.n) for _ in llr])}
    dec = bp.decoder_for(code.Hx)
    for what, co in orders.items():
        reds = [ordg.reduce(H, s, l, h, o) for s, l, h, o in zip(syn, llr, hard, co)]
        assert np.array_equal(dec.osd(syn, llr, hard, order=0, column_order=co), np.stack([r.x0 for r in reds])), what
        for method, w in (("cs", 7), ("e", 8)):
            got = dec.osd(syn, llr, hard, method=method, order=w, column_order=co)
            want = np.stack([ordg.osd_order(H, s, l, h, o, w, method, red=r)
                             for s, l, h, o, r in zip(syn, llr, hard, co, reds)])
            assert np.array_equal(got, want), (what, method, w, np.flatnonzero((got != want).any(1))[:10])
            assert np.array_equal((got.astype(np.int64) @ H.T) % 2, syn)
            one = osd.performOSD_order(H, syn[0], llr[0], hard[0], w, method, column_order=co[0])
            assert one.dtype == np.int64 and np.array_equal(one, want[0])


# ---- 4. syndromes outside the column space, order > 0: the ordered OSD-0 output ------------------------------------

@pytest.mark.parametrize("tag", ("72", "144", "288"))
def test_inconsistent_syndromes_with_an_order_get_ordered_osd0(tag):
    g = load_ties(tag)
    f = np.flatnonzero(g["kind"] == 6)
    mix = np.concatenate([f[:4], np.flatnonzero(g["kind"] == 1)[:5], f[4:]])
    dec = _decoder(tag)
    for method, w in (("cs", 7), ("e", 8)):
        got = dec.osd(g["syndromes"][mix], g["llr"][mix], g["hard"][mix], method=method, order=w,
                      column_order=g["ordering"][mix])
        inc = g["kind"][mix] == 6
        assert np.array_equal(got[inc], g["solution"][mix][inc]), (method, w)
        want = ordg.osd_order_batch(g["H"], g["syndromes"][mix][~inc], g["llr"][mix][~inc], g["hard"][mix][~inc],
                                    g["ordering"][mix][~inc], w, method)
        assert np.array_equal(got[~inc], want), (method, w)


# ---- 5. the host entry refuses what is not a permutation, before any GPU work --------------------------------------

def test_host_entry_rejects_bad_orders():
    g = load_ties("72")
    dec = _decoder("72")
    n = g["H"].shape[1]
    args = (g["syndromes"][:3], g["llr"][:3], g["hard"][:3])
    good = np.ascontiguousarray(g["ordering"][:3], np.int32)
    lib = _lib.load()
    rc, out = _raw_ordered(dec, 0, *args, good)
    assert rc == 0 and np.array_equal(out, g["solution"][:3])
    cases = {"null": None}
    for what, pos, value in (("repeated", 5, int(good[1, 6])), ("n", 0, n), ("minus one", n - 1, -1)):
        bad = good.copy()
        bad[1, pos] = value
        cases[what] = bad
    for what, order in cases.items():
        for flags in (0, _lib.osd_flags("cs", 7)):
            rc, out = _raw_ordered(dec, flags, *args, order)
            assert rc == E_INVALID, (what, rc)
            assert (out == 0xAA).all(), what                      # solution untouched
            if order is not None:
                assert b"record 1" in lib.qbp_last_error(), (what, lib.qbp_last_error())
    with pytest.raises(_lib.QbpError) as e:
        dec.osd(*args, order=0, column_order=cases["repeated"])
    assert e.value.code == E_INVALID
    # order > 0 on a matrix beyond the one-wavefront kernel: QBP_E_UNSUPPORTED, as qbp_osd_batch
    s = load_ties("st144")
    big = _decoder("st144")
    for method, w in (("cs", 7), ("e", 4)):
        with pytest.raises(_lib.QbpError) as e:
            big.osd(s["syndromes"], s["llr"], s["hard"], method=method, order=w, column_order=s["ordering"])
        assert e.value.code == _lib.E_UNSUPPORTED


# ---- 6. the drop-in ---------------------------------------------------------------------------------------------

def test_dropin_with_the_recorded_order():
    for tag in ("72", "st144"):
        g = load_ties(tag)
        H = g["H"]
        for i in (0, 30, 60, 100, 130) if tag == "72" else (0, 5):
            one = osd.performOSD(H, g["syndromes"][i].astype(np.int64), g["llr"][i], g["hard"][i].astype(np.int64),
                                 column_order=g["ordering"][i])
            assert one.dtype == np.int64 and np.array_equal(one, g["solution"][i]), (tag, i)
    g = load_ties("144")
    assert np.array_equal(osd.performOSD_batch(g["H"], g["syndromes"], g["llr"], g["hard"],
                                               column_order=g["ordering"]), g["solution"])
    two = osd.performOSD_enhanced(g["H"], g["syndromes"][3], g["llr"][3], g["hard"][3], order=2,
                                  column_order=g["ordering"][3])
    assert np.array_equal(two, g["solution"][3])


def test_dropin_under_the_numpy_order_switch_is_the_reference(tmp_path):
    """QBP_OSD_NUMPY_ORDER=1 in a fresh process: `from decoding.OSD import performOSD`, with the reference's positional
    arguments alone, returns the recorded reference solutions -- where this host's numpy is the fixture's numpy."""
    ok, why = numpy_is_the_references()
    if not ok:
        print("not run:", why)
        return
    out = tmp_path / "solutions.npy"
    script = tmp_path / "run.py"
    script.write_text(
        "import sys\n"
        "import numpy as np\n"
        "from decoding.OSD import performOSD\n"
        "from decoding.OSD_enhanced import performOSD_enhanced\n"
        "from qldpc_amd import codes, osd\n"
        "assert osd.NUMPY_ORDER and performOSD.__module__ == 'qldpc_amd.osd'\n"
        "d = np.load(sys.argv[1])\n"
        "H = codes.load_code('[[72, 12, 6]]').Hx\n"
        "sols = [performOSD(H, s.astype(np.int64), l, h.astype(np.int64))\n"
        "        for s, l, h in zip(d['72/syndromes'], d['72/llr'], d['72/hard'])]\n"
        "sols[1] = performOSD_enhanced(H, d['72/syndromes'][1].astype(np.int64), d['72/llr'][1],\n"
        "                              d['72/hard'][1].astype(np.int64), order=0)\n"
        "np.save(sys.argv[2], np.array(sols))\n")
    env = dict(os.environ, QBP_OSD_NUMPY_ORDER="1",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "qldpc_amd", "dropin")]))
    subprocess.check_call([sys.executable, str(script), GOLDEN, str(out)], env=env, cwd=str(tmp_path), timeout=300)
    g = load_ties("72")
    got = np.load(out)
    bad = np.flatnonzero((got != g["solution"]).any(1))
    assert len(bad) == 0, (bad[:10], g["kind"][bad[:10]])


def test_last_batch_record_gives_the_bits_of_the_single_call(monkeypatch):
    """Under the switch the driver's loop (a batch decode, then performOSD on rows of its arrays) is served from one
    ordered launch; every answer equals the one-syndrome call on copies of the same rows.  One BP iteration from a
    uniform prior: LLRs with real ties, where the order matters."""
    monkeypatch.setattr(osd, "NUMPY_ORDER", True)
    code = codes.load_code("[[144, 12, 12]]")
    H = code.Hx
    rng = np.random.default_rng(31)
    p = 0.06
    _, syndromes = bp.generate_errors_and_syndromes_batch(H, p, 300, rng)
    detections, converged, llrs = bp.performBeliefPropagationBatch(H, syndromes, [np.log((1 - p) / p)] * code.n,
                                                                   maxIter=1)
    fails = np.flatnonzero(~converged)
    assert len(fails) > 100
    assert sum(len(np.unique(np.abs(llrs[i]))) < code.n for i in fails) > 50          # ties
    served = {}
    for i in fails:
        served[int(i)] = osd.performOSD(H, syndromes[i], llrs[i], detections[i])
        if len(served) == 1:
            lb = bp._last_batch()
            assert lb is not None and lb.orders is not None and len(lb.solutions) == len(fails)
    assert bp._last_batch() is None                            # every failing row served from the record
    differ = 0
    for i in fails[::5]:
        args = (syndromes[i].copy(), llrs[i].copy(), detections[i].copy())
        single = osd.performOSD(H, *args)
        assert np.array_equal(served[int(i)], single), i
        assert np.array_equal(single, osd.performOSD(H, *args, column_order=osd.numpy_order(args[1])))
        assert np.array_equal(single,
                              ordg.osd0(H, args[0], args[1], args[2], osd.numpy_order(args[1])).astype(np.int64))
        monkeypatch.setattr(osd, "NUMPY_ORDER", False)
        differ += not np.array_equal(single, osd.performOSD(H, *args))
        monkeypatch.setattr(osd, "NUMPY_ORDER", True)
    print(f"numpy order differs from the column-index rule on {differ} of {len(fails[::5])} one-iteration records")
