"""GPU: the sliding-window decoder (qbp_window_*) against the numpy statement of its rule (tests/window_oracle.py)
composed from separate ordinary Decoders on the H_k -- qbp_decode_batch and qbp_osd_batch -- bit for bit (NaN equal to
NaN); the W >= R identity, poisoned and NULL outputs, batch splits, streams, refusals, and the Monte-Carlo entries against
oracle.classify_trials on the batch call's outputs."""
import ctypes as C

import numpy as np
import pytest

import window_oracle as wo
from oracle import oracle
from qldpc_amd import _lib, bp, dem, mc, window
from test_window_plan import MATRICES, P_OF, matrix, shifted_irregular, window_sizes

pytestmark = pytest.mark.gpu

MAX_ITER, ALPHA, DAMPING, CLIP = 8, 0.9, 0.75, 20.0
VARIANTS = {"sum_product": _lib.SUM_PRODUCT, "min_sum": _lib.MIN_SUM}
OSD = {"none": 0, "osd0": _lib.osd_flags("cs", 0), "cs3": _lib.osd_flags("cs", 3)}
B = 257


def inputs(name, batch=B, seed=5):
    H, cr = matrix(name)
    p = P_OF[name]
    errors = (np.random.default_rng(seed).random((batch, H.shape[1])) < p).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    return H, cr, errors, syn, np.full(H.shape[1], np.log((1 - p) / p))


class Parts:
    """Ordinary Decoders on the H_k, one per distinct matrix: the `decode` and `osd` of the statement."""

    def __init__(self, variant, osd, max_iter=MAX_ITER):
        self.variant, self.osd_mode, self.max_iter, self.decs = variant, osd, max_iter, {}

    def dec(self, Hk):
        key = (Hk.shape, Hk.tobytes())
        if key not in self.decs:
            self.decs[key] = _lib.Decoder(*bp.csr_from_H(Hk), bp.DEVICE)
        return self.decs[key]

    def decode(self, Hk, syn, prior):
        return self.dec(Hk).decode(syn, prior, self.max_iter, self.variant, ALPHA, DAMPING, CLIP)

    def osd(self, Hk, syn, llr, hard):
        d = self.dec(Hk)
        return d.osd0(syn, llr, hard) if self.osd_mode == "osd0" else d.osd(syn, llr, hard, "cs", 3)

    def statement(self, H, cr, W, F, syn, prior):
        return wo.decode(H, cr, W, F, syn, prior, self.decode, None if self.osd_mode == "none" else self.osd)


def same(got, want, what):
    for g, w, name in zip(got, want, ("correction", "converged", "iters", "llr", "window_fails")):
        assert np.array_equal(g, w, equal_nan=name == "llr"), (what, name)


def wdec(H, cr, W, F):
    return window.decoder_for(H, cr, W, F)


@pytest.mark.parametrize("osd", list(OSD))
@pytest.mark.parametrize("vname", list(VARIANTS))
@pytest.mark.parametrize("name", MATRICES)
def test_batch_equals_statement(name, vname, osd):
    H, cr, _, syn, prior = inputs(name)
    R = int(cr.max()) + 1
    parts = Parts(VARIANTS[vname], osd)
    classes = np.zeros(3, np.int64)
    for W, F in window_sizes(R):
        want = parts.statement(H, cr, W, F, syn, prior)
        classes += [int((want[4] == 0).sum()), int((want[4] > 0).sum()), int((~want[1]).sum())]
        d = wdec(H, cr, W, F)
        got = d.decode(syn, prior, MAX_ITER, VARIANTS[vname], ALPHA, DAMPING, CLIP, OSD[osd])
        same(got, want, (name, vname, osd, W, F, B))
        one = d.decode(syn[:1], prior, MAX_ITER, VARIANTS[vname], ALPHA, DAMPING, CLIP, OSD[osd])
        same(one, [a[:1] for a in want], (name, vname, osd, W, F, 1))
        d.close()
    print(f"{name} {vname} {osd}: all windows converged {classes[0]}, second stage {classes[1]}, missed {classes[2]}")
    assert classes[0] >= 8 and classes[1] >= 8
    if osd == "none":
        assert classes[2] >= 8


@pytest.mark.parametrize("name", MATRICES)
def test_whole_window_is_the_plain_decode(name):
    H, cr, _, syn, prior = inputs(name)
    R = int(cr.max()) + 1
    plain = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    for vname, variant in VARIANTS.items():
        hard, conv, iters, llr = plain.decode(syn, prior, MAX_ITER, variant, ALPHA, DAMPING, CLIP)
        for W, F in ((R, R), (R + 3, 1)):
            x, c, it, l, fails = wdec(H, cr, W, F).decode(syn, prior, MAX_ITER, variant, ALPHA, DAMPING, CLIP)
            assert np.array_equal(x, hard) and np.array_equal(it, iters) and np.array_equal(l, llr, equal_nan=True)
            assert np.array_equal(c, conv) and np.array_equal(fails, (~conv).astype(np.int32))


def device_call(d, syn, prior, flags, stream, outputs=(True,) * 5, poison=True):
    """The _device entry on torch buffers filled with a poison pattern, one element of slack on each side."""
    import torch
    dev = torch.device("cuda", bp.DEVICE)
    b, n = syn.shape[0], d.n
    d_syn = torch.from_numpy(syn).to(dev)
    d_prior = torch.from_numpy(prior).to(dev)
    shapes = [((b * n + 2,), torch.uint8, 0xA5), ((b + 2,), torch.uint8, 0xA5), ((b + 2,), torch.int32, -77),
              ((b * n + 2,), torch.float64, -1234.5), ((b + 2,), torch.int32, -77)]
    bufs = [torch.full(s, v, dtype=t, device=dev) for s, t, v in shapes]
    ptrs = [buf[1:].data_ptr() if on else 0 for buf, on in zip(bufs, outputs)]
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev)):
        s = torch.cuda.current_stream(dev)
        s.wait_stream(torch.cuda.default_stream(dev))
        d.decode_device(d_syn.data_ptr(), d_prior.data_ptr(), b, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags, *ptrs,
                        stream=s.cuda_stream)
        s.synchronize()
    host = [buf.cpu().numpy() for buf in bufs]
    for h, (_, _, v) in zip(host, shapes):
        assert h[0] == np.array(v).astype(h.dtype) and h[-1] == np.array(v).astype(h.dtype)     # the slack is untouched
    x, conv, iters, llr, fails = (h[1:-1] for h in host)
    return [x.reshape(b, n), conv, iters, llr.reshape(b, n), fails], host


def test_poisoned_null_split_and_streams():
    import torch
    H, cr, _, syn, prior = inputs("irregular")
    flags = OSD["osd0"]
    d = wdec(H, cr, 3, 1)
    want = d.decode(syn, prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags)
    want = [want[0], want[1].astype(np.uint8), want[2], want[3], want[4]]
    got, _ = device_call(d, syn, prior, flags, None)
    same(got, want, "device entry, current stream")
    got, _ = device_call(d, syn, prior, flags, torch.cuda.Stream(torch.device("cuda", bp.DEVICE)))
    same(got, want, "device entry, side stream")
    # NULL outputs: each alone, and none at all
    for keep in range(5):
        outputs = tuple(i == keep for i in range(5))
        got, host = device_call(d, syn, prior, flags, None, outputs)
        assert np.array_equal(got[keep], want[keep], equal_nan=True)
    device_call(d, syn, prior, flags, None, (False,) * 5)
    lib = _lib.load()
    s8, pr = np.ascontiguousarray(syn), np.ascontiguousarray(prior)
    conv = np.full(B, 9, np.uint8)
    assert lib.qbp_window_decode_batch(d._h, s8.ctypes.data, pr.ctypes.data, B, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP,
                                       flags, None, conv.ctypes.data, None, None, None) == 0
    assert np.array_equal(conv, want[1])
    # B = 100 + 157
    a = d.decode(syn[:100], prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags)
    b = d.decode(syn[100:], prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags)
    same([np.concatenate([u, v]) for u, v in zip(a, b)], [want[0], want[1].astype(bool)] + want[2:], "split")


def test_refusals_leave_outputs_untouched():
    H, cr, _, syn, prior = inputs("steane", 16)
    d = wdec(H, cr, 3, 1)
    lib = _lib.load()
    outs = [np.full((16, d.n), 0xA5, np.uint8), np.full(16, 0xA5, np.uint8), np.full(16, -77, np.int32),
            np.full((16, d.n), -1234.5), np.full(16, -77, np.int32)]
    before = [o.copy() for o in outs]

    def call(dec, s, flags, pr=prior, max_iter=MAX_ITER):
        return lib.qbp_window_decode_batch(dec._h, s.ctypes.data, pr.ctypes.data, s.shape[0], max_iter, _lib.MIN_SUM, ALPHA,
                                           DAMPING, CLIP, flags, *(o.ctypes.data for o in outs))
    for flags in (_lib.FLAG_LAYERED, _lib.FLAG_RELAY, _lib.FLAG_GD, _lib.FLAG_FAST_MATH, _lib.FLAG_PAIRWISE_COLSUM,
                  _lib.FLAG_DENSE_F_COLSUM, _lib.FLAG_OSD_LARGE, _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | (2 << 16),
                  _lib.FLAG_OSD_CS, 3 << 16, 1 << 30):
        assert call(d, syn, flags) == _lib.E_INVALID, hex(flags)
    nan_prior = prior.copy()
    nan_prior[3] = np.nan
    assert call(d, syn, 0, nan_prior) == _lib.E_INVALID
    assert call(d, syn, 0, max_iter=0) == _lib.E_INVALID
    assert all(np.array_equal(o, b) for o, b in zip(outs, before))
    assert call(d, syn, 0) == 0


@pytest.fixture(scope="module")
def big():
    """2592 x 7776, (W, F) = (6, 3): five windows of 864 x 2592, one class."""
    H, L, probs = dem.phenomenological("[[288, 12, 18]]", 18, 0.004)
    cr = window.phenomenological_rounds("[[288, 12, 18]]", 18)
    Hd = wo.dense(H)
    return Hd, L, probs, cr, wdec(Hd, cr, 6, 3)


def test_large_matrix_runs_on_chip_windows(big):
    H, L, probs, cr, d = big
    assert H.shape == (2592, 7776) and d.info("windows") == 5 and d.info("classes") == 1
    assert d.info("m", 0) == 864 and d.info("n", 0) == 2592 and d.info("kernel_kind", 0) == 1
    errors = (np.random.default_rng(3).random((64, 7776)) < 0.012).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = mc.dem_prior(np.full(7776, 0.012))
    parts = Parts(_lib.SUM_PRODUCT, "osd0")
    want = parts.statement(H, cr, 6, 3, syn, prior)
    got = d.decode(syn, prior, MAX_ITER, _lib.SUM_PRODUCT, ALPHA, DAMPING, CLIP, OSD["osd0"])
    print("large: window_fails", np.bincount(want[4]), "missed", int((~want[1]).sum()))
    same(got, want, "2592 x 7776")
    # a sub-matrix refusal: order-w OSD without QBP_FLAG_OSD_LARGE on 864 x 2592 -- nothing runs, nothing is written
    lib = _lib.load()
    outs = [np.full((64, 7776), 0xA5, np.uint8), np.full(64, 0xA5, np.uint8), np.full(64, -77, np.int32),
            np.full((64, 7776), -1234.5), np.full(64, -77, np.int32)]
    before = [o.copy() for o in outs]
    rc = lib.qbp_window_decode_batch(d._h, syn.ctypes.data, prior.ctypes.data, 64, MAX_ITER, 0, 1.0, 1.0, CLIP,
                                     OSD["cs3"], *(o.ctypes.data for o in outs))
    assert rc == _lib.E_UNSUPPORTED and all(np.array_equal(o, b) for o, b in zip(outs, before))


@pytest.mark.parametrize("osd", ["none", "osd0"])
@pytest.mark.parametrize("name", ["72", "irregular"])
def test_monte_carlo_entries(name, osd):
    H, cr, errors, syn, prior = inputs(name)
    n = H.shape[1]
    L = (np.random.default_rng(2).random((5, n)) < 0.3).astype(np.uint8)
    probs = np.linspace(0.5, 1.5, n) * P_OF[name]
    d = wdec(H, cr, 3, 1)
    plain = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    args = dict(max_iter=MAX_ITER, variant=_lib.MIN_SUM, alpha=ALPHA, damping=DAMPING, clip_llr=CLIP, flags=OSD[osd])

    def expected(errs):
        s = (errs.astype(np.int64) @ H.T % 2).astype(np.uint8)
        x, conv, iters, _, fails = d.decode(s, prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, OSD[osd])
        cnt = oracle.classify_trials(H, L, 6, errs, s, x, fails == 0, iters)
        cnt[10] = int((~conv).sum())
        return cnt
    want = expected(errors)
    assert want[6] >= 8 and want[1] >= 8
    assert np.array_equal(d.mc_run_errors(L, 6, errors, prior, **args), want)
    sampled = plain.mc_sample_errors_probs(probs, 1000, B, draws=2, seed=77)
    want = expected(sampled)
    got = d.mc_run_probs(L, 6, probs, prior, 1000, 1000 + B, draws=2, seed=77, **args)
    assert np.array_equal(got, want), (got, want)
    split = d.mc_run_probs(L, 6, probs, prior, 1000, 1101, draws=2, seed=77, **args)
    d.mc_run_probs(L, 6, probs, prior, 1101, 1000 + B, draws=2, seed=77, counters=split, **args)
    assert np.array_equal(split, want)
    d.set_option(_lib.OPT_MC_WEIGHT_CHUNK, 129)                  # two chunks
    assert np.array_equal(d.mc_run_probs(L, 6, probs, prior, 1000, 1000 + B, draws=2, seed=77, **args), want)
    assert np.array_equal(d.mc_run_errors(L, 6, sampled, prior, **args), want)


def test_run_dem_with_a_window():
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 6, 0.02)
    cr = window.phenomenological_rounds("[[72, 12, 6]]", 6)
    prior = mc.dem_prior(probs)
    d = wdec(H, cr, 4, 2)
    want = d.mc_run_probs(L, 6, probs, prior, 0, 300, seed=9, max_iter=MAX_ITER, flags=OSD["osd0"])
    got = mc.run_dem(H, L, probs, 300, distance=6, seed=9, max_iter=MAX_ITER, osd=True, window=(4, 2), check_round=cr)
    assert np.array_equal(got, want) and want[0] == 300
    with pytest.raises(ValueError):
        mc.run_dem(H, L, probs, 300, window=(4, 2))


@pytest.mark.parametrize("make", [wo.irregular, shifted_irregular])
def test_skipped_windows_and_syndrome_bytes(make):
    """W = F = 1 on a matrix with a round without checks: that window is skipped (and, with round 0 empty, still commits
    the empty column); syndrome bytes count in bit 0 only, as in the statement."""
    H, cr = make()
    n = H.shape[1]
    errors = (np.random.default_rng(8).random((B, n)) < P_OF["irregular"]).astype(np.uint8)
    syn = (errors.astype(np.int64) @ H.T % 2).astype(np.uint8)
    syn[::3] |= 2                                   # (bits above bit 0 are no syndrome)
    syn[1::5] |= 0x80
    prior = np.linspace(1.0, 4.0, n)
    for osd in ("none", "osd0"):
        parts = Parts(_lib.MIN_SUM, osd)
        for W, F in ((1, 1), (2, 1)):
            d = wdec(H, cr, W, F)
            assert d.info("windows") == int(cr.max()) + 1 - (W - 1)
            want = parts.statement(H, cr, W, F, syn, prior)
            got = d.decode(syn, prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, OSD[osd])
            same(got, want, (make.__name__, osd, W, F))
            assert (got[0][:, 49] == 0).all() and (got[3][:, 49] == prior[49]).all()
            assert np.array_equal(d.decode(syn & 1, prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, OSD[osd])[1], got[1])
    assert want[1].any() and (~want[1]).any()


def test_cli_equals_run_dem(tmp_path, capsys):
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 6, 0.02)
    cr = window.phenomenological_rounds("[[72, 12, 6]]", 6)
    want = mc.run_dem(H, L, probs, 300, distance=6, seed=9, max_iter=MAX_ITER, osd=True, window=(4, 2), check_round=cr)
    out = tmp_path / "cli.json"
    mc.main(["--phenomenological", "[[72, 12, 6]]", "6", "--p", "0.02", "--window", "4", "2", "--trials", "300", "--seed", "9",
             "--max-iter", str(MAX_ITER), "--osd", "--out", str(out)])
    import json
    res = json.loads(out.read_text())
    assert res["window"] == [4, 2] and res["distance"] == 6 and len(res["points"]) == 1
    assert [res["points"][0][k] for k in _lib.COUNTER_NAMES] == want.tolist() and want[0] == 300
    assert "phenomenological" in capsys.readouterr().out
