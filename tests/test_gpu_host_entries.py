"""GPU: the host-array entry points of the C ABI against their device-pointer siblings and against themselves -- every
comparison bit for bit, on Steane 3 x 7 and [[72, 12, 6]], B = 5 unless a test says otherwise.

  host = device      the host entry returns what the _device entry writes into torch buffers on the same inputs
  omitted outputs    a null output changes none of the others
  decode paths       qbp_decode_batch through the pinned buffer, and through pinned staging in one and in three pieces
  add / set          sampled Monte-Carlo entries ADD to the caller's arrays, stored-error entries SET the counters
  window MC tables   the window decoder's cached Lx columns and sampler thresholds follow the call's Lx and probs
  refusal, reuse     a call refused by the device entry after the uploads leaves a handle that decodes like a fresh one
  prior messages     the two messages of the prior check, before any output is written"""
import types

import numpy as np
import pytest

from qldpc_amd import _lib, bp, codes, gd, mc, relay, shots

pytestmark = pytest.mark.gpu

B, MAX_ITER, ALPHA, DAMPING, CLIP, T, SEED = 5, 6, 0.9, 0.75, 20.0, 400, 13
NC = _lib.NUM_COUNTERS
MC = dict(seed=SEED, max_iter=MAX_ITER, variant=_lib.MIN_SUM, alpha=ALPHA, damping=DAMPING, clip_llr=CLIP)
SENTINEL = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77, np.dtype(np.float64): -1234.5,
            np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5, np.dtype(np.int64): -99}
CASES = {"steane": ("steane", 0.12, 2, 1), "72": ("[[72, 12, 6]]", 0.05, 3, 6)}      # code, p, window size, checks per round


def fill(shape, dtype):
    return np.full(shape, SENTINEL[np.dtype(dtype)], dtype)


def ptr(a):
    return None if a is None else a.ctypes.data


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g.astype(w.dtype), w, equal_nan=w.dtype.kind == "f"), (what, i)


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    name, p, W, per_round = CASES[request.param]
    code = codes.load_code(name)
    c = types.SimpleNamespace(name=request.param, H=np.ascontiguousarray(code.Hx, np.uint8), p=p, W=W)
    c.m, c.n = c.H.shape
    c.csr = bp.csr_from_H(c.H)
    c.L, c.d = (np.ones((1, c.n), np.uint8), 3) if name == "steane" else (np.ascontiguousarray(code.Lx, np.uint8), code.distance)
    c.check_round = (np.arange(c.m) // per_round).astype(np.int32)
    rng = np.random.default_rng(3)
    c.err = (rng.random((B, c.n)) < p).astype(np.uint8)
    c.err[0] = 0
    c.err[0, :2] = 1                                    # (a pattern BP has work with on both matrices)
    c.syn = (c.err.astype(np.int64) @ c.H.T % 2).astype(np.uint8)
    c.prior = mc.prior_of(p, c.n)
    c.probs = np.linspace(0.5 * p, 1.5 * p, c.n)
    c.relay_cfg = relay.RelayConfig(relay.relay_gammas(c.n, 3, 0.125, (-0.24, 0.66), 4), [4] * 3, 1, ALPHA)
    c.gd_cfg = gd.GDConfig(3, 4, 25.0, gd.MIN_SUM, ALPHA, CLIP)

    def fresh():
        dec = _lib.Decoder(*c.csr, bp.DEVICE)
        dec.relay_configure(c.relay_cfg)
        dec.gd_configure(c.gd_cfg)
        dec.lsd_configure(1)
        dec.layered_configure(None)
        return dec
    c.fresh = fresh
    c.window = lambda: _lib.WindowDecoder(*c.csr, c.check_round, c.W, 1, bp.DEVICE)
    c.dec = fresh()
    c.wdec = c.window()
    # what the second stages read: the outputs of a short min-sum decode
    c.hard, _, _, c.llr = c.dec.decode(c.syn, c.prior, 2, _lib.MIN_SUM, ALPHA, DAMPING, CLIP)
    c.order = np.stack([np.random.default_rng(20 + r).permutation(c.n) for r in range(B)]).astype(np.int32)
    c.det = shots.pack_bits(c.syn)
    c.actual = np.random.default_rng(8).integers(0, 1 << c.L.shape[0], B, dtype=np.uint64)
    return c


def on_device(call, inputs, outputs):
    """call(input pointers, output pointers) on torch copies of `inputs` and sentinel-filled buffers of the shapes and
    dtypes of `outputs` (arrays; int64 ones start at zero: counters are added to) -> the outputs as numpy arrays."""
    import torch
    dev = torch.device("cuda", bp.DEVICE)
    d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in inputs]
    start = [np.zeros_like(o) if o.dtype == np.int64 else fill(o.shape, o.dtype) for o in outputs]
    d_out = [torch.from_numpy(s.view(np.int64) if s.dtype == np.uint64 else s).to(dev) for s in start]
    call([t.data_ptr() for t in d_in], [t.data_ptr() for t in d_out])
    torch.cuda.synchronize(dev)
    return [t.cpu().numpy().view(o.dtype).reshape(o.shape) for t, o in zip(d_out, outputs)]


# ---- host = device ---------------------------------------------------------------------------------------------------------

def test_decode_equals_device(case):
    c, d = case, case.dec
    for variant in (_lib.SUM_PRODUCT, _lib.MIN_SUM):
        hard, conv, iters, llr = d.decode(c.syn, c.prior, MAX_ITER, variant, ALPHA, DAMPING, CLIP)
        got = on_device(lambda i, o: d.decode_device(i[0], i[1], B, MAX_ITER, variant, ALPHA, DAMPING, CLIP, 0, *o),
                        [c.syn, c.prior], [hard, conv.astype(np.uint8), iters, llr])
        same(got, [hard, conv, iters, llr], ("decode", variant))


def test_osd_equals_device(case):
    c, d = case, case.dec
    ins = [c.syn, c.llr, c.hard]
    for order in (0, 2):
        sol = d.osd(c.syn, c.llr, c.hard, "cs", order)
        got = on_device(lambda i, o: d.osd_device(*i, B, o[0], "cs", order), ins, [sol])
        same(got, [sol], ("osd", order))
        sol = d.osd(c.syn, c.llr, c.hard, "cs", order, column_order=c.order)
        got = on_device(lambda i, o: d.osd_device(*i[:3], B, o[0], "cs", order, d_order=i[3]), ins + [c.order], [sol])
        same(got, [sol], ("osd ordered", order))


def test_relay_gd_lsd_equal_device(case):
    c, d = case, case.dec
    bytes_of = lambda outs: [a.astype(np.uint8) if a.dtype == bool else a for a in outs]       # (converged: bool)
    want = list(d.relay_decode(c.syn, c.prior))
    same(on_device(lambda i, o: d.relay_decode_device(*i, B, *o), [c.syn, c.prior], bytes_of(want)), want, "relay_decode")
    want = list(d.gd_decode(c.syn, c.prior))
    same(on_device(lambda i, o: d.gd_decode_device(*i, B, *o), [c.syn, c.prior], bytes_of(want)), want, "gd_decode")
    want = list(d.lsd(c.syn, c.llr, c.hard))
    same(on_device(lambda i, o: d.lsd_device(*i, B, *o), [c.syn, c.llr, c.hard], want), want, "lsd")


def test_decode_shots_equals_device(case):
    c, d = case, case.dec
    for flags in (0, _lib.FLAG_OSD0):
        cnt, pred, conv = d.decode_shots(c.L, c.det, c.prior, c.actual, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags)
        got = on_device(lambda i, o: d.decode_shots_device(c.L, i[0], i[1], B, i[2], o[0], o[1], o[2], MAX_ITER, _lib.MIN_SUM,
                                                           ALPHA, DAMPING, CLIP, flags),
                        [c.det, c.actual.view(np.int64), c.prior], [pred, conv.astype(np.uint8), cnt])
        same(got, [pred, conv, cnt], ("decode_shots", flags))
        assert cnt.sum() > 0


def test_window_decode_equals_device(case):
    c, w = case, case.wdec
    for flags in (0, _lib.osd_flags("cs", 0)):
        want = list(w.decode(c.syn, c.prior, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags))
        got = on_device(lambda i, o: w.decode_device(i[0], i[1], B, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags, *o),
                        [c.syn, c.prior], [want[0], want[1].astype(np.uint8)] + want[2:])
        same(got, want, ("window decode", flags))


def test_mc_counters_equal_device(case):
    c, d = case, case.dec
    kw = dict(MC, flags=_lib.FLAG_OSD0)
    weight = 2 if c.name == "steane" else 5
    for what, host, device in (
            ("mc_run", lambda: d.mc_run(c.L, c.d, c.p, c.prior, 0, T, **kw),
             lambda i, o: d.mc_run_device(c.L, c.d, c.p, i[0], 0, T, o[0], **kw)),
            ("mc_run_probs", lambda: d.mc_run_probs(c.L, c.d, c.probs, c.prior, 0, T, **kw),
             lambda i, o: d.mc_run_probs_device(c.L, c.d, c.probs, i[0], 0, T, o[0], **kw)),
            ("mc_run_weight", lambda: d.mc_run_weight(c.L, c.d, weight, c.prior, 0, T, **kw),
             lambda i, o: d.mc_run_weight_device(c.L, c.d, weight, i[0], 0, T, o[0], **kw))):
        want = host()
        assert want[0] == T, what
        same(on_device(device, [c.prior], [want]), [want], what)


# ---- omitted outputs -------------------------------------------------------------------------------------------------------

def omit_each(call, shapes, what):
    """call(outputs) -> rc with every output present, then with each one null in turn: the others do not change."""
    full = [fill(s, t) for s, t in shapes]
    assert call(full) == 0, what
    for k in range(len(shapes)):
        outs = [None if i == k else fill(s, t) for i, (s, t) in enumerate(shapes)]
        assert call(outs) == 0, (what, k)
        same([o for o in outs if o is not None], [f for i, f in enumerate(full) if i != k], (what, k))
    return full


def test_omitted_outputs(case):
    c, d, lib = case, case.dec, _lib.load()
    n = c.n
    syn, pr, llr, hard = c.syn.ctypes.data, c.prior.ctypes.data, c.llr.ctypes.data, c.hard.ctypes.data
    four = [((B, n), np.uint8), (B, np.uint8), (B, np.int32), ((B, n), np.float64)]
    omit_each(lambda o: lib.qbp_decode_batch(d._h, syn, pr, B, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, 0,
                                             *(ptr(a) for a in o)), four, "decode")
    omit_each(lambda o: lib.qbp_relay_decode_batch(d._h, syn, pr, B, *(ptr(a) for a in o)),
              four + [(B, np.int32), (B, np.int32)], "relay")
    omit_each(lambda o: lib.qbp_gd_decode_batch(d._h, syn, pr, B, *(ptr(a) for a in o)), four + [(B, np.int32)], "gd")
    sol, stats = fill((B, n), np.uint8), fill((B, 4), np.int32)
    assert lib.qbp_lsd_batch(d._h, syn, llr, hard, B, sol.ctypes.data, stats.ctypes.data) == 0
    alone = fill((B, n), np.uint8)
    assert lib.qbp_lsd_batch(d._h, syn, llr, hard, B, alone.ctypes.data, None) == 0
    same([alone], [sol], "lsd without stats")
    w = c.wdec
    omit_each(lambda o: lib.qbp_window_decode_batch(w._h, syn, pr, B, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP,
                                                    _lib.osd_flags("cs", 0), *(ptr(a) for a in o)),
              four + [(B, np.int32)], "window")

    # recorded shots: predictions and converged are outputs; without `actual` nothing is compared, so only they are
    def shots_call(actual, pred, conv):
        cnt = np.zeros(NC, np.int64)
        assert lib.qbp_decode_shots(d._h, c.L.ctypes.data, c.L.shape[0], c.det.ctypes.data, ptr(actual), B, pr, MAX_ITER,
                                    _lib.MIN_SUM, ALPHA, DAMPING, CLIP, _lib.FLAG_OSD0, ptr(pred), ptr(conv),
                                    cnt.ctypes.data) == 0
        return cnt
    pred, conv = fill(B, np.uint64), fill(B, np.uint8)
    cnt = shots_call(c.actual, pred, conv)
    p2, c2 = fill(B, np.uint64), fill(B, np.uint8)
    shots_call(None, p2, c2)
    same([p2, c2], [pred, conv], "shots without actual")
    p2, c2 = fill(B, np.uint64), fill(B, np.uint8)
    same([shots_call(c.actual, None, c2), c2], [cnt, conv], "shots without predictions")
    same([shots_call(c.actual, p2, None), p2], [cnt, pred], "shots without converged")
    same([shots_call(c.actual, None, None)], [cnt], "shots, counters alone")

    # the spectrum call without its iteration histogram
    def spectrum_call(with_hist):
        cnt, spec = np.zeros(NC, np.int64), np.zeros((_lib.SPECTRUM_ROWS, n + 1), np.int64)
        hist = np.zeros(MAX_ITER + 1, np.int64) if with_hist else None
        assert lib.qbp_mc_run_spectrum(d._h, c.L.ctypes.data, c.L.shape[0], c.d, c.probs.ctypes.data, 1, SEED, 0, T, pr,
                                       MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, _lib.FLAG_OSD0, cnt.ctypes.data,
                                       spec.ctypes.data, ptr(hist)) == 0
        return cnt, spec, hist
    cnt, spec, hist = spectrum_call(True)
    assert hist.sum() == T and spec.sum() > 0
    same(spectrum_call(False)[:2], [cnt, spec], "spectrum without iter_hist")


# ---- the three paths of qbp_decode_batch -----------------------------------------------------------------------------------

def pinned_bytes(b, m, n):
    """The size qbp_decode_batch compares with 256 KiB: syndromes, prior, llr, iters, hard, converged in one buffer."""
    up8 = lambda x: (x + 7) & ~7
    return up8(b * m) + n * 8 + b * n * 8 + up8(b * 4) + b * n + b


def test_decode_batch_paths():
    """[[72, 12, 6]]: B = 1 and the largest B within 256 KiB go through the mapped pinned buffer; the next B is staged
    and copied out in one piece; B = 4000 with all outputs has 72 + 1 + 4 + 576 = 653 bytes of output per syndrome, so
    copy_out cuts pieces of 2^20 // 653 + 1 = 1606 syndromes -- 1606, 1606, 788 -- and the third reuses the first
    staging buffer.  Each equals the device entry's result, in buffers that held a sentinel."""
    code = codes.load_code("[[72, 12, 6]]")
    H = np.ascontiguousarray(code.Hx, np.uint8)
    m, n = H.shape
    d = _lib.Decoder(*bp.csr_from_H(H), bp.DEVICE)
    lib = _lib.load()
    first_staged = next(b for b in range(1, 4000) if pinned_bytes(b, m, n) > 256 * 1024)
    assert first_staged == 380 and (1 << 20) // 653 + 1 == 1606
    p = 0.05
    err = (np.random.default_rng(17).random((4000, n)) < p).astype(np.uint8)
    syn_all = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    prior = mc.prior_of(p, n)
    for b in (1, first_staged - 1, first_staged, 4000):
        syn = np.ascontiguousarray(syn_all[:b])
        outs = [fill((b, n), np.uint8), fill(b, np.uint8), fill(b, np.int32), fill((b, n), np.float64)]
        assert lib.qbp_decode_batch(d._h, syn.ctypes.data, prior.ctypes.data, b, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING,
                                    CLIP, 0, *(o.ctypes.data for o in outs)) == 0
        want = on_device(lambda i, o: d.decode_device(i[0], i[1], b, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, 0, *o),
                         [syn, prior], outs)
        same(outs, want, ("decode path", b))
        assert 0 < outs[1].sum() < b or b == 1                 # (converged and unconverged syndromes in the batch)


# ---- ADD and SET -----------------------------------------------------------------------------------------------------------

def test_add_and_set(case):
    c, d, lib = case, case.dec, _lib.load()
    kw = dict(MC, flags=_lib.FLAG_OSD0)
    head = (d._h, c.L.ctypes.data, c.L.shape[0], c.d)
    tail = (c.prior.ctypes.data, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, _lib.FLAG_OSD0)
    plain = d.mc_run_probs(c.L, c.d, c.probs, c.prior, 0, T, **kw)
    start = np.arange(7, 7 + NC, dtype=np.int64)
    cnt = start.copy()
    assert lib.qbp_mc_run_probs(*head, c.probs.ctypes.data, 1, SEED, 0, T, *tail, cnt.ctypes.data) == 0
    assert np.array_equal(cnt, start + plain) and plain[0] == T             # ADDED
    errors = d.mc_sample_errors_probs(c.probs, 0, T, seed=SEED)
    cnt = start.copy()
    assert lib.qbp_mc_run_errors(*head, errors.ctypes.data, T, *tail, cnt.ctypes.data) == 0
    assert np.array_equal(cnt, plain)                                       # SET: the same trials, nothing of `start`
    # the spectrum tables, added to across two calls
    whole = d.mc_run_spectrum(c.L, c.d, c.probs, c.prior, 0, T, **kw)
    a = d.mc_run_spectrum(c.L, c.d, c.probs, c.prior, 0, T // 3, **kw)
    b = d.mc_run_spectrum(c.L, c.d, c.probs, c.prior, T // 3, T, spectrum=a[1], iter_hist=a[2], **kw)
    assert b[1] is a[1] and b[2] is a[2]
    same([a[0] + b[0], b[1], b[2]], whole, "spectrum in two calls")
    assert whole[1].sum() > 0 and whole[2].sum() == T


# ---- the Monte-Carlo tables of the window decoder --------------------------------------------------------------------------

def test_window_mc_tables(case):
    c, w, lib = case, case.wdec, _lib.load()
    kw = dict(MC, flags=_lib.osd_flags("cs", 0))
    run = lambda dec, L, probs: dec.mc_run_probs(L, c.d, probs, c.prior, 0, T, **kw)
    probs2 = np.ascontiguousarray(c.probs[::-1]) * 2.0
    L2 = c.L.copy()
    L2[:, : c.n // 2] ^= 1                                                  # (as many rows as L: only the bits differ)
    fresh = {key: run(c.window(), L, pb) for key, (L, pb) in
             dict(a=(c.L, c.probs), b=(c.L, probs2), c=(L2, c.probs)).items()}
    assert not np.array_equal(fresh["a"], fresh["b"]) and not np.array_equal(fresh["a"], fresh["c"])
    for key, L, pb in (("a", c.L, c.probs), ("b", c.L, probs2), ("a", c.L, c.probs), ("c", L2, c.probs),
                       ("a", c.L, c.probs)):
        assert np.array_equal(run(w, L, pb), fresh[key]), key
    cnt = fill(NC, np.int64)
    assert lib.qbp_window_mc_run_errors(w._h, c.L.ctypes.data, c.L.shape[0], c.d, c.err.ctypes.data, 0, c.prior.ctypes.data,
                                        MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, 0, cnt.ctypes.data) == 0
    assert not cnt.any()                                                    # T = 0 SETS the counters to zero


# ---- a refusal after the uploads, then the handle again --------------------------------------------------------------------

def test_refusal_then_reuse(case):
    """The entries whose device call can still refuse once the inputs are on their way (read off qbp.hip):
      qbp_decode_batch        two column-sum order flags without QBP_FLAG_DENSE_F_COLSUM_ITER0 are judged by the device
                              entry: QBP_E_INVALID, on the pinned path (B = 5) and on the staged one
      qbp_decode_shots        the same flags, judged inside the launch chain
      qbp_message_histograms  a NaN prior gives a message range that is not finite, known after the messages are computed
    No such refusal is reachable in the others: qbp_check_messages has resolved the column order before it uploads;
    qbp_osd_batch*, qbp_lsd_batch, the Relay-BP / BPGD entries and the Monte-Carlo entries repeat in the device call only
    checks the host entry has already passed (their remaining refusal, more than 2^30 records, needs a batch no test
    allocates); the window entries check every sub-handle's kernel choice before they upload."""
    c, d, lib = case, case.dec, _lib.load()
    n, pr = c.n, c.prior.ctypes.data
    two_orders = _lib.FLAG_DENSE_F_COLSUM | _lib.FLAG_PAIRWISE_COLSUM
    big = next(b for b in range(1, 1 << 16) if pinned_bytes(b, c.m, n) > 256 * 1024)
    syn_big = np.ascontiguousarray(np.resize(c.syn, (big, c.m)))

    def decode(dec, syn, flags):
        b = syn.shape[0]
        outs = [fill((b, n), np.uint8), fill(b, np.uint8), fill(b, np.int32), fill((b, n), np.float64)]
        rc = lib.qbp_decode_batch(dec._h, syn.ctypes.data, pr, b, MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags,
                                  *(o.ctypes.data for o in outs))
        return rc, outs
    for syn in (c.syn, syn_big):
        rc, outs = decode(d, syn, two_orders)
        assert rc == _lib.E_INVALID and b"column-sum order" in lib.qbp_last_error()
        same(outs, [fill(o.shape, o.dtype) for o in outs], "a refused decode writes nothing")
        rc, outs = decode(d, syn, 0)
        assert rc == 0
        same(outs, decode(c.fresh(), syn, 0)[1], ("decode after a refusal", syn.shape[0]))

    def decode_shots(dec, flags):
        cnt, pred, conv = np.zeros(NC, np.int64), fill(B, np.uint64), fill(B, np.uint8)
        rc = lib.qbp_decode_shots(dec._h, c.L.ctypes.data, c.L.shape[0], c.det.ctypes.data, c.actual.ctypes.data, B, pr,
                                  MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP, flags, pred.ctypes.data, conv.ctypes.data,
                                  cnt.ctypes.data)
        return rc, [cnt, pred, conv]
    rc, outs = decode_shots(d, _lib.FLAG_OSD0 | two_orders)
    assert rc == _lib.E_INVALID and b"column-sum order" in lib.qbp_last_error()
    same(outs, [np.zeros(NC, np.int64), fill(B, np.uint64), fill(B, np.uint8)], "refused shots write nothing")
    rc, outs = decode_shots(d, _lib.FLAG_OSD0)
    assert rc == 0
    same(outs, decode_shots(c.fresh(), _lib.FLAG_OSD0)[1], "shots after a refusal")

    def histograms(dec, prior):
        edges, h0, h1 = fill(9, np.float64), fill(8, np.int64), fill(8, np.int64)
        rc = lib.qbp_message_histograms(dec._h, c.syn.ctypes.data, c.err.ctypes.data, prior.ctypes.data, B, _lib.MIN_SUM,
                                        1.0, 1.0, np.inf, 0, 0, 8, edges.ctypes.data, h0.ctypes.data, h1.ctypes.data)
        return rc, [edges, h0, h1]
    nan = c.prior.copy()
    nan[1] = np.nan
    rc, outs = histograms(d, nan)
    assert rc == _lib.E_INVALID and b"not finite" in lib.qbp_last_error()
    same(outs, [fill(9, np.float64), fill(8, np.int64), fill(8, np.int64)], "refused histograms write nothing")
    rc, outs = histograms(d, c.prior)
    assert rc == 0 and outs[1].sum() + outs[2].sum() == B * len(d.col_idx)
    same(outs, histograms(c.fresh(), c.prior)[1], "histograms after a refusal")


# ---- the two messages of the prior check -----------------------------------------------------------------------------------

def test_prior_messages(case):
    c, d, w, lib = case, case.dec, case.wdec, _lib.load()
    n, syn = c.n, c.syn.ctypes.data
    nan, inf = c.prior.copy(), c.prior.copy()
    nan[n - 1] = np.nan
    inf[2] = -np.inf
    four = [fill((B, n), np.uint8), fill(B, np.uint8), fill(B, np.int32), fill((B, n), np.float64)]
    more = [fill(B, np.int32), fill(B, np.int32)]
    cnt, pred = fill(NC, np.int64), fill(B, np.uint64)
    o = [a.ctypes.data for a in four + more]
    L = (c.L.ctypes.data, c.L.shape[0])
    dec_args = (MAX_ITER, _lib.MIN_SUM, ALPHA, DAMPING, CLIP)
    refused = {
        "decode": (b"is NaN", lambda: lib.qbp_decode_batch(d._h, syn, nan.ctypes.data, B, *dec_args, 0, *o[:4])),
        "decode_shots": (b"is NaN", lambda: lib.qbp_decode_shots(d._h, *L, c.det.ctypes.data, c.actual.ctypes.data, B,
                                                                  nan.ctypes.data, *dec_args, 0, pred.ctypes.data, o[1],
                                                                  cnt.ctypes.data)),
        "window decode": (b"is NaN", lambda: lib.qbp_window_decode_batch(w._h, syn, nan.ctypes.data, B, *dec_args, 0,
                                                                          *o[:5])),
        "window mc_run_probs": (b"is NaN", lambda: lib.qbp_window_mc_run_probs(w._h, *L, c.d, c.probs.ctypes.data, 1, SEED, 0,
                                                                                T, nan.ctypes.data, *dec_args, 0,
                                                                                cnt.ctypes.data)),
        "mc_run": (b"is NaN", lambda: lib.qbp_mc_run(d._h, *L, c.d, c.p, 1, SEED, 0, T, nan.ctypes.data, *dec_args, 0,
                                                     cnt.ctypes.data)),
        "relay_decode": (b"is not finite", lambda: lib.qbp_relay_decode_batch(d._h, syn, inf.ctypes.data, B, *o)),
        "gd_decode": (b"is not finite", lambda: lib.qbp_gd_decode_batch(d._h, syn, inf.ctypes.data, B, *o[:5])),
        "layered decode": (b"is not finite", lambda: lib.qbp_decode_batch(d._h, syn, inf.ctypes.data, B, *dec_args,
                                                                           _lib.FLAG_LAYERED, *o[:4])),
    }
    for what, (message, call) in refused.items():
        assert call() == _lib.E_INVALID, what
        err = lib.qbp_last_error()
        assert message in err and (b"prior[%d]" % (n - 1 if message == b"is NaN" else 2)) in err, (what, err)
        same(four + more + [cnt, pred], [fill(a.shape, a.dtype) for a in four + more + [cnt, pred]], what)
    assert lib.qbp_decode_batch(d._h, syn, inf.ctypes.data, B, *dec_args, 0, *o[:4]) == 0      # (+-inf are legal there)
