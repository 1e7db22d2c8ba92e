"""GPU: order-w OSD on matrices beyond the one-wavefront kernel (QBP_FLAG_OSD_LARGE, osd_order_blocked_kernel), bit for
bit against the numpy statement of the spec (tests/osd_order_oracle.py) and, where both apply, against
osd_order_kernel.  Small matrices reach the new kernel through QBP_OPT_OSD_BIG = 1 / 3 on a FRESH decoder."""
import functools
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import osd_order_oracle as ordo
import osd_ordered_oracle as ordd
from qldpc_amd import _lib, bp, codes, dem, mc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = [("cs", 1), ("cs", 7), ("cs", 64), ("e", 1), ("e", 4), ("e", 12)]


def _fresh(H):
    row_ptr, col_idx, m, n = bp.csr_from_H(H)
    return _lib.Decoder(row_ptr, col_idx, m, n, bp.DEVICE)


def _forced(H, big=1):
    dec = _fresh(H)
    dec.set_option(_lib.OPT_OSD_BIG, big)
    return dec


def _oracle(H, syn, llr, hard, method, w, reds=None):
    reds = reds or [ordo.reduce(H, s, l, h) for s, l, h in zip(syn, llr, hard)]
    return np.stack([ordo.osd_order(H, s, l, h, w, method, red=r) for s, l, h, r in zip(syn, llr, hard, reds)]), reds


@pytest.mark.parametrize("name", ("[[72, 12, 6]]", "[[144, 12, 12]]"))
def test_forced_path_equals_the_one_wavefront_kernel(name):
    code = codes.load_code(name)
    H = code.Hx.astype(np.int64)
    plain = _fresh(code.Hx)
    rng = np.random.default_rng(21)
    parts = []
    for p in (0.08, 0.10, 0.12):
        err = (rng.random((600, code.n)) < p).astype(np.uint8)
        syn = (err @ H.T % 2).astype(np.uint8)
        hard, conv, _, llr = plain.decode(syn, mc.prior_of(p, code.n), 20)
        f = np.flatnonzero(~conv)[:70]
        parts.append((syn[f], llr[f], hard[f]))
    # random posteriors and hard decisions on syndromes of errors
    err = (rng.random((60, code.n)) < 0.1).astype(np.uint8)
    rl = rng.standard_normal((60, code.n)) * 3
    parts.append(((err @ H.T % 2).astype(np.uint8), rl, (rng.random((60, code.n)) < 0.3).astype(np.uint8)))
    syn, llr, hard = (np.concatenate(x) for x in zip(*parts))
    assert len(syn) >= 200, len(syn)
    forced = {big: _forced(code.Hx, big) for big in (1, 3)}
    reds = None
    changed = 0
    for method, w in CONFIGS:
        base = plain.osd(syn, llr, hard, method=method, order=w)
        want, reds = _oracle(H, syn, llr, hard, method, w, reds)
        assert np.array_equal(base, want), (method, w)
        for big, dec in forced.items():
            got = dec.osd(syn, llr, hard, method=method, order=w, large=True)
            bad = np.flatnonzero((got != want).any(1))
            assert len(bad) == 0, (method, w, big, bad[:10])
        changed += int((want != np.stack([r.x0 for r in reds])).any(1).sum())
    assert changed > 0
    # without the flag the forced decoders keep today's answer
    with pytest.raises(_lib.QbpError) as e:
        forced[1].osd(syn[:2], llr[:2], hard[:2], method="cs", order=7)
    assert e.value.code == _lib.E_UNSUPPORTED


@pytest.mark.parametrize("tag", ("72", "144"))
def test_forced_path_inconsistent_syndromes_get_osd0(tag):
    d = np.load(os.path.join(GOLDEN, "osd_inconsistent.npz"))
    H = d[f"{tag}/H"].astype(np.int64)
    syn, llr, hard, want = (d[f"{tag}/{k}"] for k in ("syndromes", "llr", "hard", "solution"))
    dec = _forced(H)
    assert np.array_equal(dec.osd0(syn, llr, hard), want)
    assert np.array_equal(dec.osd(syn, llr, hard, method="cs", order=7, large=True), want)


def _edge_cases():
    rng = np.random.default_rng(8)
    I6 = np.eye(6, dtype=np.int64)
    cases = {"no_free_columns": I6,
             "three_free_columns": np.hstack([I6, rng.integers(0, 2, (6, 3))]),
             "one_row": rng.integers(0, 2, (1, 9)) | np.eye(1, 9, dtype=np.int64)}
    for n in (64, 65, 128):
        cases[f"n{n}"] = (rng.random((20, n)) < 0.15).astype(np.int64)
    z = (rng.random((10, 40)) < 0.2).astype(np.int64)
    z[:, 7] = 0
    cases["zero_column"] = z
    return cases


@pytest.mark.parametrize("case", sorted(_edge_cases()))
def test_edge_shapes_forced_path(case):
    H = _edge_cases()[case]
    m, n = H.shape
    rng = np.random.default_rng(4)
    B = 24
    err = (rng.random((B, n)) < 0.2).astype(np.uint8)
    syn = (err @ H.T % 2).astype(np.uint8)
    llr = rng.choice([0.5, 1.0, 2.0, 3.5], size=(B, n)) * np.where(rng.random((B, n)) < 0.5, -1.0, 1.0)
    hard = (rng.random((B, n)) < 0.3).astype(np.uint8)
    special = llr.copy()
    pick = rng.random((B, n))
    special[pick < 0.05] = np.nan
    special[(pick >= 0.05) & (pick < 0.1)] = np.inf
    special[(pick >= 0.1) & (pick < 0.15)] = -np.inf
    nan0 = llr.copy()
    nan0[:, 0] = np.nan                    # with hard[:, 0] set the OSD-0 cost is NaN wherever column 0 stays 1
    hard_nan0 = hard.copy()
    hard_nan0[:, 0] = 1
    for big in (1, 3):
        dec = _forced(csr_matrix(H.astype(np.uint8)), big)
        for L, hd in ((llr, hard), (special, hard), (nan0, hard_nan0)):
            for method, w in (("cs", 7), ("e", 12), ("cs", 1)):
                got = dec.osd(syn, L, hd, method=method, order=w, large=True)
                want = ordo.osd_order_batch(H, syn, L, hd, w, method)
                assert np.array_equal(got, want), (case, big, method, w, np.flatnonzero((got != want).any(1))[:8])


@functools.lru_cache(maxsize=None)
def _natural(name, rounds, p, shots):
    """BP(20) failures of a phenomenological matrix: (H dense int64, decoder, syn, llr, hard)."""
    Hs, L, probs = dem.phenomenological(name, rounds, p)
    H = Hs.toarray().astype(np.int64)
    n = H.shape[1]
    err = (np.random.default_rng(5).random((shots, n)) < p).astype(np.uint8)
    syn = (err @ H.T % 2).astype(np.uint8)
    dec = _fresh(Hs)
    hard, conv, _, llr = dec.decode(syn, mc.dem_prior(probs), 20)
    f = np.flatnonzero(~conv)
    return H, dec, syn[f], llr[f], hard[f]


def _check_natural(H, dec, syn, llr, hard, method, w, reds=None):
    got = dec.osd(syn, llr, hard, method=method, order=w, large=True)
    want, reds = _oracle(H, syn, llr, hard, method, w, reds)
    assert np.array_equal((got.astype(np.int64) @ H.T) % 2, syn), (method, w)
    assert np.array_equal(got, want), (method, w, np.flatnonzero((got != want).any(1)))
    return int((want != np.stack([r.x0 for r in reds])).any(1).sum()), reds


def test_smallest_natural_matrix_beyond_the_limit():
    """432 x 1296 ([[72,12,6]] over 12 rounds), rows per thread 1."""
    H, dec, syn, llr, hard = _natural("[[72, 12, 6]]", 12, 0.03, 96)
    assert H.shape == (432, 1296) and len(syn) >= 12, (H.shape, len(syn))
    syn, llr, hard = syn[:12], llr[:12], hard[:12]
    assert len(np.unique(np.abs(llr[0]))) < H.shape[1]          # |llr| ties are present
    c7, reds = _check_natural(H, dec, syn, llr, hard, "cs", 7)
    e6, _ = _check_natural(H, dec, syn, llr, hard, "e", 6, reds)
    assert c7 >= 1 and e6 >= 1, (c7, e6)                        # the search changes solutions here


def test_864_by_2592():
    H, dec, syn, llr, hard = _natural("[[144, 12, 12]]", 12, 0.02, 24)
    assert H.shape == (864, 2592) and len(syn) >= 4, (H.shape, len(syn))
    _, reds = _check_natural(H, dec, syn[:4], llr[:4], hard[:4], "e", 6)
    _check_natural(H, dec, syn[:2], llr[:2], hard[:2], "cs", 7, reds[:2])


def test_two_rows_per_thread():
    """1296 x 3888 ([[144,12,12]] over 18 rounds)."""
    H, dec, syn, llr, hard = _natural("[[144, 12, 12]]", 18, 0.02, 24)
    assert H.shape == (1296, 3888) and len(syn) >= 2, (H.shape, len(syn))
    _, reds = _check_natural(H, dec, syn[:2], llr[:2], hard[:2], "e", 4)
    _check_natural(H, dec, syn[:1], llr[:1], hard[:1], "cs", 3, reds[:1])


def _raw_osd(dec, flags, syn, llr, hard):
    syn = np.ascontiguousarray(syn, np.uint8)
    llr = np.ascontiguousarray(llr, np.float64)
    hard = np.ascontiguousarray(hard, np.uint8)
    out = np.full_like(hard, 7)
    rc = _lib.load().qbp_osd_batch(dec._h, flags, syn.ctypes.data, llr.ctypes.data, hard.ctypes.data, len(syn),
                                   out.ctypes.data)
    return rc, out


def test_flag_clear_and_invalid_combinations():
    H, dec, syn, llr, hard = _natural("[[72, 12, 6]]", 12, 0.03, 96)
    args = (syn[:2], llr[:2], hard[:2])
    O = lambda w: w << _lib.OSD_ORDER_SHIFT   # noqa: E731
    for method, w in (("cs", 7), ("e", 6)):
        with pytest.raises(_lib.QbpError) as e:
            dec.osd(*args, method=method, order=w)
        assert e.value.code == _lib.E_UNSUPPORTED
    assert _lib.FLAG_OSD_LARGE == 256
    for flags in (_lib.FLAG_OSD_LARGE, _lib.FLAG_OSD_LARGE | _lib.FLAG_OSD0, _lib.FLAG_OSD_LARGE | O(7),
                  _lib.FLAG_OSD_LARGE | _lib.FLAG_OSD_CS, _lib.FLAG_OSD_LARGE | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | O(3)):
        rc, out = _raw_osd(dec, flags, *args)
        assert rc == -1 and (out == 7).all(), hex(flags)
    rc, out = _raw_osd(dec, _lib.FLAG_OSD_LARGE | _lib.FLAG_OSD_CS | O(7), *args)
    assert rc == 0 and np.array_equal(out, dec.osd(*args, method="cs", order=7, large=True))
    # the one-pivot-at-a-time kernel's matrices stay unsupported
    swaps = _forced(csr_matrix(H.astype(np.uint8)), 2)
    with pytest.raises(_lib.QbpError) as e:
        swaps.osd(*args, method="cs", order=7, large=True)
    assert e.value.code == _lib.E_UNSUPPORTED
    # on a matrix the one-wavefront kernel takes the flag changes nothing
    code = codes.load_code("[[72, 12, 6]]")
    small = _fresh(code.Hx)
    rng = np.random.default_rng(1)
    s = ((rng.random((8, code.n)) < 0.1).astype(np.int64) @ code.Hx.T % 2).astype(np.uint8)
    l = rng.standard_normal((8, code.n))
    h = (l < 0).astype(np.uint8)
    assert np.array_equal(small.osd(s, l, h, method="cs", order=7, large=True), small.osd(s, l, h, method="cs", order=7))


def test_ordered_entry():
    H, dec, syn, llr, hard = _natural("[[72, 12, 6]]", 12, 0.03, 96)
    syn, llr, hard = syn[:4], llr[:4], hard[:4]
    own = np.stack([ordo.sort_order(l) for l in llr])
    for method, w in (("cs", 7), ("e", 6)):
        assert np.array_equal(dec.osd(syn, llr, hard, method=method, order=w, column_order=own, large=True),
                              dec.osd(syn, llr, hard, method=method, order=w, large=True))
    rng = np.random.default_rng(6)
    perm = np.stack([rng.permutation(H.shape[1]) for _ in range(2)])
    got = dec.osd(syn[:2], llr[:2], hard[:2], method="cs", order=7, column_order=perm, large=True)
    assert np.array_equal(got, ordd.osd_order_batch(H, syn[:2], llr[:2], hard[:2], perm, 7, "cs"))
    with pytest.raises(_lib.QbpError) as e:
        dec.osd(syn[:2], llr[:2], hard[:2], method="cs", order=7, column_order=perm)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_inconsistent_syndromes_on_a_large_matrix():
    H, _, syn, llr, hard = _natural("[[72, 12, 6]]", 12, 0.03, 96)
    H2 = np.vstack([H, H[:1]])                                   # 433 x 1296: row 0 once more
    syn2 = np.hstack([syn[:6], 1 - syn[:6, :1]])                 # bits 0 and 432 differ: outside the column space
    dec = _fresh(csr_matrix(H2.astype(np.uint8)))
    want = dec.osd0(syn2, llr[:6], hard[:6])
    assert np.array_equal(dec.osd(syn2, llr[:6], hard[:6], method="cs", order=7, large=True), want)


def test_device_entry_on_torch_buffers():
    import torch
    H, dec, syn, llr, hard = _natural("[[72, 12, 6]]", 12, 0.03, 96)
    syn, llr, hard = syn[:8], llr[:8], hard[:8]
    dev = torch.device("cuda", bp.DEVICE)
    d_syn = torch.from_numpy(np.ascontiguousarray(syn)).to(dev)
    d_llr = torch.from_numpy(np.ascontiguousarray(llr)).to(dev)
    d_hard = torch.from_numpy(np.ascontiguousarray(hard)).to(dev)
    d_sol = torch.empty_like(d_hard)
    stream = torch.cuda.current_stream(dev)
    dec.osd_device(d_syn.data_ptr(), d_llr.data_ptr(), d_hard.data_ptr(), len(syn), d_sol.data_ptr(), method="cs",
                   order=7, stream=stream.cuda_stream, large=True)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_sol.cpu().numpy(), dec.osd(syn, llr, hard, method="cs", order=7, large=True))


def test_sort_keys_beyond_the_lds():
    """n = 8200 > 8192: the sort keys, and with them the search's per-column table, live in the workspace."""
    rng = np.random.default_rng(12)
    m, n = 24, 8200
    H = (rng.random((m, n)) < 0.01).astype(np.int64)
    err = (rng.random((4, n)) < 0.002).astype(np.uint8)
    syn = (err @ H.T % 2).astype(np.uint8)
    llr = rng.choice([0.5, 1.0, 2.0, 3.5, 4.25], size=(4, n))
    hard = np.zeros((4, n), np.uint8)
    dec = _fresh(csr_matrix(H.astype(np.uint8)))
    with pytest.raises(_lib.QbpError) as e:
        dec.osd(syn, llr, hard, method="e", order=5)
    assert e.value.code == _lib.E_UNSUPPORTED
    assert np.array_equal(dec.osd(syn, llr, hard, method="e", order=5, large=True),
                          ordo.osd_order_batch(H, syn, llr, hard, 5, "e"))
    assert np.array_equal(dec.osd(syn[:1], llr[:1], hard[:1], method="cs", order=3, large=True),   # (5 s on the CPU)
                          ordo.osd_order_batch(H, syn[:1], llr[:1], hard[:1], 3, "cs"))


def test_between_the_two_one_wavefront_kernels():
    """360 x 1080 ([[72,12,6]] over 10 rounds): OSD-0 fits the one-wavefront kernel (57 KB of LDS), osd_order_kernel's
    added LDS does not (75 KB).  Without the flag order w stays unsupported; with it the blocked kernel serves it."""
    H, dec, syn, llr, hard = _natural("[[72, 12, 6]]", 10, 0.03, 64)
    assert H.shape == (360, 1080) and len(syn) >= 6, (H.shape, len(syn))
    syn, llr, hard = syn[:6], llr[:6], hard[:6]
    for method, w in (("cs", 7), ("e", 6)):
        with pytest.raises(_lib.QbpError) as e:
            dec.osd(syn, llr, hard, method=method, order=w)
        assert e.value.code == _lib.E_UNSUPPORTED
    c7, reds = _check_natural(H, dec, syn, llr, hard, "cs", 7)
    e6, _ = _check_natural(H, dec, syn, llr, hard, "e", 6, reds)
    assert c7 + e6 >= 1, (c7, e6)
    assert np.array_equal(dec.osd(syn, llr, hard, order=0), np.stack([r.x0 for r in reds]))
    Lx = np.zeros((1, H.shape[1]), np.uint8)
    prior = mc.prior_of(0.03, H.shape[1])
    with pytest.raises(_lib.QbpError) as e:
        dec.mc_run(Lx, 0, 0.03, prior, 0, 64, max_iter=20, flags=_lib.osd_flags("cs", 7))
    assert e.value.code == _lib.E_UNSUPPORTED
    cnt = dec.mc_run(Lx, 0, 0.03, prior, 0, 64, max_iter=20, flags=_lib.osd_flags("cs", 7, large=True))
    assert cnt[0] == 64 and cnt[6] > 0 and cnt[10] == 0
