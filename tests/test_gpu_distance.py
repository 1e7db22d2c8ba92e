"""qbp_distance_search (dist_search_kernel, qbp_distance.hpp) against its numpy statement (tests/distance_oracle.py), bit
for bit: result, hist, codeword and logical mask; trial indices across 2^32 and a seed above 2^32; independence of the
grid, of the split of the range and of the caller's current stream; poisoned outputs; two matrices on one handle and
the decode call after it; the host-only refusals; and a code the project has never seen, from codes.bb_code through
distance.estimate to mc.run_sweep."""
import numpy as np
import pytest

import distance_cases as dc
import distance_oracle as do
from oracle import oracle
from qldpc_amd import _lib, bp, codes, distance, gf2, mc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def fresh(H):
    """A Decoder of its own (options set on it stay on it)."""
    return _lib.Decoder(*bp.csr_from_H(np.asarray(H)))


def raw_call(dec, G, r, L, k, seed, begin, end, result, hist, codeword, mask):
    """qbp_distance_search on poisoned buffers -> rc; None passes a null pointer."""
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    return _lib.load().qbp_distance_search(dec._h, ptr(G), r, ptr(L), k, seed, begin, end, ptr(result), ptr(hist),
                                           ptr(codeword), ptr(mask))


def poisoned(n):
    return (np.full(4, -77, np.int64), np.full(n + 1, 1000, np.int64), np.full(n, SENTINEL, np.uint8),
            np.full(1, 0xDEADBEEFDEADBEEF, np.uint64))


def check_against_statement(c, want, got):
    result, hist, codeword, mask = got
    assert np.array_equal(result, want["result"]), (result, want["result"])
    assert np.array_equal(hist, want["hist"])
    if want["codeword"] is None:
        assert codeword is None and mask is None
    else:
        assert np.array_equal(codeword, want["codeword"]) and mask == want["logical_mask"]


@pytest.mark.parametrize("name", dc.PARITY)
def test_equals_the_statement(name):
    c = dc.case(name)
    dec = bp.decoder_for(c.H)
    check_against_statement(c, dc.statement(name), dec.distance_search(c.G, c.L, c.begin, c.begin + c.trials, seed=c.seed))
    assert dec.info("threads") == 64 and dec.info("grid") >= 1
    W, NP = (c.n + 31) // 32, max(4, 1 << (c.n - 1).bit_length())
    lds = ((max(8 * NP, 4 * c.G.shape[0] * (W + 1)) + 7) & ~7) + 2 * NP      # dist_lds_bytes of qbp_distance.hpp
    assert dec.info("lds_bytes") == (lds + 15) & ~15


def test_the_cases_are_what_the_module_says():
    assert dc.case("steane").G.shape == (4, 7)
    for name in dc.BOUNDARY:
        n, r = (int(x[1:]) for x in name.split("_"))
        assert dc.case(name).G.shape == (r, n) and dc.statement(name)["result"][1] > 0
    c = dc.case("72z")
    assert c.begin < 1 << 32 < c.begin + c.trials and c.seed > 1 << 32
    assert dc.case("k64").L.shape == (64, 72) and dc.statement("k64")["logical_mask"] == 1 << 63
    d = dc.case("dup")
    assert not d.G[47:49].any() and np.array_equal(d.G[42:47], d.G[:5]) and d.G.shape[0] > gf2.rank(d.G)


def test_an_L_that_detects_nothing_leaves_codeword_and_mask():
    c = dc.case("nothing")
    dec = bp.decoder_for(c.H)
    result, hist, codeword, mask = poisoned(c.n)
    assert raw_call(dec, c.G, c.G.shape[0], c.L, c.L.shape[0], c.seed, c.begin, c.begin + c.trials, result, hist, codeword,
                    mask) == 0
    assert result.tolist() == [c.trials, -1, -1, -1] and np.all(hist == 1000)
    assert np.all(codeword == SENTINEL) and mask[0] == 0xDEADBEEFDEADBEEF
    assert dc.statement("nothing")["result"].tolist() == result.tolist()


def test_poisoned_outputs_hist_is_added_to_and_optional_outputs():
    c, want = dc.case("72x"), dc.statement("72x")
    dec = bp.decoder_for(c.H)
    result, hist, codeword, mask = poisoned(c.n)
    args = (dec, c.G, c.G.shape[0], c.L, c.L.shape[0], c.seed, c.begin, c.begin + c.trials)
    assert raw_call(*args, result, hist, codeword, mask) == 0
    assert np.array_equal(result, want["result"]) and np.array_equal(hist - 1000, want["hist"])
    assert np.array_equal(codeword, want["codeword"]) and int(mask[0]) == want["logical_mask"]
    # codeword and logical_mask may each be NULL
    for with_codeword, with_mask in ((False, True), (True, False), (False, False)):
        result, hist, codeword, mask = poisoned(c.n)
        assert raw_call(*args, result, hist, codeword if with_codeword else None, mask if with_mask else None) == 0
        assert np.array_equal(result, want["result"]) and np.array_equal(hist - 1000, want["hist"])
        assert np.array_equal(codeword, want["codeword"]) if with_codeword else np.all(codeword == SENTINEL)
        assert int(mask[0]) == (want["logical_mask"] if with_mask else 0xDEADBEEFDEADBEEF)
    # an empty range succeeds and sets result alone
    result, hist, codeword, mask = poisoned(c.n)
    assert raw_call(dec, c.G, c.G.shape[0], c.L, c.L.shape[0], c.seed, 9, 9, result, hist, codeword, mask) == 0
    assert result.tolist() == [0, -1, -1, -1] and np.all(hist == 1000) and np.all(codeword == SENTINEL)


def test_more_trials_than_one_pass_of_the_grid_and_other_grids():
    c, want = dc.case("passes"), dc.statement("passes")
    dec = fresh(c.H)
    grids = set()
    for per_cu in (1, 0, 3):
        dec.set_option(_lib.OPT_BLOCKS_PER_CU, per_cu)
        check_against_statement(c, want, dec.distance_search(c.G, c.L, c.begin, c.begin + c.trials, seed=c.seed))
        grids.add(dec.info("grid"))
        if per_cu == 1:
            assert dec.info("grid") == dec.info("num_cu") < c.trials        # a second pass, and a partial third
    assert len(grids) >= 2


@pytest.mark.parametrize("name", ["72z", "rand37"])
def test_independent_of_the_split_of_the_range(name):
    c, want = dc.case(name), dc.statement(name)
    dec = bp.decoder_for(c.H)
    end = c.begin + c.trials
    for cuts in ((c.begin + 1,), (c.begin + 20, c.begin + 21, c.begin + 37)):
        edges = (c.begin,) + cuts + (end,)
        hist = np.zeros(c.n + 1, np.int64)
        best, trials = None, 0
        for a, b in zip(edges[:-1], edges[1:]):
            result, _, codeword, mask = dec.distance_search(c.G, c.L, a, b, seed=c.seed, hist=hist)
            trials += int(result[0])
            if result[1] >= 0 and (best is None or (result[1], result[2]) < (best[0][1], best[0][2])):
                best = (result, codeword, mask)
        assert trials == c.trials and np.array_equal(hist, want["hist"])
        assert np.array_equal(best[0][1:], want["result"][1:]) and np.array_equal(best[1], want["codeword"])
        assert best[2] == want["logical_mask"]


def test_independent_of_the_callers_stream():
    import torch
    c, want = dc.case("72x"), dc.statement("72x")
    dec = bp.decoder_for(c.H)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.ones(1 << 22, device="cuda") * 3.0                 # work in flight on the caller's stream
        got = dec.distance_search(c.G, c.L, c.begin, c.begin + c.trials, seed=c.seed)
    check_against_statement(c, want, got)
    side.synchronize()
    assert float(busy[-1]) == 3.0


def test_another_G_on_the_same_handle_then_decode_batch():
    c, want = dc.case("72x"), dc.statement("72x")
    d, want_d = dc.case("dup"), dc.statement("dup")
    dec = fresh(c.H)
    check_against_statement(c, want, dec.distance_search(c.G, c.L, c.begin, c.begin + c.trials, seed=c.seed))
    check_against_statement(d, want_d, dec.distance_search(d.G, d.L, d.begin, d.begin + d.trials, seed=d.seed))
    # a second handle, with another matrix, between them
    s = dc.case("steane")
    check_against_statement(s, dc.statement("steane"),
                            fresh(s.H).distance_search(s.G, s.L, s.begin, s.begin + s.trials, seed=s.seed))
    check_against_statement(c, want, dec.distance_search(c.G, c.L, c.begin, c.begin + c.trials, seed=c.seed))
    # the next call on the handle is qbp_decode_batch, and it is still bit-exact
    rng = np.random.default_rng(3)
    errors = (rng.random((32, c.n)) < 0.04).astype(np.uint8)
    syn = (errors.astype(np.int64) @ c.H.T.astype(np.int64) % 2).astype(np.uint8)
    prior = mc.prior_of(0.04, c.n)
    hard, conv, iters, llr = dec.decode(syn, prior, 50)
    o_hard, o_conv, o_iters, _ = oracle.decode_batch(c.H, syn, prior, 50)
    assert np.array_equal(hard, o_hard) and np.array_equal(conv, o_conv) and np.array_equal(iters, o_iters)


def test_refusals_are_host_only_and_leave_the_outputs():
    c = dc.case("72x")
    dec = fresh(c.H)
    r, k = c.G.shape[0], c.L.shape[0]
    bad_row = c.G.copy()
    bad_row[r - 1, 0] ^= 1                                # weight-1 change: outside ker H (no zero column in H)
    big_G = np.zeros((2049, c.n), np.uint8)
    cases = [
        ("r = 2049", _lib.E_UNSUPPORTED, dict(G=big_G, r=2049)),
        ("a row outside ker H", _lib.E_INVALID, dict(G=bad_row)),
        ("k = 0", _lib.E_INVALID, dict(k=0)),
        ("k = 65", _lib.E_INVALID, dict(L=np.zeros((65, c.n), np.uint8), k=65)),
        ("r = 0", _lib.E_INVALID, dict(r=0)),
        ("null G", _lib.E_INVALID, dict(G=None)),
        ("null L", _lib.E_INVALID, dict(L=None)),
        ("null result", _lib.E_INVALID, dict(result=None)),
        ("null hist", _lib.E_INVALID, dict(hist=None)),
        ("end < begin", _lib.E_INVALID, dict(begin=5, end=4)),
    ]
    launches = (dec.info("threads"), dec.info("grid"), dec.info("lds_bytes"))
    for what, code, change in cases:
        result, hist, codeword, mask = poisoned(c.n)
        kw = dict(G=c.G, r=r, L=c.L, k=k, seed=1, begin=0, end=4, result=result, hist=hist, codeword=codeword, mask=mask)
        kw.update(change)
        rc = raw_call(dec, kw["G"], kw["r"], kw["L"], kw["k"], kw["seed"], kw["begin"], kw["end"], kw["result"], kw["hist"],
                      kw["codeword"], kw["mask"])
        assert rc == code, (what, rc, _lib.load().qbp_last_error())
        assert np.all(result == -77) and np.all(hist == 1000) and np.all(codeword == SENTINEL), what
        assert mask[0] == 0xDEADBEEFDEADBEEF, what
    assert launches == (dec.info("threads"), dec.info("grid"), dec.info("lds_bytes"))      # no launch was recorded
    # a null handle
    result, hist, codeword, mask = poisoned(c.n)
    assert _lib.load().qbp_distance_search(None, c.G.ctypes.data, r, c.L.ctypes.data, k, 0, 0, 4, result.ctypes.data,
                                           hist.ctypes.data, None, None) == _lib.E_INVALID
    # the Python binding raises, with the code
    with pytest.raises(_lib.QbpError) as e:
        dec.distance_search(bad_row, c.L, 0, 4)
    assert e.value.code == _lib.E_INVALID and "ker H" in str(e.value)


def test_a_state_beyond_160_KiB_is_refused():
    """n = 8192: W = 256, a row of 257 words; 200 rows are 205 600 bytes of LDS.  One check on two columns, so that
    every G row below lies in ker H."""
    n, r = 8192, 200
    H = np.zeros((1, n), np.uint8)
    H[0, :2] = 1
    dec = fresh(H)
    G = np.zeros((r, n), np.uint8)
    G[np.arange(r), 2 + np.arange(r)] = 1
    L = np.ones((1, n), np.uint8)
    result, hist, codeword, mask = poisoned(n)
    assert raw_call(dec, G, r, L, 1, 0, 0, 4, result, hist, codeword, mask) == _lib.E_UNSUPPORTED
    assert b"160 KiB" in _lib.load().qbp_last_error()
    assert np.all(result == -77) and np.all(hist == 1000) and np.all(codeword == SENTINEL)
    # 100 rows fit (102 800 bytes); every row is a weight-1 vector L detects
    result, hist, codeword, mask = dec.distance_search(G[:100], L, 0, 2)
    assert result[:2].tolist() == [2, 1] and hist[1] == 2 and codeword.sum() == 1 and mask == 1
    assert dec.info("lds_bytes") == ((max(8 * 8192, 4 * 100 * 257) + 2 * 8192 + 15) & ~15)


def test_bound_and_estimate_on_the_shipped_codes():
    c = dc.case("72x")
    code = codes.load_code("[[72, 12, 6]]")
    want = dc.statement("72x")
    out = distance.bound(code.Hx, code.Lx, trials=c.trials, seed=0)
    assert out["weight"] == want["result"][1] == 6 and out["trial"] == want["result"][2] and out["trials"] == c.trials
    assert np.array_equal(out["hist"], want["hist"]) and np.array_equal(out["codeword"], want["codeword"])
    assert out["logical"] == want["logical_mask"]
    # shards merge by (weight, trial), in any order
    shards = [distance.bound(code.Hx, code.Lx, trials=c.trials, seed=0, rank=r, world=3) for r in range(3)]
    merged = distance.merge(shards[2], distance.merge(shards[0], shards[1]))
    assert merged["weight"] == out["weight"] and merged["trial"] == out["trial"] and merged["trials"] == c.trials
    assert np.array_equal(merged["hist"], out["hist"]) and np.array_equal(merged["codeword"], out["codeword"])
    est = distance.estimate(code, trials=64)
    assert est["distance"] == 6 and est["x"]["weight"] == 6 and est["z"]["weight"] == 6 and code.distance == 6
    # a detector error model: the phenomenological model of Steane over 2 rounds
    from qldpc_amd import dem
    steane = codes.from_matrices(codes.STEANE_H, codes.STEANE_H, "test_gpu_distance steane")
    H, L, _ = dem.phenomenological(steane, 2, 0.01)
    out = distance.bound(H, L, trials=64)
    Hd = np.asarray(H.toarray() if hasattr(H, "toarray") else H).astype(np.int64)
    want = do.search(gf2.nullspace(Hd), L, 0, 0, 64)
    assert out["weight"] == want["result"][1] > 0 and np.array_equal(out["codeword"], want["codeword"])
    assert np.array_equal(out["hist"], want["hist"]) and out["trial"] == want["result"][2]
    assert not (Hd @ out["codeword"] % 2).any() and (np.asarray(L).astype(np.int64) @ out["codeword"] % 2).any()


def test_end_to_end_on_a_code_the_project_has_never_seen():
    """codes.bb_code on Z_6 x Z_6 with A = x + y^2 + y^3, B = y + x^2 + x^3 (k = 4; none of the shipped pairs) ->
    register -> distance.estimate -> mc.run_sweep with OSD: the counters are those of qbp_mc_run_errors on the same
    sampled errors with the computed Lx and distance."""
    name = "test_gpu_distance bb 6x6"
    code = codes.register(codes.bb_code(6, 6, [(1, 0), (0, 2), (0, 3)], [(0, 1), (2, 0), (3, 0)], name=name))
    assert code.Lx.shape == (4, 72) and code.distance is None
    assert all(not np.array_equal(code.Hx, codes.load_code(n).Hx) for n in codes.code_names() if codes.load_code(n).n == 72)
    with pytest.raises(ValueError, match="distance.estimate"):
        mc.run_sweep(name, [0.05], 100, osd=True)
    est = distance.estimate(name, trials=256)
    d = est["distance"]
    assert codes.load_code(name).distance == d == min(est["x"]["weight"], est["z"]["weight"]) and d >= 2
    for side, H, L in (("x", code.Hx, code.Lx), ("z", code.Hz, code.Lz)):
        cw = est[side]["codeword"]
        assert cw.sum() == est[side]["weight"] and not (H @ cw % 2).any() and (L.astype(np.int64) @ cw % 2).any()
        want = do.search(gf2.nullspace(H), L, 0, 0, 256)
        assert est[side]["weight"] == want["result"][1] and np.array_equal(est[side]["hist"], want["hist"])
    p, T = 0.05, 20000
    table = mc.run_sweep(name, [p], T, osd=True)
    dec = bp.decoder_for(code.Hx)
    errors = dec.mc_sample_errors(p, 0, T)
    want = dec.mc_run_errors(code.Lx, d, errors, mc.prior_of(p, code.n), flags=_lib.FLAG_OSD0)
    assert np.array_equal(table[0], want) and want[0] == T and want[1] > 0
