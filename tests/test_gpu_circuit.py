"""GPU Pauli-frame simulator (qbp_frame_*), circuit_dem and mc.run_circuit against tests/circuit_oracle.py, bit for
bit, into poisoned buffers, with the padding bits asserted zero."""
import ctypes as C

import numpy as np
import pytest

import circuit_cases as cc
import circuit_oracle as co
from qldpc_amd import _lib, bp, circuit, mc
from qldpc_amd import dem as dem_mod

pytestmark = pytest.mark.gpu
POISON = 0xA5
RATES = [0.01, 0.004, 0.002, 0.02]          # reset, cnot, idle, meas: all different


def torch_buffers(T, m):
    import torch
    dev = torch.device("cuda", bp.DEVICE)
    rb = (m + 7) // 8
    return (torch.full((T + 1, max(rb, 1)), POISON, dtype=torch.uint8, device=dev),
            torch.full((T + 1,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev))


def device_rows(sim, T, call):
    """Run ``call(d_det, d_obs, stream)`` into poisoned device buffers one row longer than T; the rows, after the
    guard row is found untouched."""
    import torch
    d_det, d_obs = torch_buffers(T, sim.m)
    call(d_det.data_ptr(), d_obs.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    det, obs = d_det.cpu().numpy(), d_obs.cpu().numpy().view(np.uint64)
    assert (det[T] == POISON).all() and obs[T] == np.uint64(0xA5A5A5A5A5A5A5A5)
    return det[:T, :(sim.m + 7) // 8], obs[:T]


def assert_rows(got, want_det, want_obs, m):
    bits, masks = co.pack(want_det, want_obs)
    assert np.array_equal(got[0], bits)
    assert np.array_equal(got[1], masks)
    if m % 8:
        assert not (got[0][:, -1] >> (m % 8)).any()          # padding bits


ENUM_CASES = [("422", 2, "Z", "basis"), ("422", 2, "X", "all"), ("steane", 2, "Z", "basis"), ("72", 2, "Z", "basis"),
              ("72", 2, "Z", "all"), ("hgp", 1, "Z", "basis"), ("hgp", 1, "X", "all")]


@pytest.mark.parametrize("key", ENUM_CASES + ["reset"], ids=str)
def test_every_fault(key):
    cir = cc.reset_circuit() if key == "reset" else cc.memory(*key)
    det, obs, _, _ = cc.fault_rows(key)
    sim = cir.simulator(bp.DEVICE)
    F, m = cir.n_faults, len(cir.detectors)
    assert sim.info("faults") == F and sim.info("sites") == cir.n_sites and sim.info("records") == cir.n_records
    got = device_rows(sim, F, lambda d, o, s: sim.faults_device(0, F, d, o, stream=s))
    assert_rows(got, det, obs, m)
    host = sim.faults(0, F)
    assert np.array_equal(host[0], got[0]) and np.array_equal(host[1], got[1])


def test_partial_byte_and_odd_count():
    """What test_every_fault covers: m = 3 is a partial byte, and 23 faults are no multiple of 32."""
    assert len(cc.memory("422", 2).detectors) == 3 and cc.reset_circuit().n_faults == 23


@pytest.mark.parametrize("begin", [0, 1, 31, 33])
def test_fault_begin(begin):
    key = ("steane", 2, "Z", "basis")
    cir = cc.memory(*key)
    det, obs, _, _ = cc.fault_rows(key)
    sim = cir.simulator(bp.DEVICE)
    T = 101                                                   # no multiple of 32
    got = device_rows(sim, T, lambda d, o, s: sim.faults_device(begin, T, d, o, stream=s))
    assert_rows(got, det[begin:begin + T], obs[begin:begin + T], len(cir.detectors))


def test_fault_range_splits_agree():
    key = ("72", 2, "Z", "all")
    cir = cc.memory(*key)
    _, _, bits, masks = cc.fault_rows(key)
    sim = cir.simulator(bp.DEVICE)
    for cuts in ([0, 777, 5000], [0, 33, 2049, 4100, 5000]):
        parts = [sim.faults(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), bits[:5000])
        assert np.array_equal(np.concatenate([p[1] for p in parts]), masks[:5000])


def test_dem_of_a_circuit():
    key = ("72", 2, "Z", "basis")
    cir = cc.memory(*key)
    det, obs, _, _ = cc.fault_rows(key)
    H, L, col = co.merge(det, obs)
    d = circuit.circuit_dem(cir, device=bp.DEVICE)
    assert np.array_equal(d.H.toarray(), H) and np.array_equal(d.L, L) and np.array_equal(d.fault_column, col)
    assert d.counts.sum() == (col >= 0).sum()
    H2, L2, p2 = dem_mod.parse_dem(d.to_text(RATES))
    assert np.array_equal(H2.toarray(), H) and np.array_equal(L2, L)
    assert np.allclose(p2, d.probs(RATES), rtol=1e-15, atol=0)


SAMPLE_KEY = ("steane", 2, "Z", "all")


@pytest.mark.parametrize("T", [1, 31, 32, 33, 2049])
@pytest.mark.parametrize("begin", [0, 5, 2 ** 32 - 3])
def test_sampled_shots(T, begin):
    cir = cc.memory(*SAMPLE_KEY)
    sim = cir.simulator(bp.DEVICE)
    seed = (1 << 40) + 12345                                   # above 2^32
    want = co.sample(cir, RATES, seed, begin, T)
    got = device_rows(sim, T, lambda d, o, s: sim.sample_device(RATES, T, d, o, seed=seed, shot_begin=begin, stream=s))
    assert_rows(got, *want, len(cir.detectors))
    assert T < 2049 or (want[0].any() and want[1].any())       # (the case is not trivial)
    host = sim.sample(RATES, T, seed=seed, shot_begin=begin)
    assert np.array_equal(host[0], got[0]) and np.array_equal(host[1], got[1])


def test_rates_zero_and_half():
    """One class at 0, one at 0.5: many faults per shot, every code of a pair site."""
    cir = cc.memory("72", 2)
    sim = cir.simulator(bp.DEVICE)
    rates = [0.0, 0.5, 0.03, 0.2]
    want = co.sample(cir, rates, 9, 7, 300)
    got = device_rows(sim, 300, lambda d, o, s: sim.sample_device(rates, 300, d, o, seed=9, shot_begin=7, stream=s))
    assert_rows(got, *want, len(cir.detectors))
    hits = co.sample_faults(cir, np.asarray(rates), 9, 7, 300)
    sites, _ = co.sites_of(cir)
    codes_seen = set(np.concatenate([h[1] for h, s in zip(hits, sites) if s[0] == "DEP2"]).tolist())
    assert codes_seen == set(range(1, 16))
    assert all(len(h[0]) == 0 for h, s in zip(hits, sites) if s[3] == 0)


def test_reset_circuit_sampled_with_five_classes():
    cir = cc.reset_circuit()
    sim = cir.simulator(bp.DEVICE)
    rates = [0.3, 0.25, 0.2, 0.4, 0.35]
    want = co.sample(cir, rates, 3, 0, 1000)
    assert_rows(sim.sample(rates, 1000, seed=3), *want, len(cir.detectors))


def test_more_records_than_one_chunk_and_handle_reuse():
    """QBP_FRAME_OPT_CHUNK_LANES 64: 2048 records a chunk.  A smaller T, then a larger one, on one handle; the rows do
    not depend on the chunk."""
    cir = cc.memory(*SAMPLE_KEY)
    sim = _lib.FrameSim(cir.nq, cir.table(), *cir._csr(cir.detectors, "d"), *cir._csr(cir.observables, "o"), device=bp.DEVICE)
    ref = cir.simulator(bp.DEVICE)
    sim.set_option(_lib.FRAME_OPT_CHUNK_LANES, 64)
    assert sim.info("chunk_lanes") == 64
    for T in (100, 5000, 70):
        got = sim.sample(RATES, T, seed=4, shot_begin=11)
        assert sim.info("chunks") == (T + 2047) // 2048
        want = ref.sample(RATES, T, seed=4, shot_begin=11)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert_rows(got, *co.sample(cir, RATES, 4, 11, 70), len(cir.detectors))
    key = ("72", 2, "Z", "all")                               # 21 168 faults: 11 chunks
    big = cc.memory(*key)
    sim = _lib.FrameSim(big.nq, big.table(), *big._csr(big.detectors, "d"), *big._csr(big.observables, "o"), device=bp.DEVICE)
    sim.set_option(_lib.FRAME_OPT_CHUNK_LANES, 64)
    F = big.n_faults
    got = sim.faults(0, F)
    assert sim.info("chunks") == (F + 2047) // 2048 > 1
    assert np.array_equal(got[0], cc.fault_rows(key)[2]) and np.array_equal(got[1], cc.fault_rows(key)[3])


def test_more_items_than_one_pass_of_the_assemble_grid():
    """frame_assemble_kernel strides over its items with a grid of at most 16 workgroups of 256 per CU.  70 000 shots of
    [[72,12,6]] over 2 rounds, "all" (18 bytes a row): 1 330 000 items in ONE chunk, more than one pass; the same shots
    through 64-lane chunks are 38 912 items a launch, one pass each.  Equal rows, and the last 1500 shots -- items of
    the second pass -- against the oracle."""
    import torch
    cir = cc.memory("72", 2, "Z", "all")
    T, m = 70000, len(cir.detectors)
    per_pass = 16 * torch.cuda.get_device_properties(bp.DEVICE).multi_processor_count * 256
    assert T * ((m + 7) // 8) + T > per_pass and 2048 * ((m + 7) // 8) + 2048 <= per_pass
    sim = cir.simulator(bp.DEVICE)
    got = device_rows(sim, T, lambda d, o, s: sim.sample_device(RATES, T, d, o, seed=8, shot_begin=3, stream=s))
    assert sim.info("chunks") == 1
    small = _lib.FrameSim(cir.nq, cir.table(), *cir._csr(cir.detectors, "d"), *cir._csr(cir.observables, "o"), device=bp.DEVICE)
    small.set_option(_lib.FRAME_OPT_CHUNK_LANES, 64)
    want = small.sample(RATES, T, seed=8, shot_begin=3)
    assert small.info("chunks") == (T + 2047) // 2048
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    tail = co.sample(cir, RATES, 8, 3 + T - 1500, 1500)
    assert_rows((got[0][-1500:], got[1][-1500:]), *tail, m)
    only_obs = sim.sample(RATES, T, seed=8, shot_begin=3, want_det=False)          # the items are the masks alone
    assert np.array_equal(only_obs[1], got[1])


def test_own_stream_and_null_outputs():
    import torch
    cir = cc.memory(*SAMPLE_KEY)
    sim = cir.simulator(bp.DEVICE)
    T = 500
    want = sim.sample(RATES, T, seed=2)
    stream = torch.cuda.Stream()
    d_det, d_obs = torch_buffers(T, sim.m)
    with torch.cuda.stream(stream):
        sim.sample_device(RATES, T, d_det.data_ptr(), 0, seed=2, stream=stream.cuda_stream)
        sim.sample_device(RATES, T, 0, d_obs.data_ptr(), seed=2, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_det.cpu().numpy()[:T], want[0]) and (d_det.cpu().numpy()[T] == POISON).all()
    assert np.array_equal(d_obs.cpu().numpy().view(np.uint64)[:T], want[1])
    only_det = sim.sample(RATES, T, seed=2, want_obs=False)
    only_obs = sim.faults(0, 64, want_det=False)
    assert only_det[1] is None and np.array_equal(only_det[0], want[0])
    assert only_obs[0] is None and np.array_equal(only_obs[1], cc.fault_rows(SAMPLE_KEY)[3][:64])


def test_circuit_sample_matches_the_simulator():
    cir = cc.memory(*SAMPLE_KEY)
    a = cir.sample(200, dict(reset=0.01, cnot=0.004, idle=0.002, meas=0.02), seed=5, device=bp.DEVICE)
    assert_rows(a, *co.sample(cir, RATES, 5, 0, 200), len(cir.detectors))


# ---- pipeline -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bp", "osd0", "minsum"])
def test_run_circuit_equals_run_shots_on_sampled_arrays(mode):
    kw = dict(max_iter=20)
    if mode == "osd0":
        kw.update(osd=True)
    if mode == "minsum":
        kw.update(variant=_lib.MIN_SUM, alpha=0.8)
    p, shots = 0.01, 3000
    cir = cc.memory("72", 2)
    table = mc.run_circuit(cc.code("72"), 2, [p], shots, seed=6, device=bp.DEVICE, **kw)
    d = circuit.circuit_dem(cir, device=bp.DEVICE)
    det, masks = cir.sample(shots, p, seed=6, device=bp.DEVICE)
    cnt, _, _ = mc.run_shots(d.H, d.L, det, masks, prior=mc.dem_prior(d.probs(p)), device=bp.DEVICE, **kw)
    assert np.array_equal(table[0], cnt) and cnt[0] == shots and 0 < cnt[1] < shots
    chunked = mc.run_circuit(cc.code("72"), 2, [p], shots, seed=6, device=bp.DEVICE, chunk=700, **kw)
    halves = sum(mc.run_circuit(cc.code("72"), 2, [p], shots, seed=6, device=bp.DEVICE, rank=r, world=2, reduce=False, **kw)
                 for r in range(2))
    assert np.array_equal(chunked, table) and np.array_equal(halves, table)


def test_ler_of_sampled_circuit_agrees_with_its_dem():
    """[[72,12,6]] over 3 rounds, p = 0.004, 2e5 shots, BP(50) + OSD-0: run_circuit's LER against run_dem on
    (H, L, probs), within 5 sigma of the two binomial errors combined."""
    p, shots = 0.004, 200000
    table = mc.run_circuit(cc.code("72"), 3, [p], shots, seed=1, osd=True, device=bp.DEVICE)
    d = circuit.circuit_dem(cc.memory("72", 3), device=bp.DEVICE)
    cnt = mc.run_dem(d.H, d.L, d.probs(p), shots, seed=1, osd=True, device=bp.DEVICE)
    a, b = table[0][1] / shots, cnt[1] / shots
    sigma = np.sqrt(a * (1 - a) / shots + b * (1 - b) / shots)
    print(f"LER circuit {a:.6f}  dem {b:.6f}  sigma {sigma:.6f}  difference {abs(a - b) / sigma:.2f} sigma")
    assert table[0][0] == shots and cnt[0] == shots
    assert abs(a - b) <= 5 * sigma


# ---- refusals -----------------------------------------------------------------------------------------------------
def _create(nq, ops, det=((0,),), obs=((0,),), k=None):
    ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 4)
    dp = np.concatenate([[0], np.cumsum([len(x) for x in det])]).astype(np.int32)
    di = np.asarray([i for x in det for i in x], np.int32)
    op = np.concatenate([[0], np.cumsum([len(x) for x in obs])]).astype(np.int32)
    oi = np.asarray([i for x in obs for i in x], np.int32)
    h = C.c_void_p()
    rc = _lib.load().qbp_frame_create(nq, ops.ctypes.data, ops.shape[0], dp.ctypes.data, di.ctypes.data, len(det),
                                      op.ctypes.data, oi.ctypes.data, len(obs) if k is None else k, bp.DEVICE, C.byref(h))
    return rc, h


GOOD = [(3, 0, 0, 0), (5, 0, 0, 0), (2, 0, 1, 0), (8, 0, 1, 1), (3, 1, 0, 0)]       # MZ 0, XERR 0, CX 0 1, DEP2 0 1, MZ 1


@pytest.mark.parametrize("what, args", [
    ("target >= nq", dict(ops=GOOD[:2] + [(3, 2, 0, 0)])),
    ("negative target", dict(ops=[(3, -1, 0, 0)])),
    ("CX second target >= nq", dict(ops=GOOD[:1] + [(2, 0, 2, 0)])),
    ("CX equal qubits", dict(ops=GOOD[:1] + [(2, 1, 1, 0)])),
    ("DEP2 equal qubits", dict(ops=GOOD[:1] + [(8, 0, 0, 0)])),
    ("kind", dict(ops=GOOD[:1] + [(9, 0, 0, 0)])),
    ("rate class", dict(ops=GOOD[:1] + [(5, 0, 0, 16)])),
    ("detector record", dict(ops=GOOD, det=((0, 2),))),
    ("negative record", dict(ops=GOOD, det=((-1,),))),
    ("observable record", dict(ops=GOOD, obs=((2,),))),
    ("k > 64", dict(ops=GOOD, obs=((0,),) * 65)),
    ("nq", dict(ops=GOOD, nq=0)),
])
def test_create_refusals(what, args):
    rc, h = _create(args.pop("nq", 2), **args)
    assert rc == _lib.E_INVALID and not h.value, what


def test_create_null_arguments():
    lib = _lib.load()
    ops = np.asarray(GOOD, np.int32)
    ptr = np.asarray([0, 1], np.int32)
    idx = np.asarray([0], np.int32)
    h = C.c_void_p()
    full = [2, ops.ctypes.data, 5, ptr.ctypes.data, idx.ctypes.data, 1, ptr.ctypes.data, idx.ctypes.data, 1, bp.DEVICE]
    for null in (1, 3, 4, 6, 7):
        a = list(full)
        a[null] = None
        assert lib.qbp_frame_create(*a, C.byref(h)) == _lib.E_INVALID and not h.value
    assert lib.qbp_frame_create(*full, None) == _lib.E_INVALID
    assert lib.qbp_frame_create(*full, C.byref(h)) == 0 and h.value
    lib.qbp_frame_destroy(h)


def test_call_refusals_leave_outputs_untouched():
    lib = _lib.load()
    cir = cc.reset_circuit()
    sim = cir.simulator(bp.DEVICE)
    F = cir.n_faults
    det = np.full((4, 1), POISON, np.uint8)
    obs = np.full(4, 0xA5A5A5A5A5A5A5A5, np.uint64)
    good = np.asarray([0.1] * 5)

    def sample(h, rates, n, begin, T):
        r = None if rates is None else np.ascontiguousarray(rates, np.float64)
        return lib.qbp_frame_sample(h, None if r is None else r.ctypes.data, n, 1, begin, T, det.ctypes.data,
                                    obs.ctypes.data)
    bad = [sample(None, good, 5, 0, 4), sample(sim._h, None, 5, 0, 4), sample(sim._h, good, 4, 0, 4),
           sample(sim._h, good, 5, 0, -1), sample(sim._h, good, 5, -1, 4), sample(sim._h, good, 5, 2 ** 63 - 2, 4),
           sample(sim._h, [0.1, 1.0, 0.1, 0.1, 0.1], 5, 0, 4), sample(sim._h, [0.1, np.nan, 0.1, 0.1, 0.1], 5, 0, 4),
           sample(sim._h, [0.1, -0.1, 0.1, 0.1, 0.1], 5, 0, 4),
           lib.qbp_frame_faults(None, 0, 4, det.ctypes.data, obs.ctypes.data),
           lib.qbp_frame_faults(sim._h, -1, 4, det.ctypes.data, obs.ctypes.data),
           lib.qbp_frame_faults(sim._h, F - 3, 4, det.ctypes.data, obs.ctypes.data),
           lib.qbp_frame_faults(sim._h, 0, -1, det.ctypes.data, obs.ctypes.data),
           lib.qbp_frame_faults_device(sim._h, F, 1, None, None, None),
           lib.qbp_frame_sample_device(sim._h, good.ctypes.data, 5, 1, 0, -1, None, None, None)]
    assert bad == [_lib.E_INVALID] * len(bad)
    assert sample(sim._h, good, 5, 0, 0) == 0 and lib.qbp_frame_faults(sim._h, F, 0, det.ctypes.data, obs.ctypes.data) == 0
    assert (det == POISON).all() and (obs == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    assert lib.qbp_frame_set_option(sim._h, 99, 1) == _lib.E_INVALID
    assert lib.qbp_frame_set_option(sim._h, _lib.FRAME_OPT_CHUNK_LANES, -1) == _lib.E_INVALID
    assert lib.qbp_frame_get_info(None, 0) == -1
    with pytest.raises(ValueError):
        cir.sample(4, 1.0)
    with pytest.raises(ValueError):
        mc.run_circuit("steane", 2, [0.01], 10)               # no logicals
