"""CPU: bit packing and sample files of recorded shots (qldpc_amd/shots.py), the sharding and argument checks of
mc.run_shots with an injected runner, and the new entry points' prototypes."""
import os
import re

import numpy as np
import pytest

from qldpc_amd import _lib, dem, mc, shots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("m", [3, 8, 36, 865])
def test_pack_unpack_round_trip(m):
    rng = np.random.default_rng(m)
    a = rng.integers(0, 2, size=(23, m), dtype=np.uint8)
    a[0] = 0
    a[1] = 1
    p = shots.pack_bits(a)
    assert p.dtype == np.uint8 and p.shape == (23, (m + 7) // 8)
    # stim's b8: detector c is bit c % 8 of byte c // 8
    for c in (0, 1, m // 2, m - 1):
        assert np.array_equal((p[:, c // 8] >> (c % 8)) & 1, a[:, c])
    if m % 8:
        assert not (p[:, -1] >> (m % 8)).any()                       # padding bits are zero ...
    assert np.array_equal(shots.unpack_bits(p, m), a)
    dirty = p.copy()
    if m % 8:
        dirty[:, -1] |= 0xff << (m % 8) & 0xff                       # ... and ignored when set
    assert np.array_equal(shots.unpack_bits(dirty, m), a)
    assert np.array_equal(shots.pack_bits(a.astype(bool)), p)
    # any memory order in, C-contiguous rows out (the device reads the buffer as it lies)
    for other in (np.asfortranarray(a), a[::-1][::-1], np.hstack([a, a])[:, :m]):
        q = shots.pack_bits(other)
        assert q.flags.c_contiguous and q.tobytes() == p.tobytes()
    with pytest.raises(ValueError):
        shots.unpack_bits(p, m + 8)
    with pytest.raises(ValueError):
        shots.pack_bits(a + 1)


@pytest.mark.parametrize("k", [1, 12, 64])
def test_mask_round_trip(k):
    rng = np.random.default_rng(k)
    o = rng.integers(0, 2, size=(31, k), dtype=np.uint8)
    o[0] = 1
    mk = shots.masks_of(o)
    assert mk.dtype == np.uint64 and mk.shape == (31,)
    assert int(mk[0]) == (1 << k) - 1
    for l in (0, k - 1):
        assert np.array_equal((mk >> np.uint64(l)) & np.uint64(1), o[:, l])
    assert np.array_equal(shots.obs_of(mk, k), o)
    with pytest.raises(ValueError):
        shots.masks_of(np.zeros((2, 65), np.uint8))


@pytest.mark.parametrize("fmt", ["b8", "01"])
@pytest.mark.parametrize("m,k", [(3, 1), (36, 12), (865, 64)])
def test_read_shots(tmp_path, fmt, m, k):
    rng = np.random.default_rng(m + k)
    det = rng.integers(0, 2, size=(11, m), dtype=np.uint8)
    obs = rng.integers(0, 2, size=(11, k), dtype=np.uint8)
    f_det, f_obs, f_both = (str(tmp_path / name) for name in ("dets", "obs", "both"))
    shots.write_shots(f_det, det, fmt)
    shots.write_shots(f_obs, obs, fmt)
    shots.write_shots(f_both, np.hstack([det, obs]), fmt)
    if fmt == "b8":
        assert os.path.getsize(f_det) == 11 * ((m + 7) // 8) and os.path.getsize(f_both) == 11 * ((m + k + 7) // 8)
    else:
        assert open(f_det).read().split("\n")[0] == "".join(map(str, det[0]))
    d, mk = shots.read_shots(f_det, m, fmt=fmt)
    assert mk is None and np.array_equal(d, shots.pack_bits(det))
    d, mk = shots.read_shots(f_det, m, k, fmt, obs=f_obs)                 # observables in a file of their own
    assert np.array_equal(d, shots.pack_bits(det)) and np.array_equal(mk, shots.masks_of(obs))
    d, mk = shots.read_shots(f_both, m, k, fmt)                           # observables appended to every shot
    assert np.array_equal(d, shots.pack_bits(det)) and np.array_equal(mk, shots.masks_of(obs))
    # wrong lengths
    with open(f_det, "ab") as f:
        f.write(b"1")
    if fmt == "01" or (m + 7) // 8 > 1:                                   # (one-byte b8 rows: every length is whole)
        with pytest.raises(ValueError):
            shots.read_shots(f_det, m, fmt=fmt)
    shots.write_shots(f_obs, obs[:-1], fmt)
    shots.write_shots(f_det, det, fmt)
    with pytest.raises(ValueError):
        shots.read_shots(f_det, m, k, fmt, obs=f_obs)                     # shot counts differ
    if fmt == "01" or (m + 7) // 8 != (m + k + 7) // 8:
        with pytest.raises(ValueError):
            shots.read_shots(f_det, m, k, fmt)                            # no observables behind the shots
    with pytest.raises(ValueError):
        shots.read_shots(f_det, m, fmt="hex")
    with pytest.raises(ValueError):
        shots.read_shots(f_det, m, 65, fmt)


def test_read_shots_bad_character(tmp_path):
    f = tmp_path / "dets.01"
    f.write_text("0101\n01x1\n")
    with pytest.raises(ValueError):
        shots.read_shots(str(f), 4, fmt="01")


@pytest.fixture(scope="module")
def model():
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.01, 0.02)
    rng = np.random.default_rng(0)
    det = rng.integers(0, 2, size=(101, H.shape[0]), dtype=np.uint8)
    obs = rng.integers(0, 2, size=(101, L.shape[0]), dtype=np.uint8)
    return H, L, probs, det, obs


@pytest.mark.parametrize("world", [1, 2, 3])
def test_run_shots_sharding(model, world):
    H, L, probs, det, obs = model
    T = len(det)
    packed, masks = shots.pack_bits(det), shots.masks_of(obs)
    seen = np.zeros(T, np.int64)
    calls = []

    def runner(H_, L_, det_bits, actual, prior, begin, end):
        assert det_bits.dtype == np.uint8 and det_bits.shape == packed.shape and np.array_equal(det_bits, packed)
        assert actual.dtype == np.uint64 and np.array_equal(actual, masks)
        assert np.array_equal(prior, mc.dem_prior(probs))
        seen[begin:end] += 1
        calls.append((begin, end))
        cnt = np.zeros(12, np.int64)
        cnt[0] = end - begin
        cnt[1] = int((actual[begin:end] & np.uint64(1)).sum())
        return cnt, actual[begin:end] ^ np.uint64(5), np.arange(begin, end) % 2 == 0

    total = np.zeros(12, np.int64)
    preds = []
    for rank in range(world):
        # (an identity reduction: the per-rank tables are summed here)
        cnt, pred, conv = mc.run_shots(H, L, det if rank % 2 else packed, obs if rank % 2 else masks,
                                       prior=mc.dem_prior(probs), rank=rank, world=world, runner=runner,
                                       all_reduce=lambda t: t)
        b, e = mc.shard_range(T, rank, world)
        assert pred.dtype == np.uint64 and pred.shape == (e - b,) and conv.dtype == bool and conv.shape == (e - b,)
        total += cnt
        preds.append(pred)
    assert (seen == 1).all() and len(calls) == world
    assert total[0] == T and total[1] == int((masks & np.uint64(1)).sum())
    assert np.array_equal(np.concatenate(preds), masks ^ np.uint64(5))
    reduced = mc.run_shots(H, L, packed, None, prior=mc.dem_prior(probs), rank=0, world=world,
                           runner=lambda H_, L_, d, a, p, b, e: (np.ones(12, np.int64), np.zeros(e - b, np.uint64),
                                                                 np.zeros(e - b, bool)),
                           all_reduce=lambda t: t * world)
    assert (reduced[0] == world).all()


def test_run_shots_argument_errors_come_first(model):
    H, L, probs, det, obs = model
    n = H.shape[1]
    prior = mc.dem_prior(probs)

    def runner(*a):
        raise AssertionError("the runner must not be called")

    nan_prior = prior.copy()
    nan_prior[3] = np.nan
    bad = [
        dict(L=L[:, :-1]), dict(L=np.zeros((65, n), np.uint8)), dict(L=np.zeros((0, n), np.uint8)),
        dict(detections=det[:, :-1]), dict(detections=det[0]), dict(detections=shots.pack_bits(det)[:, :-1]),
        dict(observables=obs[:-1]), dict(observables=obs[:, :-1]), dict(observables=shots.masks_of(obs)[:-1]),
        dict(prior=prior[:-1]), dict(prior=nan_prior), dict(max_iter=0),
        dict(osd_order=3), dict(osd=True, osd_method="x"), dict(osd=True, osd_method="e", osd_order=13),
    ]
    for kw in bad:
        args = dict(L=L, detections=det, observables=obs, prior=prior)
        args.update(kw)
        Lm, d, o = args.pop("L"), args.pop("detections"), args.pop("observables")
        with pytest.raises(ValueError):
            mc.run_shots(H, Lm, d, o, runner=runner, **args)


def test_prototypes_and_header():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    for name, nargs in (("qbp_decode_shots", 16), ("qbp_decode_shots_device", 17)):
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
    assert callable(_lib.Decoder.decode_shots) and callable(_lib.Decoder.decode_shots_device)
    assert "counters[QBP_NUM_COUNTERS]" in re.search(r"\bint qbp_decode_shots\(([^;]*)\);", header).group(1)
