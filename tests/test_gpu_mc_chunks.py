"""GPU: the chunking of the Monte-Carlo drivers' shared device loop does not change a table.  Every driver is run
twice on [[72, 12, 6]] -- as it is (one launch per point here), and with ``Decoder.mc_osd_step`` patched to 37, which
neither divides the trial counts nor is a multiple of 64 -- and the tables are compared digit for digit: errors are
keyed by the global trial index and counters are additive, so no tolerance is involved."""
import numpy as np
import pytest

from qldpc_amd import _lib, bp, codes, dem, mc

pytestmark = pytest.mark.gpu
CODE, P, TRIALS, STEP = "[[72, 12, 6]]", 0.05, 1000, 37


def _dem(**kw):
    H, L, probs = dem.phenomenological(CODE, 2, 0.01)
    return mc.run_dem(H, L, probs, TRIALS, **kw)


DRIVERS = {
    "sweep": lambda **kw: mc.run_sweep(CODE, [P, 0.03], TRIALS, osd=True, **kw),
    "sweep_lsd": lambda **kw: mc.run_sweep(CODE, [P, 0.03], TRIALS, lsd=0, **kw),        # a record stage other than OSD
    "dem": lambda **kw: _dem(osd=True, **kw),
    "budgets": lambda **kw: mc.run_budgets(CODE, P, TRIALS, [5, 10, 20], osd=True, **kw),     # 37 // 3: steps of 12
    "spectrum": lambda **kw: mc.run_spectrum(CODE, [P, 0.03], TRIALS, osd=True, **kw),        # (three arrays)
    "weights": lambda **kw: mc.run_weights(CODE, [3, 5], TRIALS, prior_p=P, osd=True, **kw),
    # 72 and 2556 patterns: a range per point, and a last chunk of 2556 - 69 * 37 = 3 patterns
    "enumerate": lambda **kw: mc.run_enumerate(CODE, [1, 2], prior_p=P, osd=True, **kw),
    "circuit": lambda **kw: mc.run_circuit(CODE, 2, [P], TRIALS, osd=True, **kw),
}


def _arrays(result):
    return result if isinstance(result, tuple) else (result,)


@pytest.mark.parametrize("name", list(DRIVERS))
def test_a_table_does_not_depend_on_the_step(name, monkeypatch):
    run = DRIVERS[name]
    whole = _arrays(run(device=bp.DEVICE))
    assert int(whole[0].sum()) > 0                 # (the counters: an empty table would compare equal too)
    with monkeypatch.context() as mp:
        mp.setattr(_lib.Decoder, "mc_osd_step", lambda self: STEP)
        assert bp.decoder_for(codes.load_code(CODE).Hx, device=bp.DEVICE).mc_step(_lib.FLAG_OSD0, TRIALS) == STEP
        chunked = _arrays(run(device=bp.DEVICE))
    assert len(chunked) == len(whole)
    for a, b in zip(chunked, whole):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_run_circuit_does_not_depend_on_its_chunk():
    whole = mc.run_circuit(CODE, 2, [P], TRIALS, osd=True, device=bp.DEVICE, chunk=None)
    chunked = mc.run_circuit(CODE, 2, [P], TRIALS, osd=True, device=bp.DEVICE, chunk=STEP)
    assert whole[0][0] == TRIALS and np.array_equal(chunked, whole)
