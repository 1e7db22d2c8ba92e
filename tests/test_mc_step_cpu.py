"""CPU: ``Decoder.mc_step``, the one statement of how many trials a Monte-Carlo or shot call may cover -- a share of
``mc_osd_step()`` when a flag makes the call keep per-trial records, the caller's whole range otherwise (no GPU: the
library is never loaded)."""
import pytest

from qldpc_amd import _lib

RECORDS = (_lib.FLAG_OSD0, _lib.FLAG_RELAY, _lib.FLAG_GD, _lib.FLAG_LSD)
SHAPES = ((36, 72), (2592, 7776), (100_000, 1_000_000))      # (one record step at the cap, one below it, one tiny)


def _decoder(m, n):
    dec = _lib.Decoder.__new__(_lib.Decoder)
    dec._h, dec.m, dec.n = None, m, n
    return dec


@pytest.mark.parametrize("m,n", SHAPES)
def test_record_flags_alone_and_combined_give_the_record_step(m, n):
    dec = _decoder(m, n)
    step = dec.mc_osd_step()
    assert step == max(1, min(_lib.MC_OSD_MAX_TRIALS, (8 << 30) // (m + 10 * n)))
    combined = [_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | (7 << _lib.OSD_ORDER_SHIFT), _lib.FLAG_OSD0 | _lib.FLAG_LAYERED,
                _lib.FLAG_RELAY | _lib.FLAG_QUANT, _lib.FLAG_LSD | _lib.FLAG_PAIRWISE_COLSUM,
                _lib.FLAG_OSD0 | _lib.FLAG_RELAY | _lib.FLAG_GD | _lib.FLAG_LSD]
    for flags in (*RECORDS, *combined):
        for whole in (0, 1, step - 1, step, 10 * step):
            assert dec.mc_step(flags, whole) == step, (flags, whole)


@pytest.mark.parametrize("m,n", SHAPES)
def test_a_ladder_divides_the_record_step_and_never_reaches_zero(m, n):
    dec = _decoder(m, n)
    step = dec.mc_osd_step()
    for flags in RECORDS:
        for K in (1, 2, 3, _lib.MC_MAX_BUDGETS, step, step + 1, 10 * step):
            assert dec.mc_step(flags, 10 ** 9, n_budgets=K) == max(1, step // K), (flags, K)
    assert dec.mc_step(_lib.FLAG_OSD0, 10 ** 9, n_budgets=10 * step) == 1
    for K in (1, 3, _lib.MC_MAX_BUDGETS, step + 1):
        assert dec.mc_budgets_step(K) == dec.mc_step(_lib.FLAG_OSD0, 0, K)


@pytest.mark.parametrize("m,n", SHAPES)
def test_without_records_a_call_covers_the_whole_range(m, n):
    dec = _decoder(m, n)
    step = dec.mc_osd_step()
    for flags in (0, _lib.FLAG_LAYERED, _lib.FLAG_QUANT, _lib.FLAG_PAIRWISE_COLSUM, _lib.FLAG_DENSE_F_COLSUM,
                  _lib.FLAG_LAYERED | _lib.FLAG_FORCE_FULL, _lib.FLAG_OSD_CS | (3 << _lib.OSD_ORDER_SHIFT)):
        for whole in (1, 37, step, step + 1, 1 << 40):
            for K in (1, 5):
                assert dec.mc_step(flags, whole, n_budgets=K) == whole, (flags, whole, K)
        assert dec.mc_step(flags, 0) == 1          # (an empty range: the value is still the step of a ``range``)
