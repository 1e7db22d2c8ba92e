"""CPU: the host side of layered BP's large build (QBP_OPT_LAYERED_MEM) -- the constant, the LDS arithmetic of both
builds on the shapes the option exists for, ``layered="large"`` on the Monte-Carlo drivers and the command line."""
import os
import re

import numpy as np
import pytest

import large_util as lu
import record_kernel_util as ru
from qldpc_amd import _lib, layered, mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_equals_the_header():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    m = re.search(r"\bQBP_OPT_LAYERED_MEM\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == _lib.OPT_LAYERED_MEM == 17
    values = [int(v) for v in re.findall(r"\bQBP_OPT_[A-Z0-9_]+\s*=\s*(\d+)", header)]
    assert values.count(17) == 1
    assert _lib.LAYERED_MEM == {False: lu.MEM_LDS, True: lu.MEM_AUTO}


def test_the_header_states_the_large_figure_as_restated():
    text = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp_layered.hpp")).read()
    body = re.search(r"size_t layered_large_lds_bytes\(int m, int n, int S, bool tables\)\s*\{(.*?)\}", text, re.S).group(1)
    assert "tables ? (size_t)NP_LDS_BYTES : 0" in body and "8 * (size_t)S * (size_t)n" in body
    assert "(size_t)LAYERED_WG_WORDS + (size_t)S * layered_slot_words(m)" in body


def test_lds_figures_of_the_shapes_the_option_exists_for():
    tables = ru.np_lds_bytes()
    # 40 rounds of the [[72,12,6]] phenomenological matrix: one round past the LDS build, far inside the large one
    sh = ru.ph_shape(40)
    assert (sh.m, sh.n, sh.E) == (1440, 4320, 11484)
    assert lu.layered_slot_words(1440) == 56
    assert ru.layered_lds_bytes(sh.m, sh.n, sh.E, 1, True) == tables + 8 * (11484 + 2 * 4320) + 4 * 88 > ru.LDS_LIMIT
    assert lu.layered_large_lds_bytes(sh.m, sh.n, 1, True) == tables + 8 * 4320 + 4 * 88 < ru.LDS_DEFAULT
    assert lu.layered_auto_is_large(sh) and not lu.layered_auto_is_large(ru.ph_shape(39))
    # [[288,12,18]], 18 rounds (every row of weight 8 but the first 144) and the 1008 x 8991 detector error model
    # (E is whatever it is: the large figure does not depend on it, and the LDS figure passes the limit with E = n)
    for m, n, E in ((2592, 7776, 8 * 2592 - 144), (1008, 8991, 8991)):
        assert ru.layered_lds_bytes(m, n, E, 1, True) > ru.LDS_LIMIT > lu.layered_large_lds_bytes(m, n, 1, True)
        assert ru.layered_lds_bytes(m, n, E, 1, False) > ru.LDS_LIMIT
    assert lu.layered_large_lds_bytes(2592, 7776, 1, True) == tables + 8 * 7776 + 4 * (32 + 92)
    assert ru.LDS_DEFAULT < lu.layered_large_lds_bytes(2592, 7776, 1, True) < 80 * 1024
    # where the large figure first passes 160 KiB
    for m in (1, 1008):
        n = lu.layered_n_limit(m)
        assert lu.layered_large_lds_bytes(m, n, 1, True) <= ru.LDS_LIMIT < lu.layered_large_lds_bytes(m, n + 1, 1, True)
    assert lu.layered_n_limit(1) == (ru.LDS_LIMIT - tables - 4 * (32 + 12)) // 8 and 19500 < lu.layered_n_limit(1008) < lu.layered_n_limit(1) < 20500


def test_slots_and_grid_follow_the_build():
    # 2592 x 7776, widest level 648: one slot in either build; the large build is what fits
    sh = ru.Shape.__new__(ru.Shape)
    sh.m, sh.n, sh.E = 2592, 7776, 8 * 2592 - 144
    assert lu.layered_slots(sh, 648, 1 << 20, True, 0, True) == 1
    assert lu.layered_slots(sh, 648, 1 << 20, True, 2, True) == 2         # two slots: 2 x 62 KiB of V
    assert lu.layered_slots(sh, 648, 1 << 20, True, 3, True) == 2         # a third does not fit 160 KiB
    assert lu.layered_grid(sh, 1, 1 << 20, 256, True, True) == 2 * 256    # two workgroups' LDS per CU
    # [[72,12,6]], widest level 18 of the default order: the large build holds more slots under 80 KiB
    sh72 = ru.Shape.__new__(ru.Shape)
    sh72.m, sh72.n, sh72.E = 36, 72, 216
    assert lu.layered_slots(sh72, 18, 1 << 20, False, 0, True) == lu.layered_slots(sh72, 18, 1 << 20, False, 0, False) == 14
    assert lu.layered_slots(sh72, 1, 1 << 20, True, 0, False) == ru.layered_slots(sh72, 1, 1 << 20, True) == 32
    assert lu.layered_grid(sh72, 3, 37, 256, False, True, 1) == 13 and lu.layered_grid(sh72, 3, 10 ** 6, 256, False, True, 1) == 256


class _Stub:
    """What mc._configure_layered and layered.performLayeredBPBatch need of a Decoder, recording the option writes of
    the real ``Decoder.layered_configure`` (no GPU: the library is never loaded)."""
    m, n = 3, 7

    def __init__(self):
        self.writes, self.orders = [], []

    def layered_configure(self, order=None, large=None):
        if large is not None:
            self.writes.append((_lib.OPT_LAYERED_MEM, _lib.LAYERED_MEM[large]))
        self.orders.append(order)


def test_layered_large_reaches_the_option_write():
    dec = _Stub()
    mc._configure_layered(dec, "large")
    assert dec.writes == [(17, lu.MEM_AUTO)] and dec.orders == [None]
    mc._configure_layered(dec, True)
    assert dec.writes[-1] == (17, lu.MEM_LDS) and dec.orders[-1] is None
    order = np.array([2, 0, 1])
    before = list(dec.writes)
    mc._configure_layered(dec, order)
    assert dec.writes == before and dec.orders[-1] is order            # an order leaves the option as it is
    for off in (False, None):
        mc._configure_layered(dec, off)
    assert dec.writes == before and len(dec.orders) == 3
    assert mc.layered_run_flags(_lib.FLAG_OSD0, "large", _lib.MIN_SUM) == _lib.FLAG_OSD0 | _lib.FLAG_LAYERED
    with pytest.raises(ValueError):
        mc.layered_run_flags(0, "large", _lib.DAMPED_SP)
    with pytest.raises(ValueError):
        mc.layered_run_flags(0, "huge", _lib.MIN_SUM)


def test_decoder_layered_configure_writes_the_option_before_it_configures(monkeypatch):
    calls = []

    class Lib:
        def qbp_set_option(self, h, option, value):
            calls.append(("option", option, value))
            return 0

        def qbp_layered_configure(self, h, order):
            calls.append(("configure", order))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    dec = _lib.Decoder.__new__(_lib.Decoder)
    import threading
    dec._lock, dec._h, dec.m, dec._layered = threading.RLock(), None, 3, None
    dec.layered_configure(None)
    assert calls == [("configure", None)]
    dec.layered_configure(None, large=True)                          # (the same order: no second configuration)
    assert calls[1:] == [("option", 17, 2)]
    dec.layered_configure(np.array([2, 0, 1]), large=False)
    assert calls[2][:] == ("option", 17, 0) and calls[3][0] == "configure" and len(calls) == 4
    for bad in (1, 2, "large", "force"):
        with pytest.raises(ValueError):
            dec.layered_configure(None, large=bad)
    assert len(calls) == 4


def test_perform_layered_bp_validates_large_before_any_gpu_work():
    H = np.eye(3, dtype=np.uint8)
    for bad in (1, None, "large"):
        with pytest.raises(ValueError):
            layered.performLayeredBPBatch(H, np.zeros((1, 3), np.uint8), np.ones(3), large=bad)


class _Reached(Exception):
    pass


def test_command_line_takes_layered_large_only_with_layered(capsys, monkeypatch):
    with pytest.raises(SystemExit) as e:
        mc.main(["--layered", "--layered-large", "--help"])
    assert e.value.code == 0 and "--layered-large" in capsys.readouterr().out
    for argv in (["--layered-large"], ["--layered-large", "--osd"], ["--layered-large", "--relay", "5", "12"]):
        with pytest.raises(SystemExit) as e:          # refused before any GPU work
            mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05"] + argv)
        assert e.value.code == 2 and "--layered-large needs --layered" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05", "--layered", "--layered-large", "--variant", "damped"])
    assert e.value.code == 2
    capsys.readouterr()
    seen = []

    def spy(code, ps, trials, **kw):                  # (main's first call of the driver, before any GPU work)
        seen.append(kw["layered"])
        raise _Reached

    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    monkeypatch.setattr(mc, "run_sweep", spy)
    for extra, want in ((["--layered"], True), (["--layered", "--layered-large"], "large"), ([], False)):
        with pytest.raises(_Reached):
            mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05", "--trials", "10", "--variant", "min-sum"] + extra)
        assert seen[-1] == want and type(seen[-1]) is type(want)
