"""CPU: the host side of Relay-BP's large build (QBP_OPT_RELAY_MEM) -- the constant, the LDS arithmetic of both builds
on the shapes the option exists for, ``RelayConfig.large`` and its dict form, and the command line."""
import os
import re

import numpy as np
import pytest

import record_kernel_util as ru
import large_util as lu
from qldpc_amd import _lib, mc, relay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_equals_the_header():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    m = re.search(r"\bQBP_OPT_RELAY_MEM\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == _lib.OPT_RELAY_MEM == 16
    values = [int(v) for v in re.findall(r"\bQBP_OPT_[A-Z0-9_]+\s*=\s*(\d+)", header)]
    assert values.count(16) == 1
    assert _lib.RELAY_MEM == {False: lu.MEM_LDS, True: lu.MEM_AUTO, "force": lu.MEM_LARGE}


def test_the_header_states_the_large_figure_as_restated():
    text = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp_relay.hpp")).read()
    body = re.search(r"size_t relay_large_lds_bytes\(int m, int n, bool records\)\s*\{(.*?)\}", text, re.S).group(1)
    assert "8 * (size_t)n" in body and "4 * relay_lds_words(m)" in body and "records ?" in body


def test_lds_figures_of_the_three_shapes():
    # 34 rounds of the [[72,12,6]] phenomenological matrix: one round past the LDS build, far inside the large one
    sh = ru.ph_shape(34)
    assert (sh.m, sh.n, sh.E) == (1224, 3672, 9756)
    assert ru.relay_lds_bytes(sh.m, sh.n, sh.E) == 8 * (9756 + 3 * 3672) + 4 * 126 == 166680 > ru.LDS_LIMIT
    assert lu.relay_large_lds_bytes(sh.m, sh.n) == 8 * 3672 + 4 * 126 == 29880 < ru.LDS_DEFAULT
    assert ru.relay_lds_bytes(*[getattr(ru.ph_shape(33), k) for k in "mnE"]) <= ru.LDS_LIMIT
    # [[288,12,18]], 18 rounds: the records build
    assert lu.relay_lds_words(2592) == 252
    assert lu.relay_large_lds_bytes(2592, 7776, True) == 8 * 7776 + 4 * 252 + 7776 == 70992
    assert ru.LDS_DEFAULT < 70992 < ru.LDS_LIMIT
    # where the large figure first passes 160 KiB: one check, n = 20 475 (records build: 18 200)
    n = lu.first_n_beyond_the_limit(lambda n: lu.relay_large_lds_bytes(1, n))
    assert n == 20475 and lu.relay_large_lds_bytes(1, n) == 163848 and lu.relay_large_lds_bytes(1, n - 1) == ru.LDS_LIMIT
    assert lu.first_n_beyond_the_limit(lambda n: lu.relay_large_lds_bytes(1, n, True)) == 18200
    # (1 x 20 000 fits the batch build and not the records build)
    assert lu.relay_large_lds_bytes(1, 20000) == 160048 <= ru.LDS_LIMIT < lu.relay_large_lds_bytes(1, 20000, True) == 180048


def test_large_grid_of_the_34_round_matrix():
    sh = ru.ph_shape(34)
    sh.work = ru.pad64(72 * 34) + ru.pad64(36 * 33) + ru.pad64(36)      # var_items: columns of weight 3, 2 and 1
    assert sh.work == 3776 and ru.relay_threads(sh) == 960
    assert lu.relay_large_grid(sh, 8, 256) == 8 and lu.relay_large_grid(sh, 1 << 30, 256) == 256


def test_config_round_trips_large_through_its_dict_form():
    g = relay.relay_gammas(7, 3, 0.1, (-0.2, 0.6), 1)
    assert relay.RelayConfig(g, [4, 4, 4]).large is False
    for large in (False, True, "force"):
        cfg = relay.RelayConfig(g, [4, 4, 4], 2, 0.9, 15.0, large=large)
        assert cfg.large is large or cfg.large == large
        back = relay.as_config(cfg.as_dict(), 7)
        assert back.large == large and type(back.large) is type(large)
        assert np.array_equal(back.gammas, cfg.gammas) and np.array_equal(back.leg_iters, cfg.leg_iters)
        assert (back.stop_after, back.alpha, back.clip_llr) == (2, 0.9, 15.0)
        assert relay.as_config(cfg, 7) is cfg
        short = relay.as_config(dict(legs=3, iters=4, gamma0=0.1, interval=(-0.2, 0.6), seed=1, large=large), 7)
        assert short.large == large and np.array_equal(short.gammas, g)
    assert relay.as_config(dict(legs=3, iters=4, gamma0=0.1, interval=(0, 1)), 7).large is False
    for bad in (1, 2, "yes", None):
        with pytest.raises(ValueError):
            relay.RelayConfig(g, [4, 4, 4], large=bad)


def test_run_flags_do_not_depend_on_large():
    g = relay.relay_gammas(7, 2, 0.1, (0, 1), 0)
    for large in (False, True, "force"):
        assert mc.relay_run_flags(0, relay.RelayConfig(g, [3, 3], large=large)) == _lib.FLAG_RELAY
        assert mc.relay_run_flags(_lib.FLAG_FORCE_FULL, dict(legs=2, iters=3, gamma0=0.1, interval=(0, 1), large=large)) \
            == _lib.FLAG_RELAY | _lib.FLAG_FORCE_FULL
        with pytest.raises(ValueError):
            mc.relay_run_flags(_lib.FLAG_OSD0, relay.RelayConfig(g, [3, 3], large=large))


class _Reached(Exception):
    pass


def test_command_line_takes_relay_large_only_with_relay(capsys, monkeypatch):
    with pytest.raises(SystemExit) as e:
        mc.main(["--relay", "5", "12", "--relay-large", "--help"])
    assert e.value.code == 0 and "--relay-large" in capsys.readouterr().out
    for argv in (["--relay-large"], ["--relay-large", "--osd"], ["--relay-large", "--gd", "8", "6"]):
        with pytest.raises(SystemExit) as e:          # refused before any GPU work
            mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05"] + argv)
        assert e.value.code == 2 and "--relay-large needs --relay" in capsys.readouterr().err
    seen = []

    def spy(cfg, n):                                  # (main validates the settings here, before any GPU work)
        seen.append(cfg)
        raise _Reached

    monkeypatch.setattr(relay, "as_config", spy)
    for extra, want in (([], False), (["--relay-large"], True)):
        with pytest.raises(_Reached):
            mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05", "--trials", "10", "--relay", "5", "12"] + extra)
        assert seen[-1]["large"] is want
    monkeypatch.undo()
    assert relay.as_config(seen[-1], 72).large is True and relay.as_config(seen[0], 72).large is False
