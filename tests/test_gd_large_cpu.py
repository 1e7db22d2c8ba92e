"""CPU: the host side of BP guided decimation's large build (QBP_OPT_GD_MEM) -- the constant, the LDS arithmetic of
both builds on the shapes the option exists for, the upper limit, ``GDConfig.large`` and its dict form, and the command
lines."""
import os
import re

import pytest

import large_util as lu
import record_kernel_util as ru
from qldpc_amd import _lib, gd, mc, paper_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_equals_the_header():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    m = re.search(r"\bQBP_OPT_GD_MEM\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == _lib.OPT_GD_MEM == 18
    values = [int(v) for v in re.findall(r"\bQBP_OPT_[A-Z0-9_]+\s*=\s*(\d+)", header)]
    assert values.count(18) == 1
    assert _lib.GD_MEM == {False: lu.MEM_LDS, True: lu.MEM_LARGE, "auto": lu.MEM_AUTO}


def test_the_header_states_the_large_figure_as_restated():
    text = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp_gd.hpp")).read()
    words = re.search(r"size_t gd_large_lds_words\(int m, int n\)\s*\{(.*?)\n\}", text, re.S).group(1)
    assert "GD_HEAD_WORDS + 3 * mw + 2 * nw + 1" in words
    body = re.search(r"size_t gd_large_lds_bytes\(int m, int n, bool tables\)\s*\{(.*?)\n\}", text, re.S).group(1)
    assert "NP_LDS_BYTES" in body and "8 * (size_t)n" in body and "4 * gd_large_lds_words(m, n)" in body
    # the wavefronts per CU of gd_launch are those the restated grid counts on
    host = open(os.path.join(ROOT, "qldpc_amd", "csrc", "qbp.hip")).read()
    assert "const int waves = large ? (sp ? 16 : 24) : (sp ? 20 : 28);" in host
    assert lu.GD_LARGE_WAVES_PER_CU == {True: 16, False: 24}


def test_lds_figures_of_the_two_headline_matrices():
    assert ru.GD_HEAD_WORDS == 40 and ru.np_lds_bytes() == 3072
    # 2592 x 7776: 81 + 2 * 81 check words, 2 * 243 map words
    assert lu.gd_large_lds_words(2592, 7776) == 40 + 3 * 81 + 2 * 243 + 1 == 770
    assert lu.gd_large_lds_bytes(2592, 7776, False) == 8 * 7776 + 4 * 770 == 65288
    assert lu.gd_large_lds_bytes(2592, 7776, True) == 65288 + 3072 == 68360
    # the 1008 x 8991 hyperedge model
    assert lu.gd_large_lds_words(1008, 8991) == 40 + 3 * 32 + 2 * 281 == 698
    assert lu.gd_large_lds_bytes(1008, 8991, False) == 8 * 8991 + 4 * 698 == 74720
    assert lu.gd_large_lds_bytes(1008, 8991, True) == 77792
    for m, n in ((2592, 7776), (1008, 8991)):
        for tables in (False, True):
            assert lu.gd_large_lds_bytes(m, n, tables) <= ru.LDS_LIMIT // 2        # (two workgroups per CU fit)
    # (their LDS builds are far beyond: 9 and 3 entries per column at the least)
    assert ru.gd_lds_bytes(2592, 7776, 9 * 2592, False) > ru.LDS_LIMIT < ru.gd_lds_bytes(1008, 8991, 3 * 8991, False)


@pytest.mark.parametrize("tables,T", [(False, 41), (True, 40)], ids=["min_sum", "sum_product"])
def test_first_round_count_past_the_lds_build(tables, T):
    assert lu.gd_first_rounds_beyond_the_lds_build(tables) == T
    sh, before = ru.ph_shape(T), ru.ph_shape(T - 1)
    assert ru.gd_lds_bytes(before.m, before.n, before.E, tables) <= ru.LDS_LIMIT < ru.gd_lds_bytes(sh.m, sh.n, sh.E, tables)
    want = {False: (1476, 4428, 11772, 166304, 37264), True: (1440, 4320, 11484, 165304, 39416)}[tables]
    assert (sh.m, sh.n, sh.E, ru.gd_lds_bytes(sh.m, sh.n, sh.E, tables), lu.gd_large_lds_bytes(sh.m, sh.n, tables)) == want
    assert lu.gd_large_lds_bytes(sh.m, sh.n, tables) < ru.LDS_DEFAULT          # the large build fits, with room


def test_upper_limit_of_the_large_build():
    # one check: 8 n + n / 4 bytes + 44 words (+ the tables)
    n = lu.first_n_beyond_the_limit(lambda n: lu.gd_large_lds_bytes(1, n, False))
    assert n == 19839 and lu.gd_large_lds_bytes(1, n - 1, False) == ru.LDS_LIMIT < lu.gd_large_lds_bytes(1, n, False) == 163848
    n = lu.first_n_beyond_the_limit(lambda n: lu.gd_large_lds_bytes(1, n, True))
    assert n == 19466 and lu.gd_large_lds_bytes(1, n - 1, True) == ru.LDS_LIMIT < lu.gd_large_lds_bytes(1, n, True) == 163848
    assert lu.first_n_beyond_the_limit(lambda n: lu.gd_large_lds_bytes(2592, n, False)) < 19839


def test_large_grid_of_the_41_round_matrix():
    sh = ru.ph_shape(41)
    sh.work = ru.pad64(72 * 41) + ru.pad64(36 * 40) + ru.pad64(36)      # var_items: columns of weight 3, 2 and 1
    assert sh.work == 4544 and ru.gd_threads(sh) == 512
    # 8 wavefronts per workgroup: three of them in min-sum's 24 wavefronts, two in sum-product's 16
    assert lu.gd_large_grid(sh, 8, 256, False) == 8 and lu.gd_large_grid(sh, 1 << 30, 256, False) == 3 * 256
    assert lu.gd_large_grid(sh, 1 << 30, 256, True) == 2 * 256
    assert lu.gd_large_grid(sh, 1 << 30, 256, True, blocks_per_cu=1) == 256


def test_config_takes_large_and_its_dict_form():
    assert gd.GDConfig().large is False and gd.GDConfig(4, 2).large is False
    for large in (False, True, "auto"):
        cfg = gd.GDConfig(4, 2, 25.0, gd.SUM_PRODUCT, 0.9, 15.0, large=large)
        assert cfg.large == large and type(cfg.large) is type(large)
        back = gd.as_config(dict(iters_per_round=4, max_rounds=2, variant=gd.SUM_PRODUCT, large=large))
        assert back.large == large and type(back.large) is type(large)
        assert (back.iters_per_round, back.max_rounds, back.variant) == (4, 2, gd.SUM_PRODUCT)
        assert gd.as_config(cfg) is cfg
        assert mc.gd_run_flags(0, cfg) == _lib.FLAG_GD == mc.gd_run_flags(0, dict(large=large))
    assert gd.as_config(dict(iters_per_round=4)).large is False
    for bad in (1, 0, 2, "yes", "force", None, "AUTO"):
        with pytest.raises(ValueError):
            gd.GDConfig(4, 2, large=bad)
        with pytest.raises(ValueError):
            gd.as_config(dict(large=bad))
        with pytest.raises(ValueError):
            mc.gd_run_flags(0, dict(large=bad))
    with pytest.raises(ValueError):
        gd.as_config(dict(larger=True))


class _Reached(Exception):
    pass


def test_command_line_takes_gd_large_only_with_gd(capsys, monkeypatch):
    with pytest.raises(SystemExit) as e:
        mc.main(["--gd", "8", "6", "--gd-large", "--help"])
    assert e.value.code == 0 and "--gd-large" in capsys.readouterr().out
    for argv in (["--gd-large"], ["--gd-large", "--osd"], ["--gd-large", "--relay", "5", "12"]):
        with pytest.raises(SystemExit) as e:          # refused before any GPU work
            mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05"] + argv)
        assert e.value.code == 2 and "--gd-large needs --gd" in capsys.readouterr().err
    seen = []

    def spy(cfg):                                     # (main validates the settings here, before any GPU work)
        seen.append(cfg)
        raise _Reached

    monkeypatch.setattr(gd, "as_config", spy)
    for extra, want in (([], False), (["--gd-large"], "auto")):
        with pytest.raises(_Reached):
            mc.main(["--code", "[[72, 12, 6]]", "--p", "0.05", "--trials", "10", "--gd", "8", "6"] + extra)
        assert seen[-1]["large"] == want and type(seen[-1]["large"]) is type(want)
    monkeypatch.undo()
    assert gd.as_config(seen[-1]).large == "auto" and gd.as_config(seen[0]).large is False


def test_paper_results_command_line_takes_gd_large_only_with_gd(capsys):
    for argv, text in ((["--gd-large"], "--gd-large needs --gd"), (["--gd", "8", "6", "--osd", "0"], "--gd excludes"),
                       (["--gd", "8", "6", "--lsd", "1"], "--gd excludes"), (["--gd", "0", "6"], "iters_per_round")):
        with pytest.raises(SystemExit) as e:
            paper_results.main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err
