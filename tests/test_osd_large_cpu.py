"""CPU: the host side of QBP_FLAG_OSD_LARGE -- the constant, the flag builders, the command line and the keyword's way
through ``run_dem``."""
import os
import re

import numpy as np
import pytest

from qldpc_amd import _lib, dem, mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_equals_the_header():
    header = open(os.path.join(ROOT, "include", "qbp.h")).read()
    m = re.search(r"\bQBP_FLAG_OSD_LARGE\s*=\s*(\d+)u", header)
    assert m and int(m.group(1)) == _lib.FLAG_OSD_LARGE == 256
    others = [int(v) for v in re.findall(r"\bQBP_FLAG_[A-Z0-9_]+\s*=\s*(\d+)u", header)]
    assert others.count(256) == 1 and all(v & (v - 1) == 0 for v in others)


def test_flag_builders():
    base = _lib.osd_flags("cs", 7)
    assert _lib.osd_flags("cs", 7, large=True) == base | 256
    assert _lib.osd_flags("e", 12, large=True) == _lib.osd_flags("e", 12) | _lib.FLAG_OSD_LARGE
    assert _lib.osd_flags("cs", 7, large=False) == base == _lib.osd_flags("cs", 7, False)
    with pytest.raises(ValueError):
        _lib.osd_flags("cs", 0, large=True)
    assert mc.osd_run_flags(True, "cs", 7, osd_large=True) == base | 256
    assert mc.osd_run_flags(True, "cs", 7) == base
    assert mc.osd_run_flags(False, "cs", 0) == 0
    for args in ((True, "cs", 0), (False, "cs", 0), (False, "cs", 7)):
        with pytest.raises(ValueError):
            mc.osd_run_flags(*args, osd_large=True)


def test_command_line_argument(capsys):
    with pytest.raises(SystemExit) as e:
        mc.main(["--osd", "--osd-large", "--help"])
    assert e.value.code == 0 and "--osd-large" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:              # order 0: refused before any GPU work
        mc.main(["--osd", "--osd-large"])
    assert e.value.code == 2 and "large" in capsys.readouterr().err


def test_run_dem_passes_the_bit_on(monkeypatch):
    """``run_dem`` hands ``osd_large`` to ``osd_run_flags``, whose value is the flags of every GPU call it makes."""
    H, L, probs = dem.phenomenological("[[72, 12, 6]]", 2, 0.01)
    seen = []
    real = mc.osd_run_flags

    def spy(*args):
        seen.append(real(*args))
        return seen[-1]

    monkeypatch.setattr(mc, "osd_run_flags", spy)
    runner = lambda *a: np.zeros(12, np.int64)   # noqa: E731
    for large in (False, True):
        mc.run_dem(H, L, probs, 10, osd=True, osd_order=7, osd_large=large, runner=runner)
    assert seen == [_lib.osd_flags("cs", 7), _lib.osd_flags("cs", 7) | _lib.FLAG_OSD_LARGE]
    with pytest.raises(ValueError):
        mc.run_dem(H, L, probs, 10, osd=True, osd_order=0, osd_large=True, runner=runner)
