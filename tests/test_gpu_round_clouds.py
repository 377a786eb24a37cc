"""The tiled interaction's candidate test (last group stopped at the wave's longest window)
on the clouds of tests/round_clouds.py: window lengths on both sides of every limit of the
test groups and drain rounds (tests/test_round_clouds_cpu.py asserts what they hold).

* check() of tests/test_gpu_clouds.py, unchanged: the oracle's particle order, the
  checked-candidate counts bit for bit, ar and ace within 1e-5 of the oracle, and its margin
  against the float64 sum; DDT 0-3, CellMode full and half.
* The same run in two child processes, the test hook SPH_TILE_FULL unset and set (full
  32-record groups, the library reads it once per process): ar, ace and the maxima of one
  interaction and the particles after 25 steps are equal bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import round_clouds
from test_gpu_clouds import check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("ddt", [0, 1, 2, 3])
@pytest.mark.parametrize("name", round_clouds.NAMES)
def test_round_cloud(name, ddt, cellmode):
    case = round_clouds.make(name, tdensity=ddt, cellmode=cellmode)
    check(case, ddt, "round %s ddt %d cellmode %d" % (name, ddt, cellmode))


def _child(tmp_path, tag, hook, name, coefh, cellmode):
    out = str(tmp_path / ("%s.npz" % tag))
    env = dict(os.environ)
    env.pop("SPH_TILE_FULL", None)
    if hook:
        env["SPH_TILE_FULL"] = "1"
    root = os.path.dirname(HERE)
    env["PYTHONPATH"] = os.pathsep.join([root, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.join(HERE, "round_clouds.py"), name, str(coefh), str(cellmode), out],
                       capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("test hook SPH_TILE_FULL" in r.stderr) == bool(hook), r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name,coefh,cellmode", [("even", 1.0, 1), ("patch", 1.0, 1), ("patch", 1.0, 2),
                                                  ("dam", 1.0, 1), ("dam", 1.2, 1)])
def test_hook_changes_no_bit(name, coefh, cellmode, tmp_path):
    a = _child(tmp_path, "plain", False, name, coefh, cellmode)
    b = _child(tmp_path, "full", True, name, coefh, cellmode)
    assert sorted(a) == sorted(b) and "ar" in a and any(k.startswith("p_") for k in a)
    assert np.isfinite(a["ar"]).all() and np.abs(a["ace"]).max() > 0
    for k in sorted(a):
        assert a[k].tobytes() == b[k].tobytes(), k
