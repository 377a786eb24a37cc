"""bench.py's plain run and its --dump-outputs: the result line of a run without --full
carries the headline figures only, --steps sets the timed steps, and the dumped arrays are
the particle state after the last timed step in idp order (float32/float64 .npy files, a
fixed seeded sample when the state is larger than the dump limit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = {"idp": (np.float64, 1), "pos": (np.float64, 3), "vel": (np.float32, 3), "rhop": (np.float32, 1),
         "code": (np.float32, 1)}


def _state(n, seed=1):
    rng = np.random.default_rng(seed)
    return dict(idp=rng.permutation(n).astype(np.uint32), pos=rng.random((n, 3)),
                vel=rng.random((n, 3)).astype(np.float32), rhop=rng.random(n).astype(np.float32),
                code=(np.arange(n) % 7).astype(np.uint16))


def _load(d, suffix=""):
    return {k: np.load(os.path.join(d, k + suffix + ".npy")) for k in NAMES}


def test_dump_is_idp_ordered_and_typed(tmp_path):
    import bench

    p = _state(1001)
    bench.dump_outputs(str(tmp_path / "d"), p, 0, 1)
    got = _load(str(tmp_path / "d"))
    order = np.argsort(p["idp"])
    for k, (dt, w) in NAMES.items():
        assert got[k].dtype == dt and got[k].shape == ((1001,) if w == 1 else (1001, w))
        assert np.array_equal(got[k], p[k][order].astype(dt))


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench

    p = _state(5000)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 52 * 777)  # 52 bytes per particle
    bench.dump_outputs(str(tmp_path / "a"), p, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), p, 1, 2)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"), "_rank1")
    assert sum(x.nbytes for x in a.values()) <= 52 * 777
    assert len(a["idp"]) == 777 and np.all(np.diff(a["idp"]) > 0)
    order = np.argsort(p["idp"])
    sel = a["idp"].astype(np.int64)  # idp = 0..n-1, so an idp is its own rank in idp order
    for k, (dt, _) in NAMES.items():
        assert np.array_equal(a[k], b[k])
        assert np.array_equal(a[k], p[k][order][sel].astype(dt))


def test_default_dump_limit_fits_64mb():
    import bench

    assert bench.DUMP_MAX_BYTES <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_state(tmp_path):
    d = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dp", "0.03", "--dump-outputs", d]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["timed_window"] == [10, 13]
    assert res["ms_per_step"] > 0 and res["unit"] == "particle-steps/s" and res["higher_is_better"] is True
    n = res["config"]["np"]
    assert abs(res["value"] - n * 3 / (res["ms_per_step"] * 3e-3)) <= 1e-6 * res["value"]
    # nothing of --full ran
    assert res["full"] is False and res["roofline"] is None and res["cpu_baseline"] is None
    assert res["cfg3_1gpu"] is None and "developed_flow" not in res
    got = _load(d)
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in NAMES)
    for k, (dt, w) in NAMES.items():
        assert got[k].dtype == dt and got[k].shape == ((n,) if w == 1 else (n, w))
        assert np.isfinite(got[k]).all()
    assert np.array_equal(got["idp"], np.arange(n))
    # the state after presteps + warmup + steps = 13 steps, as the solver run directly gives it
    from dualsphysics_multilayer_amd.case import DamBreakCase
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    s = SphGpuSingle(DamBreakCase(0.03), device=0)
    s.run(13)
    s.sync()
    p = s.particles()
    s.close()
    order = np.argsort(p["idp"])
    for k in ("pos", "vel", "rhop"):
        assert np.array_equal(got[k], p[k][order]), k
