"""RigidAlgorithm 2 and 0 on the GPU against the REFERENCE: the fixtures of tests/golden/make_dem.py
(case.py BlocksCase: a tank, a pool, three floating boxes of different materials; one lands on the
floor, one hits another within the kept steps) through the case loader and the C ABI.

* every kept PART within max(10 x the reference's own fast-math / strict noise, FLOOR), the excluded
  sets equal, on the tiled kernel and, for the first variant, on the per-particle kernel;
* every PART time and DemDtForce after it against the reference's PART headers; the restart variant
  starts from the reference's PART 30 and takes DemDtForce from that file;
* the first variant run with RigidAlgorithm=1 leaves the fixture;
* the unchanged path: the flume fixture (RigidAlgorithm=1) bit for bit the state the parent commit
  produced (tests/golden/dem_parent_flume_*.npz);
* the phase-level calls: sph_interaction_forces applies the DEM pass as sph_solver_run does; the
  update calls refuse floating bodies as before, so a step by phases does not exist for these cases.
"""
import os
import shutil

import numpy as np
import pytest

from golden_io import maxdiff
from test_forcing import FLOOR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "bi4")
VARIANTS = ("verlet_ddt2", "symplectic_ddt1", "verlet_ddt2_half", "verlet_ddt3_2d", "free_verlet_ddt2",
            "restart_verlet_ddt2")
PART_KEYS = ("idp", "pos", "vel", "rhop")


def fdir(v):
    return os.path.join(FIX, "dem_" + v)


def ref(v):
    return np.load(os.path.join(fdir(v), "ref.npz"))


def load_case(v, path=None, **kw):
    from dualsphysics_multilayer_amd.xmlcase import XmlCase

    g = ref(v)
    step, ddt, cellmode = (int(x) for x in g["meta"])
    if step:
        kw["step_algorithm"] = step
    if ddt:
        kw["tdensity"] = ddt
    if cellmode:
        kw["cellmode"] = cellmode
    d = fdir(v)
    name = "CaseBlocks2D" if v.endswith("_2d") else "CaseBlocks"
    if "partbegin" in g.files:
        return XmlCase(path or os.path.join(d, name), int(g["partbegin"]), d, **kw)
    return XmlCase(path or os.path.join(d, name), **kw)


def kept(g):
    return sorted(int(k[1:].split("_")[0]) for k in g.files if k.startswith("s") and k.endswith("_idp"))


def tol(g, k):
    n = g["noise_%d" % k]
    return tuple(max(10.0 * float(n[i]), FLOOR[i]) for i in range(3))


def by_idp(p):
    o = np.argsort(p["idp"], kind="stable")
    return {q: p[q][o] for q in PART_KEYS}


def distances(s, g, v, check=True):
    """Runs to every kept step; the distances from the reference's PARTs in tolerances, the time and
    DemDtForce errors.  check: assert them."""
    done = int(g["partbegin"]) if "partbegin" in g.files else 0
    worst = 0.0
    for k in kept(g):
        s.run(k - done)
        done = k
        got = by_idp(s.particles())
        want = {q: g["s%d_%s" % (k, q)] for q in PART_KEYS}
        assert np.array_equal(got["idp"], want["idp"]), "excluded/duplicated particles"
        t = tol(g, k)
        d = [maxdiff(got, want, q) for q in ("pos", "vel", "rhop")]
        st = s.stats()
        dtime = abs(st["time"] - float(g["times"][k]))
        ddem = abs(st["dem_dtforce"] - float(g["demdtforce"][k]))
        print("%s step %d: dpos %.3g / %.3g  dvel %.3g / %.3g  drho %.3g / %.3g  dtime %.3g  dDemDtForce %.3g (%.6g)" % (
            v, k, d[0], t[0], d[1], t[1], d[2], t[2], dtime, ddem, float(g["demdtforce"][k])))
        worst = max(worst, d[0] / t[0], d[1] / t[1])
        if check:
            assert d[0] <= t[0] and d[1] <= t[1] and d[2] <= t[2], (k, d, t)
            assert dtime <= 1e-8 * max(1, k), (k, st["time"], g["times"][k])
            assert ddem <= 1e-8, (k, st["dem_dtforce"], g["demdtforce"][k])
            assert st["error_flags"] == 0
    return worst


def single(case):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    return SphGpuSingle(case, device=0)


@pytest.mark.parametrize("v", VARIANTS)
def test_gpu_matches_reference_parts(v):
    g = ref(v)
    x = load_case(v)
    assert x.use_dem == (not v.startswith("free")) and x.ftmode == 2
    if v.startswith("restart"):
        assert x.demdtforce0 == float(g["demdtforce0"]) > 0
    distances(single(x), g, v)


def test_gpu_matches_reference_parts_per_particle_kernel(monkeypatch):
    monkeypatch.setenv("SPH_INTERACTION", "simple")
    distances(single(load_case("verlet_ddt2")), ref("verlet_ddt2"), "verlet_ddt2 simple")


def test_restart_takes_demdtforce_from_the_part(tmp_path):
    """The restart's first step uses the file's DemDtForce: the PART header the core writes after one
    step carries the reference's value, and with DtIni in its place (DemDtForce = 0 in the header) the
    first kept PART is missed."""
    from dualsphysics_multilayer_amd.core import read_part

    v = "restart_verlet_ddt2"
    g = ref(v)
    x = load_case(v)
    s = single(x)
    assert s.stats()["dem_dtforce"] == float(g["demdtforce0"])
    s.run(1)
    s.sync()
    fn = str(tmp_path / "Part_0031.bi4")
    s.save_part(fn, 31)
    h = read_part(fn)[0]
    assert abs(h["dem_dtforce"] - float(g["demdtforce"][31])) <= 1e-8 and h["dem_dtforce"] > 0
    x0 = load_case(v)
    x0.demdtforce0 = 0.0
    s0 = single(x0)
    assert s0.stats()["dem_dtforce"] == pytest.approx(x0._derived()["dtini"])
    s0.run(1)
    a, b = by_idp(s.particles()), by_idp(s0.particles())
    assert np.abs(a["vel"] - b["vel"]).max() > 0, "DemDtForce of the file has no effect on the first step"


def test_gpu_option_is_seen(tmp_path):
    """The first variant with RigidAlgorithm=1 fails the parity check of its fixture."""
    v = "verlet_ddt2"
    d = tmp_path / "sph"
    shutil.copytree(fdir(v), d)
    fx = d / "CaseBlocks.xml"
    xml = fx.read_text()
    assert xml.count('key="RigidAlgorithm" value="2"') == 1
    fx.write_text(xml.replace('key="RigidAlgorithm" value="2"', 'key="RigidAlgorithm" value="1"'))
    x = load_case(v, path=str(d / "CaseBlocks"))
    assert x.ftmode == 1
    assert distances(single(x), ref(v), v + " as RigidAlgorithm=1", check=False) > 100


@pytest.mark.parametrize("kernel", ["tiled", "simple"])
def test_unchanged_path_is_the_parents_state(kernel, monkeypatch):
    """RigidAlgorithm=1: the flume fixture after 20 steps, bit for bit what the parent commit gave."""
    from dualsphysics_multilayer_amd.xmlcase import XmlCase

    if kernel == "simple":
        monkeypatch.setenv("SPH_INTERACTION", "simple")
    want = np.load(os.path.join(HERE, "golden", "dem_parent_flume_%s.npz" % kernel))
    s = single(XmlCase(os.path.join(FIX, "flume_verlet_ddt2", "CaseFlume")))
    s.run(20)
    got = by_idp(s.particles())
    assert s.stats()["time"] == float(want["time"])
    for q in PART_KEYS:
        assert np.array_equal(got[q], want[q]), q


def test_phase_calls_apply_the_dem_pass():
    from dualsphysics_multilayer_amd.core import SphError

    s = single(load_case("verlet_ddt2"))
    s.run(30)  # contacts by now
    a = s.interaction()  # Interaction_Forces(1) + the maxima
    s.Interaction_Forces(1)
    s.DtVariable(False)
    st = s.stats()
    assert st["viscdtmax"] == a["viscdtmax"] and st["acemax"] == a["acemax"]
    s0 = single(load_case("free_verlet_ddt2"))
    assert a["viscdtmax"] > 100 * max(s0.interaction()["viscdtmax"], 1.0)  # the DEM dt, not the SPH one
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED"):
        s.ComputeVerlet()
