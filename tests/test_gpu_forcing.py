"""Imposed accelerations (k_accinput) and damping zones (k_damping) on the GPU.

* against the REFERENCE: every fixture of tests/golden/make_forcing.py through the case loader and
  the C ABI, every kept PART within max(10 x the reference's own fast-math / strict noise, FLOOR)
  (tests/test_dtopt.py's rule), on one domain, on two x-slabs and on two y-slabs; with the block
  cleared the run leaves the fixture; the phase calls are bitwise sph_solver_run;
* against float64 numpy, no reference: the imposed acceleration term by term on an off-lattice
  cloud (clouds.make("uniform", small=True)) with a second mkfluid on half the fluid, the AceMax
  re-reduction, and the damping factor bit by bit for every zone type.
"""
import copy

import numpy as np
import pytest

from golden_io import maxdiff
from test_forcing import FLUID, VARIANTS, _edited, damp, imposed_acc, kept, load_case, ref, tol, two_fluid_blocks

pytestmark = pytest.mark.gpu

PART_KEYS = ("idp", "pos", "vel", "rhop")


def single(case):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    return SphGpuSingle(case, device=0)


def by_idp(p):
    o = np.argsort(p["idp"], kind="stable")
    return {q: p[q][o] for q in PART_KEYS}


def run_check(s, g, v):
    done = 0
    for k in kept(g):
        s.run(k - done)
        done = k
        got = by_idp(s.particles())
        want = {q: g["s%d_%s" % (k, q)] for q in PART_KEYS}
        assert np.array_equal(got["idp"], want["idp"]), "excluded/duplicated particles"
        tp, tv, tr = tol(g, k)
        d = [maxdiff(got, want, q) for q in ("pos", "vel", "rhop")]
        st = s.stats() if not isinstance(s.stats(), list) else s.stats()[0]
        print("%s step %d: dpos %.3g / %.3g  dvel %.3g / %.3g  drho %.3g / %.3g  dt %.3g" % (
            v, k, d[0], tp, d[1], tv, d[2], tr, abs(st["time"] - float(g["times"][k]))))
        assert d[0] <= tp and d[1] <= tv and d[2] <= tr, (k, d, (tp, tv, tr))
        assert abs(st["time"] - float(g["times"][k])) <= 1e-8 * max(1, k), (k, st["time"], g["times"][k])


# ---- against the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS)
def test_gpu_matches_reference_parts(v):
    run_check(single(load_case(v)), ref(v), v)


@pytest.mark.parametrize("v", ["verlet_ddt2_acc_lin_nograv", "flume_verlet_ddt2_damp_plane_dom",
                               "symplectic_ddt1_acc_ang_file"])
def test_gpu_slabs_match_reference_parts(v):
    from dualsphysics_multilayer_amd.core import SphSlabGroup, slab_partition

    x = load_case(v)
    grp = SphSlabGroup(x, slab_partition(x, 2))
    run_check(grp, ref(v), v + " 2 x-slabs")
    grp.close()


def test_gpu_y_slabs_match_reference_parts():
    from dualsphysics_multilayer_amd.core import SphSlabGroup, slab_partition

    v = "verlet_ddt2_damp_box_cyl"
    x = load_case(v)
    grp = SphSlabGroup(x, slab_partition(x, 2, axis=1), axis=1)
    run_check(grp, ref(v), v + " 2 y-slabs")
    grp.close()


@pytest.mark.parametrize("v,off", [("verlet_ddt2_acc_lin_nograv", "accinputs"), ("symplectic_ddt1_acc_ang_file", "accinputs"),
                                   ("flume_verlet_ddt2_acc_float", "accinputs"), ("symplectic_ddt1_damp_plane", "damping"),
                                   ("flume_verlet_ddt2_damp_plane_dom", "damping"), ("verlet_ddt2_damp_box_cyl", "damping"),
                                   ("verlet_ddt2_acc_damp_2d", "accinputs"), ("verlet_ddt2_acc_damp_2d", "damping")])
def test_gpu_option_is_seen(v, off):
    """With the block cleared on the case the run leaves the reference's PART by more than 10
    tolerances (the parity tests would see a core that ignored it)."""
    x, g = load_case(v), ref(v)
    setattr(x, off, [])
    s = single(x)
    k = kept(g)[-1]
    s.run(k)
    got = by_idp(s.particles())
    want = {q: g["s%d_%s" % (k, q)] for q in PART_KEYS}
    tp, tv, _ = tol(g, k)
    print(v, off, maxdiff(got, want, "pos") / tp, maxdiff(got, want, "vel") / tv)
    assert maxdiff(got, want, "pos") > 10 * tp or maxdiff(got, want, "vel") > 10 * tv


def step_by_phases(s, n):
    """n steps through the phase calls only (tests/test_gpu_phases.py)."""
    for _ in range(n):
        if s.case.step_algorithm == 2:
            s.Interaction_Forces(2)
            s.DtVariable(False)
            s.ComputeSymplecticPre()
            s.RunCellDivide()
            s.Interaction_Forces(3)
            s.DtVariable(True)
            s.ComputeSymplecticCorr()
            s.RunCellDivide()
        else:
            s.Interaction_Forces(1)
            s.DtVariable(True)
            s.ComputeVerlet()
            s.RunCellDivide()


def same_bits(a, b, where):
    sa, sb = a.stats(), b.stats()
    for k in ("np", "npb", "npbok", "nout", "nstep", "time", "sym_dtpre", "error_flags"):
        assert sa[k] == sb[k], (where, k, sa[k], sb[k])
    pa, pb = a.particles(), b.particles()
    for k in PART_KEYS:  # device order: the divide's order itself
        assert np.array_equal(pa[k], pb[k]), (where, k)
    assert np.array_equal(a.dt_trace(), b.dt_trace()), (where, "dt_trace")


@pytest.mark.parametrize("v", ["verlet_ddt2_acc_lin_nograv", "symplectic_ddt1_damp_plane"])
def test_phase_loop_is_run(v):
    """Interaction_Forces carries the imposed accelerations, the Verlet update and the
    Symplectic corrector the damping: a phase-by-phase loop is sph_solver_run, bit for bit."""
    x = load_case(v)
    a, b = single(x), single(x)
    for done in (10, 20):
        a.run(10)
        step_by_phases(b, 10)
        same_bits(a, b, done)
    a.sync()
    # ... and neither is the run without the block
    setattr(x, "accinputs" if "acc" in v else "damping", [])
    c = single(x)
    c.run(20)
    assert not np.array_equal(by_idp(c.particles())["vel"], by_idp(a.particles())["vel"])


def test_an_input_on_the_first_fluid_block_leaves_the_second(tmp_path):
    """Through SphGpuSingle(XmlCase): mkfluid="0" of two fluid blocks (no bodies) gets the
    imposed part (-Gravity at t = 0: globalgravity false), mkfluid 1 keeps its bits."""
    from dualsphysics_multilayer_amd.xmlcase import XmlCase

    x = XmlCase(_edited(tmp_path, "verlet_ddt2_acc_lin_nograv", two_fluid_blocks))
    s = single(x)
    p, i1 = s.particles(), s.interaction()
    x.accinputs = []
    i0 = single(x).interaction()
    first, second = (p["idp"] >= 1182) & (p["idp"] < 1482), p["idp"] >= 1482
    assert first.sum() == 300 and second.sum() == 276
    assert np.array_equal(i1["ace"][~first], i0["ace"][~first]) and np.array_equal(i1["ar"], i0["ar"])
    d = i1["ace"][first].astype(np.float64) - i0["ace"][first].astype(np.float64)
    bound = 4 * ulp(np.maximum(np.abs(i1["ace"][first]), np.abs(i0["ace"][first])))
    want = np.array([0.0, 0.0, float(np.float32(9.81))])
    assert np.all(np.abs(d - want) <= bound)


def test_slab_face_inside_a_zone():
    """Two x-slabs of the off-lattice cloud (velocities up to 1 m/s, DtFixed) with a plane zone
    over the whole face region: particles cross the face while damped.  A particle that has just
    crossed is still its old slab's to damp (it migrates at the next divide, with the damped
    velocity); the velocities by idp are the single domain's.
    Tolerance: the two runs differ by the summation order of the interaction only, a few float
    ulps of |ace| <= ~600 m/s^2 per step (4 x 6e-5 m/s^2 x 2 dt = 1e-7 m/s), 10 steps, and ten
    times that for its feedback through the pressure: 1e-5 m/s.  One missed damping of a crosser
    is (1 - factor) |v| = 0.1 |v|."""
    import clouds
    from dualsphysics_multilayer_amd.core import SphSlabGroup, slab_partition

    dt, nsteps, tolv = 2e-4, 10, 1e-5
    base = copy.copy(clouds.make("uniform"))
    base.dtfixed = dt
    base.damping = [dict(type="plane", overlimit=10.0, redumax=500.0, factorxyz=[1.0, 1.0, 1.0],
                         limitmin=[-1.0, 0.0, 0.0], limitmax=[-0.99, 0.0, 0.0], dompt=None)]
    bounds = slab_partition(base, 2)
    grp, one = SphSlabGroup(base, bounds), single(base)
    own0 = set(grp.members[0].particles()["idp"].tolist())
    grp.run(nsteps)
    one.run(nsteps)
    one.sync()
    pg, p1 = grp.particles(), by_idp(one.particles())
    own1 = set(grp.members[0].particles()["idp"].tolist())
    fluid = p1["idp"] >= base.npb
    crossed = np.isin(p1["idp"], list(own0 ^ own1)) & fluid
    assert np.array_equal(pg["idp"], p1["idp"])
    # every fluid particle is damped by 1 - dt redumax = 0.9 per step (beyond limitmax: fdis = 1)
    fac, _ = damp(base.damping, dt, p1["pos"][fluid], np.ones((fluid.sum(), 3), np.float32))
    assert np.all(np.abs(fac - 0.9) < 1e-6)
    speed = np.abs(p1["vel"][crossed]).max(1)
    print("slab face in a zone: %d fluid particles changed slab (|v| %.3g .. %.3g), max |dvel| %.3g, max |dpos| %.3g" % (
        crossed.sum(), speed.min() if crossed.sum() else 0, speed.max() if crossed.sum() else 0,
        np.abs(pg["vel"] - p1["vel"]).max(), np.abs(pg["pos"] - p1["pos"]).max()))
    assert crossed.sum() >= 5 and np.sum(0.1 * speed > 100 * tolv) >= 5  # a missed damping would show
    assert np.abs(pg["vel"] - p1["vel"]).max() <= tolv
    grp.close()


ROWS2 = [[0.0, 1, 0, 0, 0, 0, 0], [1.0, 1, 0, 0, 0, 0, 0]]


def acc_dict(**kw):
    a = dict(code1=FLUID, code2=FLUID, globalgravity=True, timestart=0.0, timeend=1e30, centre=[0.0, 0.0, 0.0],
             rows=np.array(ROWS2, np.float64))
    a.update(kw)
    return a


PLANE = dict(type="plane", overlimit=0.03, redumax=2000.0, factorxyz=[1.0, 0.5, 8.0], limitmin=[0.1, 0.0, 0.0],
             limitmax=[0.25, 0.05, 0.0], dompt=None)


def test_refusals():
    from dualsphysics_multilayer_amd.case import DamBreakCase, WetDambreakNNCase
    from dualsphysics_multilayer_amd.core import SphError

    s = single(WetDambreakNNCase(0.025, width=0.2, scale=0.5))
    for call in (lambda: s.set_accinputs([acc_dict()]), lambda: s.set_damping([PLANE])):
        with pytest.raises(SphError, match="NN multiphase") as e:
            call()
        assert e.value.status == 7  # SPH_ERR_UNSUPPORTED
    for stepper in (lambda q: q.run(1), lambda q: step_by_phases(q, 1)):
        s = single(DamBreakCase(0.05))
        stepper(s)
        for call in (lambda: s.set_accinputs([acc_dict()]), lambda: s.set_damping([PLANE])):
            with pytest.raises(SphError, match="before the first step") as e:
                call()
            assert e.value.status == 3  # SPH_ERR_STATE
    s = single(DamBreakCase(0.05))
    with pytest.raises(SphError, match="less than two registers") as e:
        s.set_accinputs([acc_dict(rows=np.array(ROWS2[:1]))])
    assert e.value.status == 1  # SPH_ERR_ARG
    with pytest.raises(SphError, match="fluid blocks or floating bodies") as e:
        s.set_accinputs([acc_dict(code1=0, code2=0)])  # the fixed boundary
    assert e.value.status == 1
    with pytest.raises(SphError, match="more than 16") as e:
        s.set_accinputs([acc_dict(code1=FLUID | k, code2=FLUID | k) for k in range(17)])
    assert e.value.status == 7
    s.set_accinputs([acc_dict()])  # ... and once only
    with pytest.raises(SphError, match="once") as e:
        s.set_accinputs([acc_dict()])
    assert e.value.status == 3
    s.run(2)
    s.sync()


# ---- against float64 numpy ----------------------------------------------------------------------
class Coded:
    """A case with its own particle codes (the second mkfluid) and extra attributes."""

    explicit_codes = True

    def __init__(self, base, code=None, **kw):
        self._base = base
        self.code = np.ascontiguousarray(base.code if code is None else code, np.uint16)
        for k, v in kw.items():
            setattr(self, k, v)

    def __getattr__(self, k):
        return getattr(self._base, k)


def cloud(**kw):
    import clouds

    return clouds.make("uniform", small=True, **kw)


def ulp(x):
    """One float32 ulp at |x| (never below the smallest normal: a host that flushes denormals)."""
    return np.maximum(np.spacing(np.abs(np.asarray(x, np.float32))), np.finfo(np.float32).tiny)


def test_imposed_acceleration_term_by_term():
    base = cloud()
    gravity = np.asarray(base.case_def()["gravity"], np.float32)
    s0 = single(Coded(base))
    p0, i0 = s0.particles(), s0.interaction()
    fluid = p0["idp"] >= base.npb
    a2 = (i0["ace"].astype(np.float64) ** 2).sum(1)
    a2[~fluid] = -1
    top, second = np.argsort(a2)[-1], np.argsort(a2)[-2]
    amax, gap = np.sqrt(a2[top]), np.sqrt(a2[top]) - np.sqrt(a2[second])
    print("np %d fluid %d  |ace| max %.6g  second %.6g" % (len(fluid), fluid.sum(), amax, np.sqrt(a2[second])))
    assert gap > 400 * ulp(amax)  # (seed: the maximum stands clear of the rest by far more than the rounding)
    # the second mkfluid: a random half of the fluid that holds the particle of the maximum
    rng = np.random.default_rng(5)
    sel = fluid & (rng.random(len(fluid)) < 0.5)
    sel[top] = True
    code = np.where(base.idp >= base.npb, FLUID, 0).astype(np.uint16)
    code[p0["idp"][sel]] = FLUID | 1
    # rows 0-1: lin - Gravity = -c along the maximum's acceleration, so that it shrinks by less than
    # its lead over the second, and small angular rows; rows 2-3: every term of the size of |ace|
    c = gap / 4
    unit = i0["ace"][top].astype(np.float64) / amax
    lin = -c * unit + gravity.astype(np.float64)
    ang = 0.02 * c * np.array([1.0, -1.0, 0.5])
    rows = np.array([[0.0, *(0.5 * lin), *(0.5 * ang)], [1.0, *(1.5 * lin), *(1.5 * ang)],
                     [2.0, 30.0, -20.0, 15.0, 8.0, -6.0, 4.0], [3.0, 50.0, -10.0, 25.0, 4.0, -9.0, 7.0]])
    a = acc_dict(code1=FLUID | 1, code2=FLUID | 1, globalgravity=False, timestart=0.25, timeend=2.75,
                 centre=[0.1, 0.2, 0.05], rows=rows)
    s = single(Coded(base, code))
    pa = s.particles()
    assert np.array_equal(pa["idp"], p0["idp"]) and np.array_equal(pa["code"] == (FLUID | 1), sel)
    base_run = s.interaction()
    for k in ("ar", "ace"):  # the codes alone change nothing
        assert np.array_equal(base_run[k], i0[k])
    s.set_accinputs([a])
    # (1) inside the window, strictly between the two rows
    s.set_time(0.5)
    i1 = s.interaction()
    want = imposed_acc(a, 0.5, gravity, pa["pos"], pa["vel"])
    assert want is not None and np.abs(want[sel]).max() <= c * 1.5
    assert np.array_equal(i1["ar"], i0["ar"])  # bitwise, everywhere
    assert np.array_equal(i1["ace"][~sel], i0["ace"][~sel])  # exactly 0 on every other particle
    diff = i1["ace"][sel].astype(np.float64) - i0["ace"][sel].astype(np.float64)
    bound = 4 * ulp(np.maximum(np.abs(i1["ace"][sel]), np.abs(i0["ace"][sel])))
    err = np.abs(diff - want[sel].astype(np.float32).astype(np.float64))
    print("imposed: max |term| %.4g  worst error %.3g ulp-bounds" % (np.abs(want[sel]).max(), (err / bound).max()))
    assert np.all(err <= bound)
    assert np.abs(diff).max() > 0.5 * c  # the imposed part is really there
    # AceMax is the maximum of the final accelerations over [npb, np): smaller than without the
    # input here, so the interaction's slots were reset, not only raised
    m1 = np.sqrt((i1["ace"][fluid].astype(np.float64) ** 2).sum(1).max())
    print("acemax without %.9g with %.9g (own ace %.9g)" % (i0["acemax"], i1["acemax"], m1))
    assert abs(i1["acemax"] - m1) <= ulp(m1) and i1["acemax"] < i0["acemax"]
    assert abs(i0["acemax"] - amax) <= ulp(amax)
    # (2) outside the window: no change at all
    s.set_time(2.9)
    i2 = s.interaction()
    assert np.array_equal(i2["ace"], i0["ace"]) and np.array_equal(i2["ar"], i0["ar"]) and i2["acemax"] == i0["acemax"]
    # (3) between the last two rows: linear, angular, centripetal and Coriolis terms all of the
    # size of the pair sums (the velocities integrated over three rows), AceMax raised; then
    # (4) back between the first two (the lookup walks back): the bits of (1)
    s.set_time(2.5)
    i3 = s.interaction()
    want3 = imposed_acc(a, 2.5, gravity, pa["pos"], pa["vel"])
    diff3 = i3["ace"][sel].astype(np.float64) - i0["ace"][sel].astype(np.float64)
    bound3 = 4 * ulp(np.maximum(np.abs(i3["ace"][sel]), np.abs(i0["ace"][sel])))
    err3 = np.abs(diff3 - want3[sel].astype(np.float32).astype(np.float64))
    print("imposed at 2.5: |term| %.4g .. %.4g  worst error %.3g ulp-bounds" % (
        np.abs(want3[sel]).min(), np.abs(want3[sel]).max(), (err3 / bound3).max()))
    assert np.all(err3 <= bound3) and np.all(np.abs(want3[sel]).max(0) > 20)
    assert np.array_equal(i3["ace"][~sel], i0["ace"][~sel]) and np.array_equal(i3["ar"], i0["ar"])
    m3 = np.sqrt((i3["ace"][fluid].astype(np.float64) ** 2).sum(1).max())
    assert abs(i3["acemax"] - m3) <= ulp(m3)
    s.set_time(0.5)
    i4 = s.interaction()
    assert np.array_equal(i4["ace"], i1["ace"]) and i4["acemax"] == i1["acemax"]


DT = 1e-4
ZONES = {
    "plane": [PLANE],
    "plane_dom": [dict(PLANE, limitmax=[0.25, 0.0, 0.0], dompt=[[0.02, 0.03], [0.33, 0.2], [0.33, 0.03], [0.02, 0.2]],
                       domzmin=0.07, domzmax=0.22)],
    "box": [dict(type="box", overlimit=0.02, redumax=3000.0, factorxyz=[1.0, 1.0, 1.0], directions=63 ^ 16,  # all -front
                 limitmin_ini=[0.08, 0.06, 0.08], limitmin_end=[0.2, 0.2, 0.18], limitmax_ini=[0.02, 0.02, 0.04],
                 limitmax_end=[0.3, 0.26, 0.25])],
    "cyl_vertical": [dict(type="cylinder", overlimit=0.02, redumax=2500.0, factorxyz=[1.0, 1.0, 0.5], point1=[0.17, 0.14, 0.0],
                          point2=[0.17, 0.14, 1.0], radmin=0.03, radmax=0.1)],
    "cyl_oblique": [dict(type="cylinder", overlimit=0.02, redumax=2500.0, factorxyz=[1.0, 1.0, 1.0], point1=[0.05, 0.05, 0.05],
                         point2=[0.3, 0.25, 0.25], radmin=0.02, radmax=0.08)],
}
ZONES["overlap"] = ZONES["plane"] + ZONES["cyl_vertical"]


@pytest.fixture(scope="module")
def undamped():
    """One Verlet step (DtFixed) of the cloud without zones, and the case: shared, unchanged."""
    base = copy.copy(cloud())
    base.dtfixed = DT
    s = single(base)
    s.run(1)
    s.sync()
    p = s.particles()
    for a in p.values():
        a.setflags(write=False)
    return base, p


@pytest.mark.parametrize("name", list(ZONES))
def test_damping_bit_level(undamped, name):
    base, p0 = undamped
    zones = ZONES[name]
    s = single(Coded(base, damping=zones))
    s.run(1)
    s.sync()
    assert s.stats()["last_dt"] == DT
    p1 = s.particles()
    for k in ("idp", "pos", "rhop"):  # positions and densities are untouched, bit for bit
        assert np.array_equal(p1[k], p0[k]), k
    fluid = p0["idp"] >= base.npb
    want, near = damp(zones, DT, p0["pos"][fluid], p0["vel"][fluid])
    hit = np.any(want != p0["vel"][fluid], axis=1)
    print("%s: %d of %d fluid particles damped, closest approach to a limit %.3g m" % (name, hit.sum(), fluid.sum(), near.min()))
    assert near.min() > 1e-9  # precondition (seed): the float64 factor's branch is the device's
    assert hit.sum() > 50 and (~hit).sum() > 50
    if name == "overlap":  # ... and some particles by both zones, in sequence
        one = [np.any(damp([z], DT, p0["pos"][fluid], p0["vel"][fluid])[0] != p0["vel"][fluid], axis=1) for z in zones]
        assert (one[0] & one[1]).sum() > 20
    if name == "plane":  # the z factor is clamped at 0 in the zone's core
        assert (want[:, 2][hit] == 0).sum() > 10
    assert np.all(np.abs(p1["vel"][fluid].astype(np.float64) - want.astype(np.float64)) <= ulp(want))
    assert np.array_equal(p1["vel"][~fluid], p0["vel"][~fluid])
    assert np.array_equal(p1["vel"][fluid][~hit], p0["vel"][fluid][~hit])


def test_damping_leaves_velrhopm1():
    """The second Verlet step starts from the undamped VelrhopM1 (the initial velocity): its
    result is the numpy prediction from the one-step state, the interaction on it and the zones.
    The second step is driven by the phase calls from the downloaded interaction itself
    (sph_download_interaction leaves its ar / ace in place; DtFixed needs no maxima), so the
    prediction's accelerations are the update's own, bit for bit."""
    base = copy.copy(cloud())
    base.dtfixed = DT
    zones = ZONES["overlap"]
    s = single(Coded(base, damping=zones))
    s.run(1)
    p1, i1 = s.particles(), s.interaction()
    s.DtVariable(True)
    s.ComputeVerlet()
    s.RunCellDivide()
    s.sync()
    assert s.stats()["last_dt"] == DT and s.stats()["nstep"] == 2
    p2 = by_idp(s.particles())
    fluid = p1["idp"] >= base.npb
    keep = np.isin(p1["idp"], p2["idp"]) & fluid  # (none is excluded in two steps)
    assert keep.sum() == fluid.sum() and len(p2["idp"]) == len(p1["idp"])
    idp = p1["idp"][keep]
    g = np.asarray(base.case_def()["gravity"], np.float32).astype(np.float64)  # Gravity is a tfloat3
    vm1 = base.vel[idp].astype(np.float64)  # idp = the case's index
    pre = (vm1 + (i1["ace"][keep].astype(np.float64) + g) * (DT + DT)).astype(np.float32)  # ComputeVerletVarsFluid
    pos2 = p2["pos"][np.searchsorted(p2["idp"], idp)]
    want, near = damp(zones, DT, pos2, pre)
    assert near.min() > 1e-9
    got = p2["vel"][np.searchsorted(p2["idp"], idp)]
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp(want)
    hit2 = np.any(want != pre, axis=1)
    print("two steps: worst error %.3g ulp (%d entries above 1), %d damped" % (err.max(), (err > 1).sum(), hit2.sum()))
    assert np.all(err <= 1)
    # a damped VelrhopM1 would show: the zones of the first step reach many of these particles, by
    # factors far from 1
    f1 = damp(zones, DT, p1["pos"][keep], np.ones((keep.sum(), 3), np.float32))[0]
    assert (f1.min(1) < 0.9).sum() > 50


def test_symplectic_predictor_is_not_damped():
    base = copy.copy(cloud(step_algorithm=2, tdensity=1))
    base.dtfixed = DT
    a, b = single(base), single(Coded(base, damping=ZONES["overlap"]))
    for s in (a, b):
        s.Interaction_Forces(2)
        s.DtVariable(False)
        s.ComputeSymplecticPre()
    pa, pb = a.particles(), b.particles()
    for k in PART_KEYS:
        assert np.array_equal(pa[k], pb[k]), k
    for s in (a, b):  # ... the corrector is
        s.RunCellDivide()
        s.Interaction_Forces(3)
        s.DtVariable(True)
        s.ComputeSymplecticCorr()
        s.RunCellDivide()
    pa, pb = by_idp(a.particles()), by_idp(b.particles())
    assert np.array_equal(pa["pos"], pb["pos"]) and np.array_equal(pa["rhop"], pb["rhop"])
    fluid = pa["idp"] >= base.npb
    want, near = damp(ZONES["overlap"], b.stats()["last_dt"], pa["pos"][fluid], pa["vel"][fluid])
    assert near.min() > 1e-9 and np.any(want != pa["vel"][fluid])
    assert np.all(np.abs(pb["vel"][fluid].astype(np.float64) - want.astype(np.float64)) <= ulp(want))
