"""Inlet/outlet zones on the GPU (csrc/sph_inout.hip, the inout update of csrc/sph_step.hip).

* Reference PARTs: every fixture of tests/golden/make_inout.py through load_case and
  SphGpuSingle at PART 0 and each kept step: the idp set equal to the reference's (which
  particles were created, in which order, and which were removed), positions, velocities and
  densities within max(10 x noise, FLOOR) (noise: the reference's fast-math against its strict
  build; FLOOR of tests/test_dtopt.py), times within 1e-8 max(1, k), nout the reference's, and
  inout_stats() the growth of the ids.
* The extrapolation off the lattice (tests/inout_clouds.py): the velocity and density of the
  320 (2-D: 32) inout particles right after sph_solver_set_inout against the float64 numpy
  restatement of JSphCpu_InOut.cpp:55-237, in the modes 1, 2 and 3, with determlimit 1e-3
  (first order) and 1e+3 (zeroth order), within max(10 x e_ref, 4 x 2^-24) of the array maximum;
  e_ref: the error of the same restatement in that mode's number formats.  Nodes whose float64
  |determinant| lies within a factor 2 of determlimit are left out (at most 2 % of them).
* Two runs give the same bits; a capacity too small for a later creation stops the run; the
  core's refusals; the run driver's PARTs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import inout_clouds as ioc
from test_dtopt import FLOOR
from test_inout import VARIANTS, case_path, kept, load, ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def _gpu(case):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    return SphGpuSingle(case, device=0)


def _sorted(p):
    o = np.argsort(p["idp"], kind="stable")
    return {k: p[k][o] for k in ("idp", "pos", "vel", "rhop")}


# ---- reference PARTs ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("v", sorted(VARIANTS))
def test_gpu_matches_reference_parts(v):
    x, g = load(v), ref(v)
    s = _gpu(x)
    n0 = int(g["case_np"])
    ninit = len(x.inout["init"]["idp"])
    done = 0
    worst = []
    for k in kept(g):
        s.run(k - done)
        s.sync()
        done = k
        p, st, io = _sorted(s.particles()), s.stats(), s.inout_stats()
        assert np.array_equal(p["idp"], g["s%d_idp" % k]), "step %d: other particles exist" % k
        noise = g["noise_%d" % k]
        tol = [max(10.0 * float(noise[i]), FLOOR[i]) for i in range(3)]
        d = (np.abs(p["pos"] - g["s%d_pos" % k]).max(), np.abs(p["vel"] - g["s%d_vel" % k]).max(),
             np.abs(p["rhop"].astype(np.float64) - g["s%d_rhop" % k]).max())
        worst.append(max(d[i] / tol[i] for i in range(3)))
        print("%s step %d: distance / tolerance pos %.3f vel %.3f rhop %.3f" % ((v, k) + tuple(d[i] / tol[i] for i in range(3))))
        for i, q in enumerate(("pos", "vel", "rhop")):
            assert d[i] <= tol[i], (k, q, d[i], tol[i])
        assert abs(st["time"] - float(g["s%d_time" % k])) <= 1e-8 * max(1, k)
        assert st["nout"] == int(g["s%d_nout" % k]) and st["np"] == len(p["idp"]) and st["nstep"] == k
        # the ids grow with the particles created: IdMax and the creation count
        assert io["idmax"] == int(g["idmaxs"][k]) and io["created"] == int(g["idmaxs"][k]) - (n0 + ninit - 1)
        assert io["capacity"] == n0 + ninit + x.inout["npresizeplus0"]
        # every particle that left was dropped or removed by a zone's rules
        assert io["removed"] == n0 + ninit + io["created"] - st["np"]
        assert 0 < io["count"] <= st["np"] - x.npb
    s.close()
    print("%s worst distance / tolerance %.3f" % (v, max(worst)))


@gpu
def test_two_runs_give_the_same_bits():
    out = []
    for _ in range(2):
        s = _gpu(load("3d_verlet_ddt2_extrap"))
        s.run(100)
        s.sync()
        out.append(s.particles())  # device order
        s.close()
    for q in ("idp", "pos", "vel", "rhop", "code"):
        assert np.array_equal(out[0][q], out[1][q]), q


# ---- the extrapolation off the lattice -------------------------------------------------------
CLOUDS = [(two_d, mode, dl) for two_d in (False, True) for mode in (1, 2, 3) for dl in (1e-3, 1e3)]
_REF = {}


def _reference(two_d, dl):
    """The float64 restatement, once per cloud and determlimit."""
    if (two_d, dl) not in _REF:
        c = ioc.make(two_d, 3, dl)
        vel, rho, det, first = ioc.extrap(c)
        for a in (vel, rho, det, first):
            a.setflags(write=False)
        _REF[(two_d, dl)] = (vel, rho, det, first)
    return _REF[(two_d, dl)]


@pytest.mark.parametrize("two_d", (False, True))
def test_cloud_reaches_both_branches(two_d):
    from dualsphysics_multilayer_amd._abi import inout_arrays

    n = 4 * 8 * (1 if two_d else 10)
    # the cloud's hand-made zone is a valid input of sph_solver_set_inout: n / 4 points, 4 layers
    d, zones, points = inout_arrays(ioc.make(two_d, 1, 1e-3).inout)
    assert d.nzones == 1 and zones[0].npoints == n // 4 == len(points) and zones[0].layers == 4
    _, _, det, first = _reference(two_d, 1e-3)
    assert len(det) == n and first.all()  # |det| >= 1e-3 everywhere: the first-order mirror
    near = (np.abs(det) > 0.5e-3) & (np.abs(det) < 2e-3)
    assert near.sum() <= 0.02 * n
    _, _, det, first = _reference(two_d, 1e3)
    assert not first.any() and (np.abs(det) < 0.5e3).all()  # the zeroth-order values


@gpu
@pytest.mark.parametrize("two_d,mode,dl", CLOUDS)
def test_extrapolation_on_clouds(two_d, mode, dl):
    c = ioc.make(two_d, mode, dl)
    rvel, rrho, det, first = _reference(two_d, dl)
    S, M = ioc.MODE_FORMATS[mode]
    mvel, mrho, _, mfirst = ioc.extrap(c, sums=S, matrix=M, kernel=np.float32)
    keep = ~((np.abs(det) > 0.5 * dl) & (np.abs(det) < 2 * dl))
    assert (~keep).sum() <= 0.02 * len(det) and np.array_equal(mfirst[keep], first[keep])
    s = _gpu(c)
    p = _sorted(s.particles())
    s.close()
    sel = p["idp"] >= c.np
    assert np.array_equal(p["idp"][sel], c.inout["init"]["idp"])
    assert np.array_equal(p["pos"][sel], c.inout["init"]["pos"])
    gvel, grho = p["vel"][sel].astype(np.float64), p["rhop"][sel].astype(np.float64)
    for name, got, want, own in (("vel", gvel, rvel, mvel), ("rhop", grho, rrho, mrho)):
        scale = np.abs(want[keep]).max()
        e_ref = np.abs(own[keep] - want[keep]).max() / scale
        err = np.abs(got[keep] - want[keep]).max() / scale
        bound = max(10.0 * e_ref, 4 * 2.0 ** -24)
        print("cloud 2d=%s mode %d determlimit %g %s: err %.2e e_ref %.2e bound %.2e" % (two_d, mode, dl, name, err, e_ref, bound))
        assert err <= bound, (name, err, bound)
    # the values are not the initial ones: the kernel ran
    assert (grho != 1000).all() and (np.abs(gvel[:, 0]) > 0).all()


# ---- capacity ----------------------------------------------------------------------------------
class _WithCapacity:
    """A loaded case with an explicit particle capacity for its zones."""

    def __init__(self, case, capacity):
        self.__dict__.update(case.__dict__)
        self._case, self.inout_capacity = case, capacity

    def __getattr__(self, k):
        return getattr(self._case, k)


@gpu
def test_capacity_exceeded_stops_the_run():
    from dualsphysics_multilayer_amd._abi import SPH_FLAG_INOUT_FULL
    from dualsphysics_multilayer_amd.core import SphError

    v = "2d_verlet_ddt3_fixed"
    x, g = load(v), ref(v)
    n0, ninit, column = x.np, len(x.inout["init"]["idp"]), int(g["column"])
    # one particle short of a column: the first column the inlet creates does not fit (the
    # particles the outlet drops in the same pass hold their slots until the sort)
    s = _gpu(_WithCapacity(x, n0 + ninit + column - 1))
    s.run(150)
    with pytest.raises(SphError, match="SPH_ERR_NOMEM.*new inlet particles"):
        s.sync()
    st, io = s.stats(), s.inout_stats()
    assert st["error_flags"] & SPH_FLAG_INOUT_FULL
    k = int(st["nstep"])
    assert 0 < k < 150 and io["created"] == 0 and io["capacity"] == n0 + ninit + column - 1
    got = _sorted(s.particles())
    s.close()
    # the last valid state: the same case with head-room after the k steps the run took, without
    # the column that did not fit (the zones' rules and the imposed data of step k were applied)
    r = _gpu(x)
    r.run(k)
    r.sync()
    assert r.inout_stats()["created"] == column and r.stats()["error_flags"] == 0
    want = _sorted(r.particles())
    r.close()
    new = ~np.isin(want["idp"], got["idp"])
    assert new.sum() == column and (want["idp"][new] > n0 + ninit - 1).all()
    for q in ("idp", "pos", "vel", "rhop"):
        assert np.array_equal(got[q], want[q][~new]), q


# ---- refusals ---------------------------------------------------------------------------------
class _Over:
    """A case whose case_def() is another's with some fields replaced."""

    def __init__(self, case, **kw):
        self.__dict__.update(case.__dict__)
        self._case, self._kw = case, kw

    def __getattr__(self, k):
        return getattr(self._case, k)

    def case_def(self):
        return dict(self._case.case_def(), **self._kw)


@gpu
def test_core_refuses_unsupported_combinations():
    from dualsphysics_multilayer_amd.core import SphError, SphGpuSingle, SphSlabGroup, load_library

    from dualsphysics_multilayer_amd import _abi
    from dualsphysics_multilayer_amd.case import NN_EXAMPLE_PHASES
    from dualsphysics_multilayer_amd.core import SphGpuSlab, _check, case_derive

    x = load("3d_verlet_ddt2_extrap")
    mdbc = _Over(x, tboundary=2)
    mdbc.boundnormal = np.full((x.np, 3), 0.01, np.float32)
    lo = x.case_def()["map_realposmin"]
    for case, msg in ((_Over(x, tvisco=2), "Laminar.SPS or shifting"),
                      (_Over(x, shift_mode=1, shift_coef=-2.0), "Laminar.SPS or shifting"),
                      (_Over(x, kernel=1), "Cubic spline kernel"), (_Over(x, peri_active=1), "periodic boundaries"),
                      (mdbc, "mDBC"),
                      (_Over(x, symmetry=1, map_realposmin=(lo[0], 0.0, lo[2])), "Symmetry"),  # (the mirror plane y = 0)
                      (_Over(x, rheology=2, nphases=1, phases=(dict(NN_EXAMPLE_PHASES[2], mkfluid=0),)), "NN multiphase")):
        with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*inlet/outlet zones with.*" + msg) as ei:
            SphGpuSingle(case, device=0)
        assert ei.value.status == 7
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*slab solvers"):
        SphSlabGroup(x, [0, 8, 16], devices=[0, 0])
    # a slab solver of its own (one rank over the shared-memory transport): refused by the binding
    # for a case with zones, and by the core when the zones are handed to it directly
    ncx = int(case_derive(x.case_def())["dom_cells"][0])
    shm = dict(transport="shm", slot_bytes=1 << 20)
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*slab solvers"):
        SphGpuSlab(x, 0, 1, [0, ncx], "/sph_inout_refused_a_%d" % os.getpid(), **shm)
    y = load("3d_verlet_ddt2_extrap")
    io, y.inout = y.inout, None
    sl = SphGpuSlab(y, 0, 1, [0, ncx], "/sph_inout_refused_b_%d" % os.getpid(), **shm)
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*not implemented for slab solvers"):
        sl.set_inout(io)
    sl.close()
    s = _gpu(x)
    L = load_library()
    # only sph_solver_run steps a solver with zones
    for call in (lambda: s.RunCellDivide(), lambda: s.Interaction_Forces(1), lambda: s.DtVariable(True),
                 lambda: s.ComputeVerlet(), lambda: s.ComputeSymplecticPre(), lambda: s.ComputeSymplecticCorr()):
        with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*phase-level calls"):
            call()
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*restart not allowed"):
        s.set_time(0.1)
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*gauges with inlet/outlet"):
        s.set_gauges([dict(type="velocity", output=True, computestart=0, computeend=1, computedt=0, outputstart=0,
                           outputend=1, outputdt=0, point0=(0.2, 0.1, 0.05))])
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*moving boundaries with inlet/outlet"):
        _check(L.sph_solver_set_motion(s._h, 1, 0, None, 0, None))
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*floating bodies with inlet/outlet"):
        _check(L.sph_solver_set_floatings(s._h, 1, (_abi.SphFloatingDef * 1)(), 0.0))
    with pytest.raises(SphError, match="SPH_ERR_STATE.*already configured"):
        s.set_inout(x.inout)
    s.run(1)
    s.sync()
    s.close()
    # after a step: SPH_ERR_STATE
    y = load("3d_verlet_ddt2_extrap")
    io, y.inout = y.inout, None
    s = _gpu(y)
    s.run(1)
    s.sync()
    with pytest.raises(SphError, match="SPH_ERR_STATE.*before the first step"):
        s.set_inout(io)
    with pytest.raises(SphError, match="SPH_ERR_STATE.*no inlet/outlet zones"):
        s.inout_stats()
    s.close()
    assert L.sph_solver_set_inout(None, None, None, None, 0) == 1  # SPH_ERR_ARG


# ---- InitCheckProximity in the core ------------------------------------------------------------
def _shifted_inlet(tmp_path):
    """The 2-D fixture with the inlet's points half a dp from the first fluid column."""
    from test_inout import V2, _edit

    return load_case_path(_edit(tmp_path, V2, '<point x="-0.02" z="0.02"/><point2 x="-0.02" z="0.24"/>',
                                '<point x="-0.01" z="0.02"/><point2 x="-0.01" z="0.24"/>'))


def load_case_path(path):
    from dualsphysics_multilayer_amd.xmlcase import load_case

    return load_case(path)


@gpu
def test_core_excludes_the_fluid_next_to_the_zones(tmp_path):
    from dualsphysics_multilayer_amd.core import SphError

    x = _shifted_inlet(tmp_path)
    out = x.inout["outignore"]
    assert len(out) == 12  # the loader's own check (tests/test_inout.py)
    s = _gpu(x)
    p, st = _sorted(s.particles()), s.stats()
    # the core's pass dropped the same 12 fluid particles, uncounted, and holds every other one
    want = np.sort(np.concatenate([np.delete(x.idp, out), x.inout["init"]["idp"]]))
    assert np.array_equal(p["idp"], want) and st["np"] == len(want) and st["nout"] == 0
    s.run(3)
    s.sync()
    assert s.stats()["np"] == len(want) and s.stats()["error_flags"] == 0
    s.close()
    # a boundary particle that close: the inlet's points moved down to the floor's level
    y = _shifted_inlet(tmp_path)
    io, y.inout = y.inout, None
    s = _gpu(y)
    bad = dict(io, zones=[dict(z) for z in io["zones"]])
    bad["zones"][0]["points"] = io["zones"][0]["points"] + np.array([0.0, 0.0, -0.02])
    with pytest.raises(SphError, match="SPH_ERR_ARG.*too close to inout particles") as ei:
        s.set_inout(bad)
    assert ei.value.status == 1
    # points outside the domain: refused before anything changed, so the valid zones still go in
    bad["zones"][0]["points"] = io["zones"][0]["points"] + np.array([-10.0, 0.0, 0.0])
    with pytest.raises(SphError, match="SPH_ERR_ARG.*outside the domain"):
        s.set_inout(bad)
    assert s.stats()["np"] == y.np
    s.set_inout(io)
    assert np.array_equal(_sorted(s.particles())["idp"], want)
    s.close()


# ---- the run driver ---------------------------------------------------------------------------
@gpu
def test_driver_writes_the_reference_particles(tmp_path):
    from dualsphysics_multilayer_amd.core import read_part

    v = "2d_verlet_ddt3_fixed"
    g = ref(v)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "dualsphysics_multilayer_amd", case_path(v), str(tmp_path / "out"),
                    "-nsteps:75", "-svsteps:1", "-saveposdouble:1", "-sv:binx"], check=True, env=env,
                   cwd=str(tmp_path), timeout=120)
    for k in (0, 1, 75):
        h, p = read_part(os.path.join(str(tmp_path / "out"), "Part_%04u.bi4" % k))
        assert h["npok"] == len(g["s%d_idp" % k]) and np.array_equal(np.sort(p["idp"]), g["s%d_idp" % k])
        assert abs(h["timestep"] - float(g["times"][k])) <= 1e-8 * max(1, k)
