"""Periodic boundaries on the GPU (csrc/sph_periodic.hip, the wrap of update_pos).

* Reference PARTs: every fixture of tests/golden/make_periodic.py (the REFERENCE DualSPHysics
  v5.2 CPU solver on cases of case.py PeriodicChannelCase) through load_case and SphGpuSingle:
  every kept PART within max(10 x noise, FLOOR) of the reference's (noise: its fast-math against
  its strict build; FLOOR of tests/test_dtopt.py), the idp sets equal, nout the reference's,
  times within 1e-8 max(1, k); the restart fixture from the reference's own PART.
* Interaction on the periodic clouds (tests/periodic_clouds.py), DDT 0-3, both cell modes: the
  originals' ar and ace against clouds.brute on the explicit-image cloud within 10 x e_ref
  (e_ref: the oracle's own error on that cloud, over the originals), against the oracle on it
  within 1e-5 of the array maximum, and BIT FOR BIT what the plain solver computes on the
  explicit-image cloud (the duplicates sort into the same cells in the same order), in the same
  device order; the duplicate counts are numpy's; a translated and wrapped cloud gives the same
  values within the sum of the two runs' bounds.
* Stepping off the lattice with DtFixed until particles wrap on both axes; the phase calls
  against run() bit for bit; a capacity too small for a later divide; the refused combinations;
  the run driver's PART headers.

Verlet and the duplicates: the reference's ComputeVerletVarsFluid updates a duplicate like any
particle (only the Symplectic update skips them, JSphCpu.cpp:1488,1590); the core does the same.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clouds
import periodic_clouds as pc
from golden_io import maxdiff
from test_dtopt import FLOOR
from test_periodic import FIX, VARIANTS, case_path, fixture_case, fixture_ref, kept

pytestmark = pytest.mark.gpu

MARGIN = 10.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu(case):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    return SphGpuSingle(case, device=0)


def _K(case):
    from dualsphysics_multilayer_amd.core import case_derive

    return case_derive(case.case_def())


# ---- reference PARTs ------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS)
def test_gpu_matches_reference_parts(v):
    x, g = fixture_case(v), fixture_ref(v)
    first = int(g["first"])
    s = _gpu(x)
    if first:
        s.set_time(x.time0, x.symdtpre0)
    done = first
    for k in kept(g):
        s.run(k - done)
        done = k
        got = s.particles()
        o = np.argsort(got["idp"], kind="stable")
        got = {q: got[q][o] for q in ("idp", "pos", "vel", "rhop")}
        ref = {q: g["s%d_%s" % (k, q)] for q in ("idp", "pos", "vel", "rhop")}
        n = g["noise_%d" % k]
        tol = tuple(max(10.0 * float(n[i]), FLOOR[i]) for i in range(3))
        st = s.stats()
        d = [maxdiff(got, ref, q) if len(got["idp"]) == len(ref["idp"]) else np.inf for q in ("pos", "vel", "rhop")]
        print("%s PART %d: dpos %.3e (tol %.3e) dvel %.3e (%.3e) drho %.3e (%.3e) dt %.3e nout %d npbper %d npfper %d"
              % (v, k, d[0], tol[0], d[1], tol[1], d[2], tol[2], abs(st["time"] - float(g["times"][k - first])),
                 st["nout"], st["npbper"], st["npfper"]))
        assert np.array_equal(got["idp"], ref["idp"]), "excluded/duplicated particles"
        assert st["np"] == len(ref["idp"]) and st["nout"] == int(g["s%d_nout" % k])
        assert d[0] <= tol[0] and d[1] <= tol[1] and d[2] <= tol[2], (k, d, tol)
        assert abs(st["time"] - float(g["times"][k - first])) <= 1e-8 * max(1, k)
        assert st["npfper"] > 0 and st["error_flags"] == 0
    s.close()


# ---- interaction on the periodic clouds -------------------------------------------------------
def _interaction(case):
    """interaction() of a fresh solver into NaN-seeded buffers + its particles and stats."""
    from dualsphysics_multilayer_amd._abi import SphInterOut
    from dualsphysics_multilayer_amd.core import _check, load_library

    g = _gpu(case)
    n = g.stats()["np"]
    ar = np.full(n, np.nan, np.float32)
    ace = np.full((n, 3), np.nan, np.float32)
    out = SphInterOut(ar.ctypes.data_as(C.POINTER(C.c_float)), ace.ctypes.data_as(C.POINTER(C.c_float)), 0, 0, 0)
    _check(load_library().sph_download_interaction(g._h, C.byref(out)))
    res = dict(ar=ar, ace=ace, acemax=out.acemax, idp=g.particles()["idp"], stats=g.stats())
    g.close()
    return res


def _errs(ar, ace, ref_ar, ref_ace, keep):
    """max |d| over the originals, relative to the originals' maximum of the reference."""
    return (float(np.abs(ar - ref_ar)[keep].max() / np.abs(ref_ar).max()),
            float(np.abs(ace - ref_ace).max() / np.abs(ref_ace).max()))


_CACHE = {}


def cloud_run(name, ddt, cellmode, shift=None):
    """Everything one periodic cloud needs, once: the periodic solver's interaction (by idp),
    the float64 reference and the oracle on the explicit-image cloud (originals, by idp), their
    errors, the plain solver on the explicit-image cloud."""
    key = (name, ddt, cellmode, shift)
    if key in _CACHE:
        return _CACHE[key]
    import oracle.pyoracle  # noqa: F401  (clouds.oracle_floor; a broken oracle fails these tests only)

    case = pc.make(name, tdensity=ddt, cellmode=cellmode, shift=shift)
    K = _K(case)
    e, orig, info = pc.extended(case, K)
    Ke = _K(e)
    ref = clouds.brute(e, Ke, ddt)
    assert not ref["shell"].any() and not ref["amb"].any()
    fast, strict, _ = clouds.oracle_floor(e, ref, ddt)
    ref_ar, ref_ace = ref["ar"][orig], ref["ace"][orig]
    keep = np.ones(case.np, bool)
    e_ref = [0.0, 0.0]
    for run in (fast, strict):  # the oracle's error over the originals, the larger of its two builds
        by = np.empty(e.np, np.int64)
        by[run["idp"]] = np.arange(e.np)
        ea, ec = _errs(run["ar"][by][orig].astype(np.float64), run["ace"][by][orig].astype(np.float64), ref_ar, ref_ace,
                       keep)
        e_ref = [max(e_ref[0], ea), max(e_ref[1], ec)]
    by = np.empty(e.np, np.int64)
    by[fast["idp"]] = np.arange(e.np)
    ora = dict(ar=fast["ar"][by][orig], ace=fast["ace"][by][orig])
    ig = _interaction(case)
    assert not np.isnan(ig["ar"]).any() and not np.isnan(ig["ace"]).any()
    gp = np.empty(case.np, np.int64)
    gp[ig["idp"]] = np.arange(case.np)
    gpu = dict(ar=ig["ar"][gp], ace=ig["ace"][gp])
    out = dict(case=case, e=e, orig=orig, info=info, ref_ar=ref_ar, ref_ace=ref_ace, e_ref=e_ref, ora=ora, gpu=gpu,
               ig=ig)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("ddt", [0, 1, 2, 3])
@pytest.mark.parametrize("name", pc.NAMES)
def test_periodic_cloud_interaction(name, ddt, cellmode):
    r = cloud_run(name, ddt, cellmode)
    case, e, orig, info, ig = r["case"], r["e"], r["orig"], r["info"], r["ig"]
    keep = np.ones(case.np, bool)
    g_ar, g_ace = _errs(r["gpu"]["ar"].astype(np.float64), r["gpu"]["ace"].astype(np.float64), r["ref_ar"],
                        r["ref_ace"], keep)
    o_ar = float(np.abs(r["gpu"]["ar"] - r["ora"]["ar"]).max() / np.abs(r["ora"]["ar"]).max())
    o_ace = float(np.abs(r["gpu"]["ace"] - r["ora"]["ace"]).max() / np.abs(r["ora"]["ace"]).max())
    st = ig["stats"]
    print("periodic %s ddt %d cellmode %d: vs brute ar %.2e ace %.2e | e_ref ar %.2e ace %.2e | vs oracle ar %.2e ace "
          "%.2e | np %d dups %d + %d (numpy %d + %d)" % (name, ddt, cellmode, g_ar, g_ace, r["e_ref"][0], r["e_ref"][1],
                                                         o_ar, o_ace, st["np"], st["npbper"], st["npfper"],
                                                         info["nbound"], info["nfluid"]))
    # counts: normal particles only; the duplicates are numpy's
    assert (st["np"], st["npb"], st["npbok"], st["nout"]) == (case.np, case.npb, case.npb, 0)
    assert (st["npbper"], st["npfper"]) == (info["nbound"], info["nfluid"])
    assert np.array_equal(np.sort(ig["idp"]), case.idp)
    # against the float64 sum and the oracle on the explicit-image cloud
    assert g_ar <= MARGIN * r["e_ref"][0], (g_ar, r["e_ref"][0])
    assert g_ace <= MARGIN * r["e_ref"][1], (g_ace, r["e_ref"][1])
    assert o_ar <= 1e-5 and o_ace <= 1e-5, (o_ar, o_ace)
    # the plain solver on the explicit-image cloud: the originals bit for bit, in the same order
    ip = _interaction(e)
    isorig = np.full(e.np, -1, np.int64)
    isorig[orig] = np.arange(case.np)  # explicit-image idp -> the original's idp
    sel = isorig[ip["idp"]] >= 0
    assert np.array_equal(isorig[ip["idp"]][sel], ig["idp"].astype(np.int64)), "device order of the originals"
    assert np.array_equal(ip["ar"][sel].view(np.uint32), ig["ar"].view(np.uint32))
    assert np.array_equal(ip["ace"][sel].view(np.uint32), ig["ace"].view(np.uint32))
    # AceMax is over the normal particles only
    a2 = (ig["ace"].astype(np.float32) ** 2).sum(axis=1)[ig["idp"] >= case.npb].max()
    assert ig["acemax"] == pytest.approx(float(np.sqrt(a2)), rel=1e-6)


@pytest.mark.parametrize("cellmode", [1, 2])
def test_periodic_cloud_translation(cellmode):
    """The xy cloud shifted by a vector that is no cell multiple and wrapped: the same periodic
    system in other cells, other duplicates.  ar and ace by idp agree within the sum of the two
    runs' bounds against the float64 sum."""
    a = cloud_run("xy", 2, cellmode)
    cs = float(np.float32(_K(a["case"])["scell"]))
    b = cloud_run("xy", 2, cellmode, shift=(0.37 * cs, -0.61 * cs, 0.0))
    assert b["info"]["src"].tolist() != a["info"]["src"].tolist()  # other particles are duplicated
    bound_ar = MARGIN * (a["e_ref"][0] + b["e_ref"][0]) * np.abs(a["ref_ar"]).max()
    bound_ace = MARGIN * (a["e_ref"][1] + b["e_ref"][1]) * np.abs(a["ref_ace"]).max()
    d_ar = np.abs(a["gpu"]["ar"].astype(np.float64) - b["gpu"]["ar"]).max()
    d_ace = np.abs(a["gpu"]["ace"].astype(np.float64) - b["gpu"]["ace"]).max()
    print("translation cellmode %d: d ar %.3e (bound %.3e) d ace %.3e (bound %.3e)" % (cellmode, d_ar, bound_ar, d_ace,
                                                                                      bound_ace))
    assert d_ar <= bound_ar and d_ace <= bound_ace


# ---- stepping off the lattice -----------------------------------------------------------------
DT, NSTEPS = 1.5e-4, 40


def _stepping_case(step_algorithm):
    c = pc.make("xy", tdensity=1 if step_algorithm == 2 else 2, step_algorithm=step_algorithm, vamp=2.0, rhoamp=0.004)
    c.dtfixed = DT
    # z is not periodic and the cloud fills the box to its top: one cell of head-room, so that
    # no particle leaves the map there (the periods in x and y stay)
    lo, hi = c.map_limits()
    c._map = (lo, hi + np.array([0.0, 0.0, 0.07]))
    c._cloud_key = None
    return c


@pytest.mark.parametrize("step_algorithm", [1, 2])
def test_stepping_wraps_and_phases_match_run(step_algorithm):
    from test_gpu_phases import same_bits, step_by_phases

    case = _stepping_case(step_algorithm)
    lo, hi = case.map_limits()
    a, b = _gpu(case), _gpu(case)
    npbper = a.stats()["npbper"]
    assert npbper > 0
    for _ in range(4):
        a.run(NSTEPS // 4)
        step_by_phases(b, NSTEPS // 4)
        same_bits(a, b, "periodic phases vs run")
        st = a.stats()
        assert st["npbper"] == npbper and st["npfper"] > 0  # the boundary is at rest
        assert st["nout"] == 0 and st["error_flags"] == 0 and st["np"] == case.np
    p = a.particles()
    assert np.array_equal(np.sort(p["idp"]), case.idp)
    o = np.argsort(p["idp"])
    pos = p["pos"][o]
    for ax in (0, 1):  # every normal particle inside the real map on the periodic axes
        assert (pos[:, ax] >= lo[ax]).all() and (pos[:, ax] < hi[ax]).all()
    jump = np.abs(pos - case.pos) > 0.5 * (hi - lo)
    print("stepping algorithm %d: wrapped x %d y %d, time %.6f" % (step_algorithm, jump[:, 0].sum(), jump[:, 1].sum(),
                                                                  a.stats()["time"]))
    assert jump[:, :2].any(axis=1).sum() >= 20 and jump[:, 0].sum() >= 5 and jump[:, 1].sum() >= 5
    if step_algorithm == 1:  # (the first Symplectic step runs with DtIni, JSphCpuSingle.cpp:696)
        assert a.stats()["time"] == pytest.approx(NSTEPS * DT, rel=1e-12)
    a.close()
    b.close()


# ---- capacity ---------------------------------------------------------------------------------
def _drift_case():
    """The x cloud with its fluid kept more than the interaction distance from both x faces (no
    fluid duplicate at creation), drifting towards the +x face."""
    c = pc.make("x", tdensity=2)
    K = _K(c)
    ks = float(np.float32(K["kernelsize"]))
    lo, hi = c.map_limits()
    x = c.pos[:, 0]
    keep = (np.arange(c.np) < c.npb) | ((x > lo[0] + 1.2 * ks) & (x < hi[0] - 1.08 * ks))
    c.pos, c.vel, c.rhop = c.pos[keep].copy(), c.vel[keep].copy(), c.rhop[keep].copy()
    c.np = int(keep.sum())
    c.idp = np.arange(c.np, dtype=np.uint32)
    c.vel[c.npb:] = (3.0, 0.0, 0.0)
    c.dtfixed = DT
    c._map = (lo, hi + np.array([0.0, 0.0, 0.07]))  # head-room at the top (z is not periodic)
    c._cloud_key = None
    return c


def test_capacity_exceeded_stops_the_run(monkeypatch):
    from dualsphysics_multilayer_amd._abi import SPH_FLAG_PERIODIC_FULL
    from dualsphysics_multilayer_amd.core import SphError

    case = _drift_case()
    monkeypatch.setenv("SPH_PERI_MINCAP", "1")  # read at creation
    s = _gpu(case)
    monkeypatch.delenv("SPH_PERI_MINCAP")
    st0 = s.stats()
    assert st0["npfper"] == 0 and st0["npbper"] > 0
    s.run(60)
    with pytest.raises(SphError, match="SPH_ERR_NOMEM.*periodic duplicates"):
        s.sync()
    st = s.stats()
    assert st["error_flags"] & SPH_FLAG_PERIODIC_FULL
    k = int(st["nstep"])
    # (y is not periodic: a particle may leave the map there, as in the run with head-room below)
    assert 0 < k < 60 and st["np"] + st["nout"] == case.np
    got = s.particles()
    s.close()
    # the last valid state: the same case with head-room after the k steps the run completed
    r = _gpu(case)
    r.run(k)
    r.sync()
    assert r.stats()["npfper"] > 0 and r.stats()["error_flags"] == 0 and r.stats()["nout"] == st["nout"]
    ref = r.particles()
    r.close()
    og, orf = np.argsort(got["idp"]), np.argsort(ref["idp"])
    for q in ("idp", "pos", "vel", "rhop"):
        assert np.array_equal(got[q][og], ref[q][orf]), q


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


def _refused(make):
    from dualsphysics_multilayer_amd.core import SphError

    with pytest.raises(SphError, match="(?i)SPH_ERR_UNSUPPORTED.*periodic") as ei:
        make()
    assert ei.value.status == 7


def test_refused_combinations():
    from dualsphysics_multilayer_amd import _abi
    from dualsphysics_multilayer_amd.case import NN_EXAMPLE_PHASES
    from dualsphysics_multilayer_amd.core import SphGpuSlab, SphSlabGroup, _check, load_library, slab_partition

    base = pc.make("x", tdensity=2)
    _refused(lambda: SphSlabGroup(base, slab_partition(base, 2)))
    # a slab solver of its own (one rank over the shared-memory transport)
    ncx = int(_K(base)["dom_cells"][0])
    _refused(lambda: SphGpuSlab(base, 0, 1, [0, ncx], "/sph_periodic_refused_%d" % os.getpid(), transport="shm",
                                slot_bytes=1 << 20))
    mdbc = _Over(base, tboundary=2)
    mdbc.boundnormal = np.full((base.np, 3), 0.01, np.float32)
    _refused(lambda: _gpu(mdbc))
    _refused(lambda: _gpu(_Over(base, rheology=2, nphases=1, phases=(NN_EXAMPLE_PHASES[0],))))
    _refused(lambda: _gpu(_Over(base, tvisco=2, visco=1e-6)))
    _refused(lambda: _gpu(_Over(base, shift_mode=3)))
    _refused(lambda: _gpu(_Over(base, symmetry=1)))
    s = _gpu(base)
    L = load_library()
    _refused(lambda: _check(L.sph_solver_set_motion(s._h, 1, 0, None, 0, None)))
    ft = (_abi.SphFloatingDef * 1)()
    _refused(lambda: _check(L.sph_solver_set_floatings(s._h, 1, ft, 0.0)))
    gd = (_abi.SphGaugeDef * 1)()
    _refused(lambda: _check(L.sph_solver_set_gauges(s._h, 1, gd, 16)))
    s.close()


# ---- the run driver ---------------------------------------------------------------------------
def test_driver_writes_periodic_part_headers(tmp_path):
    from dualsphysics_multilayer_amd.core import read_part

    g = fixture_ref("x_verlet_ddt2")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = ["-nsteps:2", "-svsteps:1", "-saveposdouble:1", "-sv:binx"]
    runs = [([case_path("x_verlet_ddt2"), str(tmp_path / "a")], 2),
            # -partbegin on a periodic case: from the reference's PART 25
            ([case_path("x_verlet_ddt2_restart"), str(tmp_path / "b"), "-partbegin:25",
              os.path.join(FIX, "periodic_x_verlet_ddt2_restart")], 27)]
    for argv, last in runs:
        subprocess.run([sys.executable, "-m", "dualsphysics_multilayer_amd"] + argv + common, check=True, env=env,
                       cwd=str(tmp_path), timeout=120)
        h, p = read_part(os.path.join(argv[1], "Part_%04u.bi4" % last))
        assert h["peri_mode"] == int(g["peri_mode"]) == 1
        for name in ("peri_xinc", "peri_yinc", "peri_zinc"):
            assert np.array_equal(np.array(h[name]), g[name]), name
        assert np.array_equal(np.array(h["map_posmin"]), g["map_posmin"])
        assert np.array_equal(np.array(h["map_posmax"]), g["map_posmax"])
        assert h["npok"] == len(g["s1_idp"]) and np.array_equal(np.sort(p["idp"]), g["s1_idp"])
