"""RigidAlgorithm 0 and 2 on the GPU, on the off-lattice cloud of tests/dem_clouds.py (a fixed slab, a
moving block, three floating blobs of different materials, fluid in between; 2,578 particles, 657
contacts on 218 floating particles).

* the DEM pass (csrc/sph_dem.hip) against the float64 restatement of JSphCpu::InteractionForcesDEM:
  the acceleration it adds per particle (the run with RigidAlgorithm=2 minus the run with 0, whose
  pair sums are the same kernel's), the ViscDt maximum and AceMax; particles without a contact
  bitwise unchanged.  Bound: 10 x e_ref, the float32 restatement's distance from the float64 one.
* the FTMODE_Ext pair rule of both interaction kernels against a float64 sum over all pairs that
  carries the `compute` flag; the same comparison with RigidAlgorithm=1 must fail.

The cloud is checked (tests/test_dem.py, and again here from the same facts) to hold: a p1 with
contacts in bound and in fluid cells, one touching two other blocks, one with only its own block
around it, a contact with zero tangential velocity, a candidate pair with vn = 0, a floating particle
without contact whose demvisc exceeds every contacting particle's (so a kernel that folds demdt
without the non-zero-sum rule fails) and p1 whose candidates differ between full and half cells.

Measured on an MI355X: see DESIGN.md section 6l.
"""
import numpy as np
import pytest

import dem_clouds
from test_gpu_clouds import gpu_interaction

pytestmark = pytest.mark.gpu

MARGIN = 10.0
_CACHE = {}


def _derive(case):
    from dualsphysics_multilayer_amd.core import case_derive

    return case_derive(case.case_def())


def _ref(cellmode):
    """The float64 / float32 restatements of one cell mode, computed once."""
    if cellmode not in _CACHE:
        c = dem_clouds.make(2, cellmode)
        K = _derive(c)
        d64 = dem_clouds.dem(c, K, K["dtini"])
        d32 = dem_clouds.dem(c, K, K["dtini"], np.float32)
        b = {(ext, t): dem_clouds.brute_ft(c, K, ext, t) for ext in (True, False) for t in (np.float64, np.float32)}
        _CACHE[cellmode] = dict(K=K, d64=d64, d32=d32, b=b)
    return _CACHE[cellmode]


def _by_idp(g, n):
    o = np.empty(n, np.int64)
    o[np.asarray(g["idp"], np.int64)] = np.arange(n)
    return dict(ar=g["ar"][o], ace=g["ace"][o])


def _run(rigid, cellmode, simple, monkeypatch):
    if simple:
        monkeypatch.setenv("SPH_INTERACTION", "simple")
    c = dem_clouds.make(rigid, cellmode)
    g = gpu_interaction(c)
    assert (g["stats"]["np"], g["stats"]["npb"], g["stats"]["nout"]) == (c.np, c.npb, 0)
    g.update(_by_idp(g, c.np))
    return c, g


def test_cloud_holds_the_cases():
    c = dem_clouds.make(2, 1)
    f = dem_clouds.facts(c, _ref(1)["K"], _ref(2)["K"])
    P = f["placed"]
    assert f["both"] >= 1 and f["two_blocks"] >= 1 and f["own_block_only"] >= 1 and f["candidates_differ"] >= 1
    assert f["ncont"][P["A"]] == 1 and f["ncont"][P["E"]] == 0 and f["visc"][P["C"]] == 0.0
    assert f["visc"][P["E"]] == f["visc_quiet_max"] > f["visc_contact_max"] == f["demdt"]
    assert f["demdt"] > _ref(1)["b"][(True, np.float64)]["viscdt"]  # the DEM dt is what ViscDtMax shows
    assert c.np <= 5000


@pytest.mark.parametrize("simple", [False, True], ids=["tiled", "simple"])
@pytest.mark.parametrize("cellmode", [1, 2])
def test_dem_kernel_against_float64(cellmode, simple, monkeypatch):
    R = _ref(cellmode)
    a64, demdt64, ncont, _ = R["d64"]
    a32, demdt32, _, _ = R["d32"]
    scale = np.abs(a64).max()
    e_ref = np.abs(a32 - a64).max() / scale
    e_ref_dt = abs(float(demdt32) - demdt64) / demdt64
    c, g2 = _run(2, cellmode, simple, monkeypatch)
    _, g0 = _run(0, cellmode, simple, monkeypatch)
    dace = g2["ace"].astype(np.float64) - g0["ace"].astype(np.float64)
    e_gpu = np.abs(dace - a64).max() / scale
    e_dt = abs(float(g2["viscdtmax"]) - demdt64) / demdt64
    final = g2["ace"][c.npb:].astype(np.float64)
    acemax64 = float(np.sqrt((final * final).sum(axis=1).max()))
    e_acemax = abs(float(g2["acemax"]) - acemax64) / acemax64
    print("cellmode %d %s: e_ref dace %.2e demdt %.2e | gpu dace %.2e (ratio %.1f) demdt %.2e (ratio %.1f) | "
          "acemax %.6e vs %.6e (%.1e), pair sums alone %.6e"
          % (cellmode, "simple" if simple else "tiled", e_ref, e_ref_dt, e_gpu, e_gpu / e_ref, e_dt,
             e_dt / e_ref_dt, g2["acemax"], acemax64, e_acemax, g0["acemax"]))
    # particles without a contact: bitwise what the run without DEM gives; ar is never touched
    quiet = ~np.any(a64 != 0, axis=1)
    assert quiet.sum() > 0 and (~quiet).sum() == (ncont > 0).sum()
    assert np.array_equal(g2["ace"][quiet].view(np.uint32), g0["ace"][quiet].view(np.uint32))
    assert np.array_equal(g2["ar"].view(np.uint32), g0["ar"].view(np.uint32))
    assert np.all(np.any(g2["ace"][~quiet] != g0["ace"][~quiet], axis=1))
    # the contact accelerations and the DEM time step
    assert e_gpu <= MARGIN * e_ref, (e_gpu, e_ref)
    assert e_dt <= MARGIN * e_ref_dt, (e_dt, e_ref_dt, float(g2["viscdtmax"]), demdt64)
    # AceMax is the maximum over the final accelerations (float sum of squares, then a square root),
    # not the pair sums' maximum
    assert e_acemax <= 4 * 2.0 ** -24, (g2["acemax"], acemax64)
    assert float(g0["acemax"]) < 0.5 * float(g2["acemax"])


@pytest.mark.parametrize("simple", [False, True], ids=["tiled", "simple"])
@pytest.mark.parametrize("cellmode", [1, 2])
def test_ftmode_ext_pair_rule(cellmode, simple, monkeypatch):
    R = _ref(cellmode)
    ext64, ext32 = R["b"][(True, np.float64)], R["b"][(True, np.float32)]
    sph64, sph32 = R["b"][(False, np.float64)], R["b"][(False, np.float32)]
    assert ext64["nskipped"] > 0
    c, g0 = _run(0, cellmode, simple, monkeypatch)
    _, g1 = _run(1, cellmode, simple, monkeypatch)

    def err(g, ref):
        return {q: float(np.abs(g[q].astype(np.float64) - ref[q]).max() / np.abs(ref[q]).max()) for q in ("ar", "ace")}

    e_ref = err(ext32, ext64)
    e_ref1 = err(sph32, sph64)
    e0, e0_wrong, e1 = err(g0, ext64), err(g1, ext64), err(g1, sph64)
    print("cellmode %d %s: e_ref ar %.2e ace %.2e | RigidAlgorithm=0 ar %.2e ace %.2e (ratio %.1f %.1f) | "
          "RigidAlgorithm=1 against the Ext sum ar %.2e ace %.2e, against its own ar %.2e ace %.2e (e_ref %.2e %.2e)"
          % (cellmode, "simple" if simple else "tiled", e_ref["ar"], e_ref["ace"], e0["ar"], e0["ace"],
             e0["ar"] / e_ref["ar"], e0["ace"] / e_ref["ace"], e0_wrong["ar"], e0_wrong["ace"], e1["ar"], e1["ace"],
             e_ref1["ar"], e_ref1["ace"]))
    for q in ("ar", "ace"):
        assert e0[q] <= MARGIN * e_ref[q], (q, e0[q], e_ref[q])
        assert e0_wrong[q] > MARGIN * e_ref[q], (q, e0_wrong[q])  # the skipped pairs carry weight
        assert e1[q] <= MARGIN * e_ref1[q], (q, e1[q], e_ref1[q])  # and RigidAlgorithm=1 keeps them
    assert float(g0["viscdtmax"]) == pytest.approx(ext64["viscdt"], rel=1e-5)
    assert not g0["ace"][: c.npb].any()


@pytest.mark.parametrize("simple", [False, True], ids=["tiled", "simple"])
def test_acemax_when_a_contact_lowers_the_maximum(simple, monkeypatch):
    """dem_clouds.make_acemax: the floating particle that holds the pair sums' maximum of |ace| is
    stopped by a contact.  The reported AceMax is the float64 maximum over the final accelerations,
    well below the pair sums' maximum, which a fold over slots that were not cleared would keep."""
    if simple:
        monkeypatch.setenv("SPH_INTERACTION", "simple")
    c, ip, _ = dem_clouds.make_acemax()
    K = _derive(c)
    pair = dem_clouds.brute_ft(c, K, True)["ace"]
    dace = dem_clouds.dem(c, K, K["dtini"])[0]
    mag = lambda a: np.sqrt((a[c.npb:] * a[c.npb:]).sum(axis=1))  # noqa: E731
    pair_max, final_max = float(mag(pair).max()), float(mag(pair + dace).max())
    assert mag(pair).argmax() + c.npb == ip and final_max < 0.5 * pair_max  # the state, from the cloud itself
    assert mag(pair + dace)[ip - c.npb] < 1e-3 * pair_max
    g = gpu_interaction(c)
    g.update(_by_idp(g, c.np))
    final = g["ace"][c.npb:].astype(np.float64)
    acemax64 = float(np.sqrt((final * final).sum(axis=1).max()))
    print("%s: pair-sum maximum %.6e (float64), final maximum %.6e (float64 restatement) / %.6e (float64 over the GPU's "
          "final ace), reported AceMax %.6e" % ("simple" if simple else "tiled", pair_max, final_max, acemax64, g["acemax"]))
    assert abs(float(g["acemax"]) - acemax64) <= 4 * 2.0 ** -24 * acemax64
    assert abs(float(g["acemax"]) - final_max) <= 1e-4 * final_max
    assert float(g["acemax"]) < 0.5 * pair_max


def test_refusals(tmp_path):
    from dualsphysics_multilayer_amd.core import SphError, SphGpuSingle, SphSlabGroup
    from dualsphysics_multilayer_amd.xmlcase import XmlCase
    from test_dem import _variant

    x = XmlCase(_variant(tmp_path, rigid=2))
    g = SphGpuSingle(x, device=0)
    with pytest.raises(SphError, match="SPH_ERR_STATE"):  # once
        g.set_rigid(2, True, x.demdata)
    g.run(2)
    g.sync()
    st = g.stats()
    assert st["dem_dtforce"] == st["last_dt"] > 0 and st["error_flags"] == 0
    g.close()
    # DEM data that lacks the floating body's block, a mode that does not exist, DEM without FTMODE_Ext
    x1 = XmlCase(_variant(tmp_path, rigid=1))
    for args in ((2, True, [d for d in x.demdata if d["mk"] != 13]), (3, False, []), (1, True, x.demdata)):
        g = SphGpuSingle(x1, device=0)
        with pytest.raises(SphError, match="SPH_ERR_ARG"):
            g.set_rigid(*args)
        g.close()
    # mDBC is refused by the core too (configured at creation, before the rigid algorithm)
    import os

    xm = XmlCase(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bi4", "flume_symplectic_ddt1_mdbc",
                              "CaseFlume"))
    g = SphGpuSingle(xm, device=0)
    with pytest.raises(SphError, match="SPH_ERR_UNSUPPORTED.*mDBC"):
        g.set_rigid(2, False, [])
    g.close()
    # slabs take RigidAlgorithm=1 only
    for rigid in (0, 2):
        xs = XmlCase(_variant(tmp_path, rigid=rigid))
        ncx = _derive(xs)["dom_cells"][0]
        with pytest.raises(SphError, match="SPH_ERR_ARG.*single domain"):
            SphSlabGroup(xs, [0, ncx // 2, ncx])


def test_dem_without_floating_block_is_plain_sph(tmp_path):
    """RigidAlgorithm=2 without a floating block: DEM is switched off with the reference's warning and
    the case runs as it does with RigidAlgorithm=1, bit for bit."""
    import os
    import shutil

    from dualsphysics_multilayer_amd.core import SphGpuSingle
    from dualsphysics_multilayer_amd.xmlcase import XmlCase

    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bi4", "forcing_verlet_ddt2_damp_box_cyl")
    out = {}
    for rigid in (1, 2):
        d = tmp_path / ("r%d" % rigid)
        shutil.copytree(src, d)
        fn = d / "CaseDambreak.xml"
        xml = fn.read_text()
        assert 'key="RigidAlgorithm" value="1"' in xml
        fn.write_text(xml.replace('key="RigidAlgorithm" value="1"', 'key="RigidAlgorithm" value="%d"' % rigid))
        x = XmlCase(str(d / "CaseDambreak"))
        assert x.ftmode == 0 and not x.use_dem
        assert (rigid == 2) == any("DEM was disabled" in m for m in x.messages)
        g = SphGpuSingle(x, device=0)
        g.run(5)
        g.sync()
        p = g.particles()
        o = np.argsort(p["idp"])
        out[rigid] = (p["pos"][o], p["vel"][o], p["rhop"][o], g.stats()["time"])
        g.close()
    for a, b in zip(out[1], out[2]):
        assert np.array_equal(a, b)
