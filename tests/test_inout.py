"""Inlet/outlet zones (<special><inout>), host side: the case loader (inout.py) against the
REFERENCE solver's own PART 0 and configuration, every refusal, the proximity check, and the
fixtures' self-checks.

Fixtures (tests/golden/make_inout.py): the reference DualSPHysics v5.2 CPU solver run on the
cases of case.py InOutChannelCase, 150 steps, PART 0 and three kept PARTs, the fast-math vs
strict-build noise floor, and for every step the smallest distance of a particle to the inlet
plane or a far face (`guard`) next to that step's position noise.
"""
import os

import numpy as np
import pytest

from dualsphysics_multilayer_amd.xmlcase import CaseError, load_case

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "bi4")
# variant: (directory of its case, loader overrides)
VARIANTS = {
    "2d_verlet_ddt3_fixed": ("2d_verlet_ddt3_fixed", {}),
    "2d_symplectic_ddt1_extrap": ("2d_symplectic_ddt1_extrap", {}),
    "3d_verlet_ddt2_extrap": ("3d_verlet_ddt2_extrap", {}),
    "3d_verlet_ddt2_extrap_half": ("3d_verlet_ddt2_extrap", dict(cellmode=2)),
    "3d_verlet_ddt2_refill1": ("3d_verlet_ddt2_refill1", {}),
}
DP = 0.02


def case_path(v):
    return os.path.join(FIX, "inout_" + VARIANTS[v][0], "CaseInOut")


def ref(v):
    return np.load(os.path.join(FIX, "inout_" + v, "ref.npz"))


def kept(g):
    return sorted(int(k[1:].split("_")[0]) for k in g.files if k.startswith("s") and k.endswith("_idp"))


def load(v):
    return load_case(case_path(v), **VARIANTS[v][1])


# ---- the loader against the reference --------------------------------------------------------
@pytest.mark.parametrize("v", sorted(VARIANTS))
def test_initial_particles_equal_the_reference_part0(v):
    x, g = load(v), ref(v)
    init = x.inout["init"]
    n0 = int(g["case_np"])
    assert n0 == x.np
    sel = g["s0_idp"] >= n0
    assert np.array_equal(g["s0_idp"][sel], init["idp"])
    assert np.array_equal(g["s0_pos"][sel], init["pos"])  # bit for bit
    # codes: CODE_TYPE_FLUID_INOUT + zone, zone by zone (LoadInitPartsData)
    zones = x.inout["zones"]
    want = np.concatenate([np.full(z["npartinit"], 0x1FE0 + i, np.uint16) for i, z in enumerate(zones)])
    assert np.array_equal(init["code"], want)
    assert (init["vel"] == 0).all() and (init["rhop"] == 1000).all()
    # no fluid particle lies within 0.8 dp of one: PART 0 holds the whole case
    assert len(x.inout["outignore"]) == 0 and np.array_equal(g["s0_idp"][~sel], np.sort(x.idp))
    assert x.inout["codenewpart"] == 0x1801


# (cfgzone, cfgupdate) of the inlet and the outlet: profile | velocity mode | density mode | check
# input (JSphInOutZone::GetConfigZone), refilling | input treatment | remove (GetConfigUpdate)
CFG = {
    "2d_verlet_ddt3_fixed": ((0x10, 0x02), (0x90, 0x12)),
    "2d_symplectic_ddt1_extrap": ((0x20, 0x02), (0xA8, 0x12)),
    "3d_verlet_ddt2_extrap": ((0x20, 0x02), (0xA8, 0x12)),
    "3d_verlet_ddt2_extrap_half": ((0x20, 0x02), (0xA8, 0x12)),
    "3d_verlet_ddt2_refill1": ((0x92, 0x0C), (0x90, 0x18)),
}


@pytest.mark.parametrize("v", sorted(VARIANTS))
def test_zone_configuration(v):
    x = load(v)
    io = x.inout
    two_d = v.startswith("2d")
    nx = 40 if two_d else 24
    inlet, outlet = io["zones"]
    f32 = np.float32
    # the planes half a dp in front of the points (x = -dp and x = nx dp), pointing into the fluid
    assert np.array_equal(inlet["plane"], np.array([1, 0, 0, DP / 2], f32))
    assert np.array_equal(outlet["plane"], np.array([-1, 0, 0, nx * DP - DP / 2], f32))
    for z in (inlet, outlet):
        assert z["width"] == float(f32(DP * 4)) and z["layers"] == 4
    assert (inlet["cfgzone"], inlet["cfgupdate"]) == CFG[v][0]
    assert (outlet["cfgzone"], outlet["cfgupdate"]) == CFG[v][1]
    # box limits: the points' extent +- dp/2, from the plane to (2 layers + 1) dp/2 behind it
    assert inlet["boxlimitmin"][0] == f32(-DP / 2 - 9 * DP / 2) and inlet["boxlimitmax"][0] == f32(-DP / 2)
    assert outlet["boxlimitmin"][0] == f32(nx * DP - DP / 2)
    # FreeCentre / FreeLimits as the reference's Run.out prints them (%g)
    if two_d:
        fc, lo, hi = (0.39, 0, 0.180707), (-0.01, -0.00141421, -0.00141421), (0.79, 0.00141421, 0.362828)
        assert io["npresizeplus0"] == 192  # "MemoryResizeNp: ... (initial: +192 particles)"
    else:
        fc, lo, hi = (0.23, 0.1, 0.120866), (-0.01, -0.00173205, -0.00173205), (0.47, 0.201732, 0.243464)
        assert io["npresizeplus0"] == 720
    assert np.allclose(io["freecentre"], fc, rtol=2e-6, atol=1e-12)
    assert np.allclose(io["freelimitmin"], lo, rtol=2e-6) and np.allclose(io["freelimitmax"], hi, rtol=2e-6)
    assert io["determlimit"] == float(f32(1e-3 if v.startswith("3d_verlet_ddt2_extrap") else 1e3))
    assert io["extrapolatemode"] == 1 and io["useboxlimit"]


def test_velocity_profiles_and_zsurf():
    x = load("3d_verlet_ddt2_refill1")
    inlet, outlet = x.inout["zones"]
    # the parabola through (dp, 1.5), (3 dp, 2.2), (5 dp, 2.5): a z^2 + b z + c, held as float
    a, b, c = (float(q) for q in inlet["veldata"][0][:3])
    for z, v in ((DP, 1.5), (3 * DP, 2.2), (5 * DP, 2.5)):
        assert a * z * z + b * z + c == pytest.approx(v, abs=2e-5)
    assert np.array_equal(outlet["veldata"][0], np.array([-2.5, 0, 0, 0], np.float32))
    assert inlet["zsurf"] == float(np.float32(4.5 * DP)) and inlet["removezsurf"] and outlet["removezsurf"]
    # refilling 1: the points above zsurf start without particles (36 of the 45 points, 4 layers)
    assert inlet["nptinit"] == 45 and inlet["npartinit"] == 144 and int(inlet["pointsinit"].sum()) == 36
    x = load("2d_verlet_ddt3_fixed")
    assert x.inout["zones"][0]["zsurf"] == float(np.float32(12.5 * DP)) and x.inout["zones"][0]["npartinit"] == 48
    # CoefHydro = rhop0 (-g) / b in float (JSphInOut.cpp:536)
    assert x.inout["coefhydro"] == pytest.approx(1000 * 9.81 / x.cteb, rel=1e-6)
    # no <imposezsurf>: Zsurf is FLT_MAX
    assert load("3d_verlet_ddt2_extrap").inout["zones"][1]["zsurf"] == float(np.finfo(np.float32).max)


def test_messages_of_the_reference():
    x = load("2d_symplectic_ddt1_extrap")
    assert any("InputTreatment==Convert is not recommended" in m or "VelocityMode==Extrapolated is not recommended" in m
               for m in x.messages)
    assert any("Velocity limits are unknown" in m for m in x.messages)


# ---- refusals ---------------------------------------------------------------------------------
def _edit(tmp_path, v, old, new, count=1):
    d = os.path.dirname(case_path(v))
    for f in ("CaseInOut.xml", "CaseInOut.bi4"):
        open(tmp_path / f, "wb").write(open(os.path.join(d, f), "rb").read())
    xml = (tmp_path / "CaseInOut.xml").read_text()
    assert old in xml, old
    (tmp_path / "CaseInOut.xml").write_text(xml.replace(old, new, count))
    return str(tmp_path / "CaseInOut")


V3, V2 = "3d_verlet_ddt2_refill1", "2d_verlet_ddt3_fixed"
REFUSED = [
    # (variant, text to replace, replacement, message)
    (V3, "<box>", '<circle><point x="0" y="0" z="0"/><radius v="1"/></circle><box>', "<circle> is not supported"),
    (V3, "<zone3d><box>", '<zone3d><particles mkfluid="1" direction="right"/><box>', r"<particles mkfluid=\"1\">"),
    (V3, "</box>", '<rotateaxis angle="30" anglesunits="degrees"/></box>', "<rotateaxis> of <box> is not supported"),
    (V2, "</line>", '<rotate angle="30" anglesunits="degrees"/></line>', "<rotate> of <line> is not supported"),
    (V2, '<imposevelocity mode="0">', '<imposevelocity mode="1">', "imposevelocity mode=1 .variable velocity. is not supported"),
    (V2, '<imposevelocity mode="0">', '<imposevelocity mode="3">', "imposevelocity mode=3 .interpolated velocity. is not"),
    (V2, '<velocity v="3.5"/>', '<velocity v="3.5"/><flowvelocity active="true"/>', "<flowvelocity> is not supported"),
    (V2, '<velocity v="3.5"/>', '<velocity v="3.5"/><awas/>', "<awas> is not supported"),
    (V2, '<imposezsurf mode="0">', '<imposezsurf mode="1">', "imposezsurf mode=1 .variable zsurf. is not supported"),
    (V2, '<imposezsurf mode="0">', '<imposezsurf mode="2">', "imposezsurf mode=2 .calculated zsurf. is not supported"),
    (V2, '<refilling value="0"/>', '<refilling value="2"/>', "refilling value=2 .advanced refilling. is not supported"),
    (V2, "<inout>", "<inout><refillingdata/>", "<refillingdata> of <inout> is not valid"),
    # combinations this core does not run with zones
    (V3, '<parameter key="ViscoTreatment" value="1"/>', '<parameter key="ViscoTreatment" value="2"/>',
     "Laminar.SPS viscosity with <special><inout>"),
    (V3, '<parameter key="Shifting" value="0"/>', '<parameter key="Shifting" value="1"/>', "Shifting with <special><inout>"),
    (V3, "</parameters>", '<parameter key="XPeriodicIncZ" value="0"/></parameters>', "Periodic boundaries with <special><inout>"),
    (V3, "</parameters>", '<parameter key="Symmetry" value="1"/></parameters>', "Symmetry with <special><inout>"),
    (V3, "<special>", '<special><gauges><velocity name="v"><point x="0.2" y="0.1" z="0.05"/></velocity></gauges>',
     "<special><gauges> with <special><inout>"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_loader_refuses(tmp_path, k):
    v, old, new, msg = REFUSED[k]
    path = _edit(tmp_path, v, old, new)
    with pytest.raises(CaseError, match=msg):
        load_case(path)


def test_the_sixteenth_zone_is_the_last(tmp_path):
    # 17 active zones: refused before the seventeenth is read
    path = _edit(tmp_path, V2, "</inout>", "</inout>")
    xml = open(path + ".xml").read()
    zone = xml[xml.index("<inoutzone>"):xml.index("</inoutzone>") + len("</inoutzone>")]
    open(path + ".xml", "w").write(xml.replace("</inout>", 15 * zone + "</inout>"))
    with pytest.raises(CaseError, match="Maximum number of inlet/outlet zones has been reached"):
        load_case(path)


def test_restart_and_mdbc_are_refused(tmp_path):
    path = _edit(tmp_path, V3, "</parameters>", '<parameter key="Boundary" value="2"/></parameters>')
    with pytest.raises(CaseError, match="mDBC with <special><inout>"):
        load_case(path)
    d = os.path.dirname(case_path(V3))
    open(tmp_path / "Part_0001.bi4", "wb").write(open(os.path.join(d, "CaseInOut.bi4"), "rb").read())
    path = _edit(tmp_path, V3, "<special>", "<special>")
    with pytest.raises(CaseError, match="Simulation restart not allowed when Inlet/Outlet is used"):
        load_case(path, partbegin=1, partbegin_dir=str(tmp_path))


NNPHASES = ('<nnphases><phase mkfluid="0"><rhop value="1000"/><visco value="0.05"/><tau_yield value="0.0005"/>'
            '<HBP_m value="0"/><HBP_n value="1"/><phasetype value="0"/></phase></nnphases>')


def test_nn_multiphase_is_refused(tmp_path):
    path = _edit(tmp_path, V3, "</parameters>", '<parameter key="RheologyTreatment" value="2"/></parameters>')
    xml = open(path + ".xml").read()
    open(path + ".xml", "w").write(xml.replace("<special>", "<special>" + NNPHASES))
    with pytest.raises(CaseError, match="NN multiphase with <special><inout>"):
        load_case(path)


@pytest.mark.parametrize("fixture,name,what", [
    ("dem_verlet_ddt2", "CaseBlocks", "Floating bodies"),
    ("flume_verlet_ddt2_motion_nested_cir", "CaseFlume", "Moving boundaries"),
])
def test_bodies_are_refused(tmp_path, fixture, name, what):
    """A case of the suite with floating bodies / a motion program: it loads as it is and is
    refused once the zones of an inout fixture are added to it."""
    d = os.path.join(FIX, fixture)
    for f in os.listdir(d):
        if f != "ref.npz":
            open(tmp_path / f, "wb").write(open(os.path.join(d, f), "rb").read())
    path = str(tmp_path / name)
    x = load_case(path)
    assert (x.case_nfloat if what.startswith("Floating") else x.case_nmoving) > 0 and x.inout is None
    zones = open(case_path(V3) + ".xml").read()
    zones = zones[zones.index("<inout>"):zones.index("</inout>") + len("</inout>")]
    xml = open(path + ".xml").read()
    assert "<special>" not in xml
    open(path + ".xml", "w").write(xml.replace("</execution>", "<special>" + zones + "</special></execution>"))
    with pytest.raises(CaseError, match=what + ".* with <special><inout>: not supported"):
        load_case(path)


def test_inactive_inout_is_no_inout(tmp_path):
    path = _edit(tmp_path, V2, "<inout>", '<inout active="false">')
    assert load_case(path).inout is None


def test_wavepaddles_stay_refused(tmp_path):
    path = _edit(tmp_path, V2, "<special>", "<special><wavepaddles/>")
    with pytest.raises(CaseError, match="<special><wavepaddles> is not supported"):
        load_case(path)


# ---- InitCheckProximity -----------------------------------------------------------------------
def test_proximity_warning_excludes_the_fluid(tmp_path):
    # the inlet's points half a dp from the first fluid column: its 12 particles lie within 0.8 dp
    path = _edit(tmp_path, V2, '<point x="-0.02" z="0.02"/><point2 x="-0.02" z="0.24"/>',
                 '<point x="-0.01" z="0.02"/><point2 x="-0.01" z="0.24"/>')
    x = load_case(path)
    out = x.inout["outignore"]
    assert len(out) == 12 and (x.pos[out, 0] == 0).all() and (out >= x.npb).all()
    assert any(m.endswith("12 fluid particles were excluded since they are too close to inout particles. Check VTK "
                          "file CfgInOut_ExcludedParticles.vtk") for m in x.messages)


def test_proximity_error_for_a_boundary_particle(tmp_path):
    # ... and down to the floor's level: the floor particle (0, 0, 0) is 0.5 dp from an inout one
    path = _edit(tmp_path, V2, '<point x="-0.02" z="0.02"/><point2 x="-0.02" z="0.24"/>',
                 '<point x="-0.01" z="0"/><point2 x="-0.01" z="0.24"/>')
    with pytest.raises(CaseError, match="There are inout fluid or boundary particles too close to inout particles"):
        load_case(path)


def test_points_outside_the_domain(tmp_path):
    path = _edit(tmp_path, V2, '<point x="-0.02" z="0.02"/><point2 x="-0.02" z="0.24"/>',
                 '<point x="-0.2" z="0.02"/><point2 x="-0.2" z="0.24"/>')
    with pytest.raises(CaseError, match="Point for inlet conditions with position .* is outside the domain"):
        load_case(path)


# ---- the generator writes the fixtures' cases -------------------------------------------------
def test_generator_reproduces_the_fixture_case(tmp_path):
    import sys

    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_inout
    finally:
        sys.path.pop(0)
    from dualsphysics_multilayer_amd.case import InOutChannelCase

    for v in ("2d_verlet_ddt3_fixed", "3d_verlet_ddt2_refill1"):
        c = InOutChannelCase(**make_inout.VARIANTS[v][0])
        os.makedirs(tmp_path / v)
        path = c.write(str(tmp_path / v))
        assert open(path + ".xml").read() == open(case_path(v) + ".xml").read()
        x = load_case(path)
        lo, hi = c.map_limits()
        assert np.array_equal(x.map_limits()[0], lo) and np.array_equal(x.map_limits()[1], hi)


# ---- self-checks of ref.npz (the generator's conditions, from the file alone) -----------------
@pytest.mark.parametrize("v", sorted(VARIANTS))
def test_fixture_conditions(v):
    g = ref(v)
    ks = kept(g)
    assert ks[0] == 0 and len(ks) == 4 and ks[-1] <= 150 and len(g["times"]) == ks[-1] + 1
    assert max(len(g["s%d_idp" % k]) for k in ks) <= 2500
    column = int(g["column"])
    created = int(g["idmaxs"][-1] - g["idmaxs"][0])
    removed = int(g["nps"][0]) + created - int(g["nps"][-1])
    # enough life-cycle events by the last kept step
    assert created >= 2 * column and removed >= 2 * column
    assert int(g["s%d_idp" % ks[-1]].max()) == int(g["idmaxs"][-1])
    if v == "3d_verlet_ddt2_refill1":  # inputtreatment 2 and `remove` each removed a particle
        assert int(g["removed_input"]) >= 1 and int(g["removed_zsurf"]) >= 1
        assert int(g["s%d_nout" % ks[-1]]) == int(g["removed_input"]) + int(g["removed_zsurf"])
    # creation does not depend on rounding: no particle within 100 x the step's position noise of
    # the inlet plane or a far face, at any step
    assert len(g["guard"]) == ks[-1] + 1 and (g["guard"] > 100 * g["noisepos"]).all()
    for k in ks[1:]:
        assert g["noise_%d" % k].shape == (3,) and (g["noise_%d" % k] >= 0).all()
        assert float(g["s%d_time" % k]) == float(g["times"][k])
