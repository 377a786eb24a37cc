"""RigidAlgorithm 0 and 2 without a device: the loader (modes, <properties>, the DEM table of
JSph::LoadDemData, the refusals), DemDtForce in the PART header, and the float32 restatement of
JSphCpu::InteractionForcesDEM against the float64 one on the cloud the GPU tests use.

The cases are the flume fixture (a fixed tank, two moving blocks, one floating box) with a
<properties> section written here.
"""
import os
import shutil

import numpy as np
import pytest

import dem_clouds
from dualsphysics_multilayer_amd.xmlcase import CaseError, CaseProperties, XmlCase

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "golden", "bi4", "flume_verlet_ddt2")

PROPS = """<properties>
<links>
<link mk="10" property="steel"/>
<link mk="11-12" property="soft+user"/>
<link mk="13" property="pvc"/>
</links>
<property name="steel" Young_Modulus_unused="1">
<Young_Modulus value="210000000000.0" comment="Young Modulus (N/m2)"/>
<PoissonRatio value="0.3"/>
<Restitution_Coefficient value="0.8"/>
<Kfric value="0.45"/>
</property>
<property name="user" Kfric_User="0.3" Restitution_Coefficient_User="0.55" _remark="x"/>
<propertyfile file="Floating_Materials.xml" path="materials"/>
</properties>
"""
MATFILE = """<?xml version="1.0" encoding="UTF-8" ?>
<materials>
<property name="pvc">
<Young_Modulus value="3000000000.0"/>
<PoissonRatio value="0.3"/>
<Restitution_Coefficient value="0.6"/>
<Kfric value="0.15"/>
</property>
<property name="soft">
<Young_Modulus value="1000000.0"/>
<PoissonRatio value="0.45"/>
<Restitution_Coefficient value="0.9"/>
<Kfric value="0.5"/>
</property>
</materials>
"""
ATTR = {10: "steel", 11: "soft+user", 12: "soft+user", 13: "pvc"}


def _variant(tmp_path, rigid=2, props=PROPS, matfile=MATFILE, attr=ATTR, edit=None):
    d = tmp_path / ("c%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    shutil.copy(os.path.join(SRC, "CaseFlume.bi4"), d / "CaseFlume.bi4")
    xml = open(os.path.join(SRC, "CaseFlume.xml")).read()
    xml = xml.replace('key="RigidAlgorithm" value="1"', 'key="RigidAlgorithm" value="%d"' % rigid)
    for mk, name in attr.items():
        xml = xml.replace(' mk="%d" ' % mk, ' mk="%d" property="%s" ' % (mk, name))
    xml = xml.replace("<fluid mkfluid", props + "<fluid mkfluid") if props else xml
    assert 'property="' in xml or not attr
    if edit:
        xml = edit(xml)
    (d / "CaseFlume.xml").write_text(xml)
    if matfile:
        (d / "Floating_Materials.xml").write_text(matfile)
    return str(d / "CaseFlume")


def test_properties_after_blocks_are_accepted(tmp_path):
    """<properties> may stand anywhere among the blocks (here before <fluid>)."""
    x = XmlCase(_variant(tmp_path, rigid=1))
    assert x.ftmode == 1 and not x.use_dem and x.demdata == []


@pytest.mark.parametrize("rigid", [0, 2])
def test_rigid_modes_load(tmp_path, rigid):
    x = XmlCase(_variant(tmp_path, rigid=rigid))
    assert x.rigidalgorithm == rigid and x.ftmode == 2
    assert x.use_dem == (rigid == 2)
    assert len(x.demdata) == (4 if rigid == 2 else 0)


def test_rigid_3_and_others_refused(tmp_path):
    with pytest.raises(CaseError, match="RigidAlgorithm=3"):
        XmlCase(_variant(tmp_path, rigid=3))
    with pytest.raises(CaseError, match="Rigid algorithm is not valid"):
        XmlCase(_variant(tmp_path, rigid=4))


def test_dem_table_is_load_dem_data(tmp_path):
    """StDemData per boundary block by hand (JSph.cpp:1189-1227), in float: a composition "soft+user"
    (sorted, the first property that has a value gives it; the _User values override), a property
    file, tau, and massp = MassBound with mass = 0 for the fixed and moving blocks."""
    x = XmlCase(_variant(tmp_path))
    f32 = np.float32
    got = {d["mk"]: d for d in x.demdata}
    assert sorted(got) == [10, 11, 12, 13]

    def tau(young, poisson):
        return float((f32(1) - f32(poisson) * f32(poisson)) / f32(young))

    mb = float(f32(1.5625e-02))
    want = {10: dict(code=0x0, mass=0.0, massp=mb, tau=tau(2.1e11, 0.3), kfric=float(f32(0.45)), restitu=float(f32(0.8))),
            11: dict(code=0x800, mass=0.0, massp=mb, tau=tau(1e6, 0.45), kfric=float(f32(0.3)), restitu=float(f32(0.55))),
            12: dict(code=0x801, mass=0.0, massp=mb, tau=tau(1e6, 0.45), kfric=float(f32(0.3)), restitu=float(f32(0.55))),
            13: dict(code=0x1000, mass=float(f32(0.9765625)), massp=float(f32(0.0078125)), tau=tau(3e9, 0.3),
                     kfric=float(f32(0.15)), restitu=float(f32(0.6)))}
    for mk, w in want.items():
        for k, v in w.items():
            assert got[mk][k] == v, (mk, k, got[mk][k], v)
    assert x.properties.property_mk(11) == "soft+user"
    assert x.properties.property_mk(99) == ""


@pytest.mark.parametrize("name", ["Kfric", "Restitution_Coefficient", "Young_Modulus", "PoissonRatio"])
def test_missing_value_raises_reference_message(tmp_path, name):
    props = PROPS.replace("<%s value=" % name, "<_%s value=" % name)
    with pytest.raises(CaseError, match=r"Object mk=10 \(mkbound=0\) - Value of %s is invalid\." % name):
        XmlCase(_variant(tmp_path, props=props))
    # collision-free bodies read no material
    assert XmlCase(_variant(tmp_path, rigid=0, props=props)).ftmode == 2


def test_property_errors(tmp_path):
    with pytest.raises(CaseError, match="Property information of mk=12 does not correspond to Links"):
        XmlCase(_variant(tmp_path, attr={**ATTR, 12: "soft"}))
    with pytest.raises(CaseError, match="Property information of mk=10 does not correspond to Links"):
        XmlCase(_variant(tmp_path, rigid=1, attr={k: v for k, v in ATTR.items() if k != 10}))
    with pytest.raises(CaseError, match="Property 'pvc' not found"):
        XmlCase(_variant(tmp_path, matfile=MATFILE.replace('"pvc"', '"pvx"')))
    with pytest.raises(CaseError, match=r"Type of links \(mkbound or mkfluid\) is invalid"):
        XmlCase(_variant(tmp_path, props=PROPS.replace('<link mk="10"', '<link mkbound="0"')))
    with pytest.raises(CaseError, match="Cannot find the element 'stuff'"):
        XmlCase(_variant(tmp_path, props=PROPS.replace('path="materials"', 'path="stuff"')))
    with pytest.raises(CaseError, match="File of properties was not found"):
        XmlCase(_variant(tmp_path, matfile=None))
    with pytest.raises(CaseError, match="Value already exists"):
        XmlCase(_variant(tmp_path, props=PROPS.replace("<Kfric value=\"0.45\"/>", "<Kfric value=\"0.45\"/>"
                                                       "</property><property name=\"steel\" Kfric=\"1\">")))


def test_links_compose_sorted_without_repeats():
    import xml.etree.ElementTree as ET

    p = CaseProperties(ET.fromstring(
        '<properties><links><link mk="1,3-4" property="b + a"/><link mk="3" property="c+a"/></links>'
        '<property name="a" x="1"/><property name="b" x="2"><y value="5"/></property><property name="c" z="3"/>'
        '</properties>'))
    assert p.property_mk(1) == "a+b" and p.property_mk(3) == "a+b+c" and p.property_mk(2) == ""
    assert p.value_float("a+b", "x") == 1.0 and p.value_float("b+a", "x") == 2.0
    assert p.exists_subvalue("a+b", "y", "value") and not p.exists_subvalue("a", "y", "value")
    assert p.subvalue_float("a+b+c", "y", "value", -1.0) == 5.0 and p.subvalue_float("a", "y", "value", -1.0) == -1.0


@pytest.mark.parametrize("rigid", [0, 2])
def test_refused_combinations(tmp_path, rigid):
    def key(name, old, new):
        return lambda s: s.replace('key="%s" value="%s"' % (name, old), 'key="%s" value="%s"' % (name, new))

    with pytest.raises(CaseError, match="Laminar\\+SPS viscosity with RigidAlgorithm=%d" % rigid):
        XmlCase(_variant(tmp_path, rigid=rigid, edit=key("ViscoTreatment", 1, 2)))
    with pytest.raises(CaseError, match="Shifting with RigidAlgorithm=%d" % rigid):
        XmlCase(_variant(tmp_path, rigid=rigid, edit=key("Shifting", 0, 3)))
    with pytest.raises(CaseError, match="mDBC with RigidAlgorithm=%d" % rigid):
        XmlCase(_variant(tmp_path, rigid=rigid), tboundary=2)


def test_part_header_keeps_demdtforce(tmp_path):
    from dualsphysics_multilayer_amd.core import read_part, write_part

    h, p = read_part(os.path.join(SRC, "CaseFlume.bi4"))
    assert h["dem_dtforce"] == 0.0
    h.update(cpart=3, timestep=0.25, dem_dtforce=1.2345678901234e-4)
    fn = str(tmp_path / "Part_0003.bi4")
    write_part(fn, h, p)
    h2, p2 = read_part(fn)
    assert h2["dem_dtforce"] == 1.2345678901234e-4
    assert np.array_equal(p2["idp"], p["idp"])


# ---- the restatements -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud_k():
    from dualsphysics_multilayer_amd.core import case_derive

    out = {}
    for cm in (1, 2):
        c = dem_clouds.make(2, cm)
        out[cm] = (c, case_derive(c.case_def()))
    return out


def test_cloud_holds_the_cases(cloud_k):
    (c, K), (_, K2) = cloud_k[1], cloud_k[2]
    f = dem_clouds.facts(c, K, K2)
    P = f["placed"]
    assert f["both"] >= 1 and f["two_blocks"] >= 1 and f["own_block_only"] >= 1 and f["candidates_differ"] >= 1
    assert len(dem_clouds.candidates(c, K)[P["G"]][0]) == 0
    assert f["ncont"][P["A"]] == 1 and f["ncont"][P["E"]] == 0 and f["visc"][P["C"]] == 0.0
    assert f["visc"][P["E"]] == f["visc_quiet_max"] > f["visc_contact_max"] == f["demdt"]
    assert c.np <= 5000


@pytest.mark.parametrize("cellmode", [1, 2])
def test_float32_restatement_against_float64(cloud_k, cellmode):
    """e_ref of the DEM restatement (relative to max |dace| and to demdt) and of the pair sums: a guard
    against a broken restatement, <= 1e-4."""
    c, K = cloud_k[cellmode]
    a64, d64, n64, _ = dem_clouds.dem(c, K, K["dtini"])
    a32, d32, n32, _ = dem_clouds.dem(c, K, K["dtini"], np.float32)
    e_ace = np.abs(a32 - a64).max() / np.abs(a64).max()
    e_dt = abs(float(d32) - d64) / d64
    print("cellmode %d: e_ref dace %.2e demdt %.2e, contacts %d" % (cellmode, e_ace, e_dt, n64.sum()))
    assert np.array_equal(n64, n32)
    assert e_ace <= 1e-4 and e_dt <= 1e-4
    b64, b32 = dem_clouds.brute_ft(c, K, True), dem_clouds.brute_ft(c, K, True, np.float32)
    for q in ("ar", "ace"):
        assert np.abs(b32[q] - b64[q]).max() / np.abs(b64[q]).max() <= 1e-4
