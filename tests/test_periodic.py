"""Periodic boundaries without a GPU: the case loader, the derived map limits, and the numpy
restatement of RunPeriodic that tests/test_gpu_periodic.py compares the device pass with.

* Loader: every periodic <parameter> key (JSph.cpp:718-730), the real map (border Dp/2 and no
  <simulationdomain> on a periodic axis, JPartsLoad4.cpp:339-347, JSph.cpp:1382-1384), the
  refused combinations.  The fixtures of tests/golden/make_periodic.py carry the reference's
  own MapRealPosMin/Max and Peri?inc (read from its PART header): the loader and the core must
  give exactly those.
* Periodic clouds (tests/periodic_clouds.py): their explicit-image extension has duplicates at
  every periodic face and corner images on two axes, leaves no pair inside clouds.SHELL (so no
  particle is left out of a comparison), and gives every original particle exactly the
  neighbours of the minimum-image rule; the CPU oracle counts the same pairs on it.
"""
import os

import numpy as np
import pytest

import clouds
import periodic_clouds as pc

from dualsphysics_multilayer_amd.case import PeriodicChannelCase
from dualsphysics_multilayer_amd.core import case_derive
from dualsphysics_multilayer_amd.xmlcase import CaseError, XmlCase, load_case

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "bi4")
VARIANTS = ("x_verlet_ddt2", "x_verlet_ddt2_half", "xy_incy_symplectic_ddt1", "x_2d_verlet_ddt3",
            "x_verlet_ddt2_restart")


def case_path(v):
    """The case files of a variant: the -cellmode:half run and the restart are runs of case 1."""
    base = "x_verlet_ddt2" if v in ("x_verlet_ddt2_half", "x_verlet_ddt2_restart") else v
    return os.path.join(FIX, "periodic_" + base, "CasePeriodic")


def fixture_case(v):
    d = os.path.join(FIX, "periodic_" + v)
    if v.endswith("_restart"):
        return load_case(case_path(v), partbegin=int(np.load(os.path.join(d, "ref.npz"))["partbegin"]), partbegin_dir=d)
    kw = dict(cellmode=2) if v.endswith("_half") else {}
    return load_case(case_path(v), **kw)


def fixture_ref(v):
    return np.load(os.path.join(FIX, "periodic_" + v, "ref.npz"))


def kept(g):
    return sorted(int(k[1:].split("_")[0]) for k in g.files if k.startswith("s") and k.endswith("_idp"))


# ---- loader ---------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS)
def test_fixture_limits_equal_the_reference_header(v):
    """MapRealPosMin/Max and the three incs of the loader + core are the values the reference
    wrote into its PART header, bit for bit."""
    x, g = fixture_case(v), fixture_ref(v)
    k = case_derive(x.case_def())
    lo, hi = x.map_limits()
    assert np.array_equal(lo, g["map_posmin"]) and np.array_equal(hi, g["map_posmax"])
    assert k["peri_active"] == int(g["peri_mode"]) == x.peri_active
    for name in ("peri_xinc", "peri_yinc", "peri_zinc"):
        assert np.array_equal(np.array(k[name]), g[name]), (name, k[name], g[name])
    ks = float(np.float32(k["kernelsize"]))
    for a in range(3):
        w = ks if (x.peri_active >> a) & 1 else 0.0
        assert k["map_posmin"][a] == lo[a] - w and k["map_posmax"][a] == hi[a] + w
        assert k["dom_posmin"][a] == k["map_posmin"][a]
        assert k["dom_cells"][a] == int(np.ceil((k["map_posmax"][a] - k["map_posmin"][a]) / float(np.float32(k["scell"]))))


@pytest.mark.parametrize("v", VARIANTS)
def test_fixture_wraps_particles(v):
    """The condition the generator asserted, again from ref.npz alone: by the last kept PART at
    least 20 fluid particles jumped by about one period between kept PARTs (case 2: at least 5
    on each axis)."""
    g = fixture_ref(v)
    ks = kept(g)
    size = g["map_posmax"] - g["map_posmin"]
    wrapped = [set(), set(), set()]
    for a, b in zip(ks[:-1], ks[1:]):
        assert np.array_equal(g["s%d_idp" % a], g["s%d_idp" % b])
        d = g["s%d_pos" % b] - g["s%d_pos" % a]
        for ax in range(3):
            if (int(g["peri_mode"]) >> ax) & 1:
                wrapped[ax] |= set(g["s%d_idp" % a][np.abs(d[:, ax]) > 0.5 * size[ax]].tolist())
    if v.endswith("_restart"):
        return  # one kept PART: pinned for the restart itself
    assert len(wrapped[0] | wrapped[1] | wrapped[2]) >= 20
    if v.startswith("xy_"):
        assert len(wrapped[0]) >= 5 and len(wrapped[1]) >= 5


def _write(tmp_path, peri, extra="", **kw):
    c = PeriodicChannelCase(0.02, 20, 20, 10, 9, peri, **kw)  # every period longer than 2 KernelSize, z too
    path = c.write(str(tmp_path))
    if extra:
        xml = open(path + ".xml").read()
        open(path + ".xml", "w").write(xml.replace("</parameters>", extra + "</parameters>"))
    return c, path


@pytest.mark.parametrize("key,active,comp", [
    ("XPeriodicIncY", 1, (0, 1)), ("XPeriodicIncZ", 1, (0, 2)), ("YPeriodicIncX", 2, (1, 0)),
    ("YPeriodicIncZ", 2, (1, 2)), ("ZPeriodicIncX", 4, (2, 0)), ("ZPeriodicIncY", 4, (2, 1))])
def test_loader_parses_the_offset_keys(tmp_path, key, active, comp):
    c, path = _write(tmp_path, {key: 0.06})
    x = XmlCase(path)
    assert x.peri_active == active == c.peri_active
    incs = np.array([x.peri_xinc, x.peri_yinc, x.peri_zinc])
    want = np.zeros((3, 3))
    want[comp] = 0.06
    assert np.array_equal(incs, want)
    # generator and loader agree on the limits; the core derives the own-axis component
    assert all(np.array_equal(a, b) for a, b in zip(x.map_limits(), c.map_limits()))
    k = case_derive(x.case_def())
    assert k == case_derive(c.case_def())
    ax = comp[0]
    own = np.array(k[("peri_xinc", "peri_yinc", "peri_zinc")[ax]])
    lo, hi = x.map_limits()
    assert own[ax] == -(hi[ax] - lo[ax]) and own[comp[1]] == 0.06
    # a periodic axis: border Dp/2, whatever <simulationdomain> says
    assert lo[ax] == x.case_posmin[ax] - 0.01 and hi[ax] == x.case_posmax[ax] + 0.01


@pytest.mark.parametrize("key,active", [("XYPeriodic", 3), ("XZPeriodic", 5), ("YZPeriodic", 6)])
def test_loader_parses_the_two_axis_keys(tmp_path, key, active):
    """XYPeriodic and its siblings set two axes and zero every offset given before them."""
    c, path = _write(tmp_path, {"XPeriodicIncY": 0.06, key: 1})
    x = XmlCase(path)
    assert x.peri_active == active == c.peri_active
    assert not np.array([x.peri_xinc, x.peri_yinc, x.peri_zinc]).any()
    assert case_derive(x.case_def()) == case_derive(c.case_def())


def test_loader_two_keys_with_offset(tmp_path):
    c, path = _write(tmp_path, {"XPeriodicIncY": 0.06, "YPeriodicIncZ": 0})
    x = XmlCase(path)
    assert x.peri_active == 3 and x.peri_xinc == [0.0, 0.06, 0.0] and x.peri_yinc == [0.0, 0.0, 0.0]


def test_loader_refuses_2d_with_periodic_y(tmp_path):
    _, path = _write(tmp_path, {"XPeriodicIncZ": 0}, data2d=True)
    XmlCase(path)  # 2-D with PeriX is fine
    xml = open(path + ".xml").read()
    open(path + ".xml", "w").write(xml.replace("XPeriodicIncZ", "YPeriodicIncZ"))
    with pytest.raises(CaseError, match="periodic conditions in Y with 2D"):
        XmlCase(path)


def test_loader_refuses_symmetry_with_periodic_y(tmp_path):
    _, path = _write(tmp_path, {"YPeriodicIncZ": 0}, extra='<parameter key="Symmetry" value="1"/>')
    with pytest.raises(CaseError, match="Symmetry is not allowed with periodic conditions in axis Y"):
        XmlCase(path)


GAUGES = """<special><gauges><default><savevtkpart value="false"/><computedt value="0"/><computetime start="0" end="10"/>
<output value="true"/><outputdt value="0"/><outputtime start="0" end="10"/></default>
<velocity name="V0"><point x="0.2" y="0.2" z="0.04"/></velocity></gauges></special>"""


NNPHASES = """<special><nnphases><phase mkfluid="0"><rhop value="1000"/><visco value="0.05"/><tau_yield value="0.0005"/>
<HBP_m value="0"/><HBP_n value="1"/><phasetype value="0"/></phase></nnphases></special>"""
PERIKEY = '<parameter key="XPeriodicIncZ" value="0"/>'


def _refused_with_key_only(path, names, **over):
    """The case loads without the periodic key and is refused with it, by the periodic check and
    naming every feature in `names`."""
    xml = open(path + ".xml").read()
    assert "Periodic" not in xml
    assert XmlCase(path, **over).peri_active == 0
    open(path + ".xml", "w").write(xml.replace("</parameters>", PERIKEY + "</parameters>"))
    with pytest.raises(CaseError, match="with periodic boundaries: not supported") as ei:
        XmlCase(path, **over)
    for name in names:
        assert name in str(ei.value), (name, str(ei.value))


def _plain_channel(tmp_path, extra="", special=""):
    """The channel case without a periodic key (its limits are then the ordinary ones)."""
    c, path = _write(tmp_path, {"XPeriodicIncZ": 0})
    xml = open(path + ".xml").read().replace(PERIKEY, "")
    xml = xml.replace("</parameters>", extra + "</parameters>").replace("</execution>", special + "</execution>")
    open(path + ".xml", "w").write(xml)
    return path


@pytest.mark.parametrize("name,extra,special,over", [
    ("Symmetry", '<parameter key="Symmetry" value="1"/>', "", {}),
    ("mDBC", "", "", dict(tboundary=2)),
    ("Laminar+SPS viscosity", "", "", dict(tvisco=2)),
    ("Shifting", "", "", dict(shift_mode=3)),
    ("NN multiphase", '<parameter key="RheologyTreatment" value="2"/>', NNPHASES, {}),
    ("<special><gauges>", "", GAUGES, {}),
])
def test_loader_refuses_unsupported_combinations(tmp_path, name, extra, special, over, monkeypatch):
    """Each refused feature on a case that is valid without the periodic key."""
    path = _plain_channel(tmp_path, extra, special)
    if name == "mDBC":  # the normals file is read after the periodic check; valid without the key needs one
        from dualsphysics_multilayer_amd.core import write_normals

        n = XmlCase(path).npb
        write_normals(path + "_Normals.nbi4", np.tile([0.0, 0.0, 0.01], (n, 1)), 0.02, XmlCase(path).h, "CasePeriodic")
    _refused_with_key_only(path, [name], **over)


def test_loader_refuses_moving_and_floating_bodies(tmp_path):
    """The committed wave flume (a piston, a flap, a floating box, with its <motion> and <floating>
    blocks) loads as it is and is refused with a periodic key, for both kinds of bodies."""
    d = os.path.join(FIX, "flume_verlet_ddt2")
    for f in os.listdir(d):
        if f.startswith("CaseFlume"):
            open(tmp_path / f, "wb").write(open(os.path.join(d, f), "rb").read())
    path = str(tmp_path / "CaseFlume")
    x = XmlCase(path)
    assert x.case_nmoving > 0 and x.case_nfloat > 0
    _refused_with_key_only(path, ["Moving boundaries", "Floating bodies"])


def test_loader_refuses_a_part_of_another_periodic_mode(tmp_path):
    """A PART whose PeriMode differs from the case's is an error (JPartsLoad4::CheckConfig)."""
    from dualsphysics_multilayer_amd.core import read_part, write_part

    c, path = _write(tmp_path, {"XPeriodicIncZ": 0})
    h, p = read_part(path + ".bi4")
    for mode, ok in ((1, True), (3, False), (0, False)):
        h2 = dict(h, peri_mode=mode, cpart=1, map_posmin=list(c.map_limits()[0]), map_posmax=list(c.map_limits()[1]))
        write_part(str(tmp_path / "Part_0001.bi4"), h2, p)
        if ok:
            assert XmlCase(path, partbegin=1, partbegin_dir=str(tmp_path)).np == c.np
        else:
            with pytest.raises(CaseError, match="periodic configuration"):
                XmlCase(path, partbegin=1, partbegin_dir=str(tmp_path))


def test_core_refuses_invalid_periodic_definitions():
    from dualsphysics_multilayer_amd.core import SphError

    c = PeriodicChannelCase(0.02, 20, 20, 6, 3, {"XPeriodicIncZ": 0})
    cd = c.case_def()
    with pytest.raises(SphError, match="peri_active"):
        case_derive(dict(cd, peri_active=8))
    with pytest.raises(SphError, match="(?i)periodic conditions in Y"):
        case_derive(dict(cd, peri_active=2, data2d=1))
    lo, hi = cd["map_realposmin"], cd["map_realposmax"]
    with pytest.raises(SphError, match="(?i)periodic conditions in axis Y"):
        case_derive(dict(cd, peri_active=2, symmetry=1, map_realposmin=(lo[0], 0.0, lo[2])))
    # a period of at most twice the interaction distance
    ks = float(np.float32(case_derive(cd)["kernelsize"]))
    with pytest.raises(SphError, match="periodic boundaries: a periodic axis must be longer than twice"):
        case_derive(dict(cd, map_realposmax=(lo[0] + 2.0 * ks, hi[1], hi[2])))
    assert case_derive(dict(cd, map_realposmax=(lo[0] + 2.01 * ks, hi[1], hi[2])))["peri_active"] == 1
    # no periodic axis: the cell domain is the real map, as before periodic boundaries existed
    k = case_derive(dict(cd, peri_active=0))
    assert k["dom_posmin"] == list(lo) and not any(k["map_posmin"]) and not any(k["map_posmax"])
    assert k["dom_cells"] == [int(np.ceil((hi[a] - lo[a]) / float(np.float32(k["scell"])))) for a in range(3)]


# ---- periodic clouds ------------------------------------------------------------------------
def _K(case):
    return case_derive(case.case_def())


@pytest.mark.parametrize("name", pc.NAMES)
def test_extension_has_every_face_and_corners(name):
    case = pc.make(name, tdensity=0)
    K = _K(case)
    e, orig, info = pc.extended(case, K)
    print(name, "np", case.np, "npb", case.npb, "dups", info["nbound"], info["nfluid"], info["faces"], "corner",
          info["corner"])
    assert case.np <= 4000 and case.np - case.npb > 256
    for ax, (lo_n, hi_n) in info["faces"].items():
        assert lo_n > 0 and hi_n > 0, (name, ax)
    assert set(info["faces"]) == {a for a in range(3) if (case.peri_active >> a) & 1}
    if name != "x":
        assert info["corner"] > 0
    # the originals keep their values and order; the duplicates copy their source
    assert np.array_equal(e.pos[orig], case.pos) and np.array_equal(e.vel[orig], case.vel)
    assert np.array_equal(e.rhop, case.rhop[info["src"]])
    lo, hi = e.map_limits()
    assert (e.pos >= lo).all() and (e.pos < hi).all()
    # every duplicate lies outside the real map on at least one periodic axis
    dup = np.setdiff1d(np.arange(e.np), orig)
    rlo, rhi = case.map_limits()
    assert ((e.pos[dup] < rlo) | (e.pos[dup] >= rhi)).any(axis=1).all()


@pytest.mark.parametrize("name", pc.NAMES)
def test_extension_leaves_no_pair_in_the_shell(name):
    """brute on the extended cloud reports shell == 0: no pair is within 2e-6 of r = 2h, so float
    and double agree on every pair and no particle is left out of any comparison."""
    for cm in (1, 2):
        case = pc.make(name, tdensity=2, cellmode=cm)
        e, orig, _ = pc.extended(case, _K(case))
        ref = clouds.brute(e, _K(e), 2)
        assert not ref["shell"].any(), (name, ref["shell"])
        assert not ref["amb"].any()


@pytest.mark.parametrize("name", pc.NAMES)
def test_extension_gives_the_minimum_image_neighbours(name):
    """The numpy restatement of PeriodicMakeList is complete and has no double images: the real
    pairs of the ORIGINAL particles in the extended cloud are those of the minimum-image rule
    over all 27 period combinations."""
    case = pc.make(name, tdensity=0)
    K = _K(case)
    e, orig, _ = pc.extended(case, K)
    P = clouds.pairs(e, _K(e))
    isorig = np.zeros(e.np, bool)
    isorig[orig] = True
    fi, fj = P["i"] >= e.npb, P["j"] >= e.npb
    real = P["real"] & isorig[P["i"]]
    got = np.array([(real & fi & fj).sum(), (real & fi & ~fj).sum(), (real & ~fi & fj).sum()], np.int64)
    want = pc.image_counts(case, K)
    print(name, got, want)
    assert np.array_equal(got, want)
    # ... and more than the same cloud sees without its images
    plain = clouds.pairs(case, K)
    assert got.sum() > (plain["real"] & ((plain["i"] >= case.npb) | (plain["j"] >= case.npb))).sum()


@pytest.mark.parametrize("name", pc.NAMES)
def test_oracle_counts_the_same_pairs_on_the_extension(name):
    oracle = pytest.importorskip("oracle.pyoracle")
    for cm in (1, 2):
        case = pc.make(name, tdensity=0, cellmode=cm)
        e, orig, _ = pc.extended(case, _K(case))
        ref = clouds.brute(e, _K(e), 0)
        o = oracle.OracleSolver(e, nthreads=4)
        s = o.stats()
        assert (s["np"], s["npb"], s["nout"]) == (e.np, e.npb, 0)
        assert np.array_equal(o.count_pairs().astype(np.int64)[[1, 3, 5]], ref["counts"])


def test_wrap_is_a_translation_of_the_same_system():
    """The shifted and wrapped cloud of the translation test is the same periodic system: the
    same minimum-image pair counts, every particle inside the real map."""
    case = pc.make("xy", tdensity=0)
    K = _K(case)
    cs = float(np.float32(K["scell"]))
    sh = pc.make("xy", tdensity=0, shift=(0.37 * cs, -0.61 * cs, 0.0))
    lo, hi = sh.map_limits()
    assert (sh.pos >= lo).all() and (sh.pos < hi).all() and not np.array_equal(sh.pos, case.pos)
    assert np.array_equal(pc.image_counts(sh, K), pc.image_counts(case, K))


def test_loader_refuses_a_periodic_axis_closed_by_walls(tmp_path):
    """A periodic axis with a boundary wall over the whole cross-section at each end (the
    committed dam break tank, walls at x = 0 and x = 1.6) is refused as a configuration error.
    Boundary particles that merely reach the faces close nothing: a floor-only channel and a
    channel with side walls, each with a fluid block in the middle away from both faces, load;
    so does an axis with one closed end (the floor under ZPeriodic)."""
    for ext in (".xml", ".bi4"):
        open(tmp_path / ("CaseDambreak" + ext), "wb").write(open(os.path.join(FIX, "CaseDambreak" + ext), "rb").read())
    xml = (tmp_path / "CaseDambreak.xml").read_text()
    (tmp_path / "CaseDambreak.xml").write_text(xml.replace("<parameters>", "<parameters>\n" + PERIKEY))
    with pytest.raises(CaseError, match="Periodic axis X is closed by a boundary wall at each end"):
        XmlCase(str(tmp_path / "CaseDambreak"))
    from dualsphysics_multilayer_amd.core import read_part, write_part

    for k, ywalls in enumerate((False, True)):
        sub = tmp_path / ("block%d" % k)
        sub.mkdir()
        c, path = _write(sub, {"XPeriodicIncZ": 0}, ywalls=ywalls)
        h, p = read_part(path + ".bi4")
        fl = p["idp"] >= c.npb
        x = p["pos"][:, 0]
        keep = ~fl | ((x > 0.1) & (x < 0.3))  # the fluid block: x in (0.1, 0.3) of the period [-0.01, 0.39)
        assert 0 < (fl & keep).sum() < fl.sum()
        q = {a: np.ascontiguousarray(v[keep]) for a, v in p.items()}
        q["idp"] = np.arange(keep.sum(), dtype=np.uint32)
        nfl = int((fl & keep).sum())
        write_part(path + ".bi4", dict(h, case_np=len(q["idp"]), case_nfluid=nfl, map_posmin=[0.0] * 3, map_posmax=[0.0] * 3), q)
        xml = open(path + ".xml").read().replace('np="%d"' % c.np, 'np="%d"' % len(q["idp"]))
        xml = xml.replace('begin="%d" count="%d"' % (c.npb, c.np - c.npb), 'begin="%d" count="%d"' % (c.npb, nfl))
        open(path + ".xml", "w").write(xml)
        loaded = XmlCase(path)
        assert loaded.peri_active == 1 and loaded.np == len(q["idp"])
    sub = tmp_path / "z"
    sub.mkdir()
    _, path = _write(sub, {"ZPeriodicIncX": 0})
    assert XmlCase(path).peri_active == 4
