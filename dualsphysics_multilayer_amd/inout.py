"""``<special><inout>`` as the reference loads it (host only): the zones' points, planes, limits,
config bytes, velocity coefficients and the initial inout particles.

Mirrors ``JSphInOut::LoadXmlInit / ReadXml / Config`` (JSphInOut.cpp:129-224, 529-670),
``JSphInOutZone::ReadXml`` (JSphInOutZone.cpp:180-276), ``JSphInOutPoints`` (``Create2d_Line``,
``Create3d_Box``, ``ComputeDomainFromPoints``, ``CheckPoints``; JSphInOutPoints.cpp:198-362,
503-634), the fixed modes of ``JSphInOutVel`` and ``JSphInOutZsurf``, ``ComputeFreeDomain``
(JSphInOut.cpp:368-450), ``LoadInitPartsData`` (:675-695) and ``InitCheckProximity`` (:704-775).
The reference reads several values as float (``ReadElementFloat``): those are narrowed here the
same way, so that the derived planes and limits are the reference's.

What this core does not run raises ``CaseError`` naming the element or value: ``<circle>``,
``<particles mkfluid=...>``, ``rotate`` / ``rotateaxis``, velocity modes 1 and 3, ``flowvelocity``,
AWAS, ``imposezsurf`` modes 1 and 2, ``refilling`` 2 and more than 16 zones.
"""
from __future__ import annotations

import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
# 16-bit typecode (DualSphDef.h:186-190, 195)
CODE_TYPE_FLUID_INOUT = 0x1FE0
MAXZONES = 16
# JSphInOutDef.h:42-83, JSphInOutZone.h:67-73
VELP_UNIFORM, VELP_LINEAR, VELP_PARABOLIC = 0x00, 0x01, 0x02
VELM_FIXED, VELM_EXTRAPOLATED = 0x00, 0x08
RHOP_CONSTANT, RHOP_HYDROSTATIC, RHOP_EXTRAPOLATED = 0x00, 0x10, 0x20
CHECKINPUT_MASK = 0x80
REFILLADVANCED_MASK, REFILLSPFULL_MASK, REMOVEINPUT_MASK, REMOVEZSURF_MASK, CONVERTINPUT_MASK = 1, 2, 4, 8, 16
VELB_INLET, VELB_OUTLET, VELB_REVERSE, VELB_UNKNOWN = 0, 1, 2, 3
ZSURF_UNDEFINED, ZSURF_FIXED = 0, 1

f32 = np.float32


def _error():
    from .xmlcase import CaseError

    return CaseError


def _f(v) -> float:
    """A double narrowed to float, as a Python float."""
    return float(f32(v))


def _atof(text: str, what: str) -> float:
    try:
        return float(text)
    except (TypeError, ValueError):
        raise _error()(f"Inlet/outlet: the value of {what} is not a number: {text!r}") from None


def _check_names(ele, names: str, what: str) -> None:
    """JXml::CheckElementNames: every child (not starting with '_') is one of `names`."""
    ok = {n.lstrip("*") for n in names.split()}
    for ch in ele:
        if isinstance(ch.tag, str) and not ch.tag.startswith("_") and ch.tag not in ok:
            raise _error()(f"Inlet/outlet: the element <{ch.tag}> of <{what}> is not valid or not supported.")


def _attr(ele, child: str, attr: str, what: str, optional: bool = False, default=None):
    """Attribute `attr` of the child element `child` as text (JXml::ReadElement*)."""
    e = ele.find(child)
    if e is None or e.get(attr) is None:
        if optional:
            return default
        raise _error()(f"Inlet/outlet: the value {child}.{attr} of <{what}> is missing.")
    return e.get(attr)


def _rfloat(ele, child, attr, what, optional=False, default=0.0) -> float:
    v = _attr(ele, child, attr, what, optional, None)
    return _f(default) if v is None else _f(_atof(v, f"{child}.{attr}"))


def _rdouble(ele, child, attr, what, optional=False, default=0.0) -> float:
    v = _attr(ele, child, attr, what, optional, None)
    return float(default) if v is None else _atof(v, f"{child}.{attr}")


def _rdouble3(ele, child, what) -> np.ndarray:
    return np.array([_rdouble(ele, child, a, what) for a in "xyz"], np.float64)


def _rbool(ele, child, attr, what, optional=False, default=False) -> bool:
    v = _attr(ele, child, attr, what, optional, None)
    if v is None:
        return default
    v = v.strip().lower()
    if v in ("true", "1"):
        return True
    if v in ("false", "0"):
        return False
    raise _error()(f"Inlet/outlet: the value {child}.{attr} of <{what}> is not a valid boolean: {v!r}")


def _ruint(ele, child, attr, what, optional=False, default=0) -> int:
    v = _attr(ele, child, attr, what, optional, None)
    if v is None:
        return default
    try:
        return int(v)
    except ValueError:
        raise _error()(f"Inlet/outlet: the value {child}.{attr} of <{what}> is not an integer: {v!r}") from None


def _active(ele) -> bool:
    return (ele.get("active") or "true").strip().lower() not in ("false", "0")


def _unit(v: np.ndarray) -> np.ndarray:
    """fgeo::VecUnitary (FunGeo3d.h:289-292)."""
    m = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return v / m if m else v


def _points_count(size: float, dp: float) -> tuple[int, float]:
    """Intervals and spacing along one extent (JSphInOutPoints.cpp:239-244, 316-322)."""
    n = int(size / dp)
    d = dp
    if size - dp * n > dp * 0.95:
        n += 1
        d = size / float(n)
    return n, d


class _Zone:
    pass


def _refuse_rotation(ele, what: str) -> None:
    for tag in ("rotate", "rotateaxis"):
        if ele.find(tag) is not None:
            raise _error()(f"Inlet/outlet: <{tag}> of <{what}> is not supported by this core.")


def _create_line(z, ele, dp, posy) -> None:
    """JSphInOutPoints::Create2d_Line + ComputeDomainFromPoints (2-D)."""
    _refuse_rotation(ele, "line")
    px1, pz1 = _rfloat(ele, "point", "x", "line"), _rfloat(ele, "point", "z", "line")
    px2, pz2 = _rfloat(ele, "point2", "x", "line"), _rfloat(ele, "point2", "z", "line")
    d = np.zeros(3)
    if ele.find("direction") is not None:
        d[0], d[2] = _rfloat(ele, "direction", "x", "line"), _rfloat(ele, "direction", "z", "line")
    if d.any():
        z.direction = _unit(d)
    pt1, pt2 = np.array([px1, posy, pz1]), np.array([px2, posy, pz2])
    v = pt2 - pt1
    dist = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    npt, dpp = _points_count(dist, dp)
    npt += 1
    vec = _unit(v) * dpp
    z.points = np.array([pt1 + vec * float(p) for p in range(npt)], np.float64).reshape(-1, 3)
    # ComputeDomainFromPoints (JSphInOutPoints.cpp:503-528)
    pmin, pmax = z.points.min(axis=0), z.points.max(axis=0)
    dir1 = z.direction * (dp / 2)
    nfar = 2 * z.layers + 1
    dir2 = _unit(pmax - pmin) * (dp / 2)
    pnearmin, pnearmax = pmin + dir1 - dir2, pmax + dir1 + dir2
    pfarmin = pnearmin - dir1 * nfar
    dirup, dirfar = pnearmax - pnearmin, pfarmin - pnearmin
    pd = np.zeros((10, 3))
    pd[0] = pnearmin
    pd[1] = pd[0] + dirup
    pd[2] = pd[0] + dirup + dirfar
    pd[3] = pd[0] + dirfar
    pd[8] = (pd[1] + pd[0]) / 2
    pd[9] = pd[8] + z.direction * (dp * z.layers)
    z.ptdom = pd


def _create_box(z, ele, dp) -> None:
    """JSphInOutPoints::Create3d_Box."""
    _refuse_rotation(ele, "box")
    pt0, spt = _rdouble3(ele, "point", "box"), _rdouble3(ele, "size", "box")
    if spt[0] != 0 and spt[1] != 0 and spt[2] != 0:
        raise _error()("Inlet/outlet: <box> size: One size of axis must be zero.")
    ptx, pty, ptz = pt0 + [spt[0], 0, 0], pt0 + [0, spt[1], 0], pt0 + [0, 0, spt[2]]
    d = _unit(_rdouble3(ele, "direction", "box"))
    if d.any():
        z.direction = _unit(d)
    (npx, dpx), (npy, dpy), (npz, dpz) = (_points_count(s, dp) for s in spt)
    npx, npy, npz = npx + 1, npy + 1, npz + 1
    zero = np.zeros(3)
    vx = _unit(ptx - pt0) * dpx if spt[0] else zero
    vy = _unit(pty - pt0) * dpy if spt[1] else zero
    vz = _unit(ptz - pt0) * dpz if spt[2] else zero
    pts = [pt0 + vx * float(ix) + vy * float(iy) + vz * float(iz)
           for iz in range(npz) for iy in range(npy) for ix in range(npx)]
    z.points = np.array(pts, np.float64).reshape(-1, 3)
    if npz == 1:
        vxx, vyy = vx * float(npx), vy * float(npy)
    elif npy == 1:
        vxx, vyy = vx * float(npx), vz * float(npz)
    elif npx == 1:
        vxx, vyy = vy * float(npy), vz * float(npz)
    else:
        raise _error()("Inlet/outlet: <box>: Configuration is invalid to calculate domain.")
    dir1 = z.direction * (dp / 2)
    nfar = 2 * z.layers + 1
    pd = np.zeros((10, 3))
    pd[0] = pt0 + dir1 - _unit(vxx) * (dp / 2) - _unit(vyy) * (dp / 2)
    pd[1] = pd[0] + vxx
    pd[2] = pd[1] + vyy
    pd[3] = pd[0] + vyy
    for k in range(4):
        pd[4 + k] = pd[k] - dir1 * nfar
    pd[8] = (pd[0] + pd[2]) / 2
    pd[9] = pd[8] + z.direction * (dp * z.layers)
    z.ptdom = pd


def _read_velocity(z, ele) -> None:
    """JSphInOutVel::ReadXml, DefineBehaviour and ComputeInitialVel for the fixed and the
    extrapolated mode (JSphInOutVel.cpp:107-264, 329-337, 399-420)."""
    E = _error()
    xele = ele.find("imposevelocity")
    if xele is None:
        raise E(f"Inlet/outlet zone {z.id}: <imposevelocity> is missing.")
    try:
        mode = int(xele.get("mode"))
    except (TypeError, ValueError):
        raise E(f"Inlet/outlet zone {z.id}: imposevelocity mode is missing or not valid.") from None
    if mode in (1, 3):
        raise E(f"Inlet/outlet zone {z.id}: imposevelocity mode={mode} "
                f"({'variable' if mode == 1 else 'interpolated'} velocity) is not supported by this core.")
    if mode not in (0, 2):
        raise E(f"Inlet/outlet zone {z.id}: imposevelocity mode={mode}: Value is not valid.")
    if xele.find("flowvelocity") is not None:
        raise E(f"Inlet/outlet zone {z.id}: <flowvelocity> is not supported by this core.")
    if xele.find("awas") is not None:
        raise E(f"Inlet/outlet zone {z.id}: <awas> is not supported by this core.")
    z.velmode = VELM_FIXED if mode == 0 else VELM_EXTRAPOLATED
    z.velprofile = VELP_UNIFORM
    z.inputvel = [0.0, 0.0, 0.0]
    z.inputvelposz = [0.0, 0.0, 0.0]
    coefs = np.zeros(4, f32)
    if mode == 0:
        have = [xele.find(t) is not None for t in ("velocity", "velocity2", "velocity3")]
        if sum(have) > 1:
            raise E(f"Inlet/outlet zone {z.id}: Several definitions for velocity were found.")
        _check_names(xele, "velocity velocity2 velocity3 flowvelocity", "imposevelocity")
        w = "imposevelocity"
        if have[0] or not any(have):
            z.inputvel[0] = _rfloat(xele, "velocity", "v", w)
            coefs[0] = f32(z.inputvel[0]) * f32(1.0)  # InputVel*FlowToVel
        if have[1]:
            z.velprofile = VELP_LINEAR
            v, v2 = f32(_rfloat(xele, "velocity2", "v", w)), f32(_rfloat(xele, "velocity2", "v2", w))
            pz, pz2 = f32(_rfloat(xele, "velocity2", "z", w)), f32(_rfloat(xele, "velocity2", "z2", w))
            z.inputvel[:2], z.inputvelposz[:2] = [float(v), float(v2)], [float(pz), float(pz2)]
            m = f32(f32(v2 - v) / f32(pz2 - pz))
            coefs[0], coefs[1] = m, f32(v - f32(m * pz))
        if have[2]:
            z.velprofile = VELP_PARABOLIC
            v = [f32(_rfloat(xele, "velocity3", a, w)) for a in ("v", "v2", "v3")]
            p = [f32(_rfloat(xele, "velocity3", a, w)) for a in ("z", "z2", "z3")]
            z.inputvel, z.inputvelposz = [float(x) for x in v], [float(x) for x in p]
            coefs[:3] = _parabola_coefs(v, p)
        vmin, vmax = min(z.inputvel[:1 + z.velprofile]), max(z.inputvel[:1 + z.velprofile])
    else:
        vmin, vmax = -FLT_MAX, FLT_MAX
    z.velmin, z.velmax = vmin, vmax
    if vmin >= 0 and vmax >= 0:
        z.velbehaviour = VELB_INLET
    elif vmin <= 0 and vmax <= 0:
        z.velbehaviour = VELB_OUTLET
    elif vmin < 0 <= vmax and vmin != -FLT_MAX and vmax != FLT_MAX:
        z.velbehaviour = VELB_REVERSE
    else:
        z.velbehaviour = VELB_UNKNOWN
    z.veldata = np.stack([coefs, np.zeros(4, f32)])


def _parabola_coefs(v, p) -> np.ndarray:
    """a, b, c of vel = a z^2 + b z + c through three (z, v), in float as the reference's
    fmath::InverseMatrix3x3 (FunctionsMath.h:99-101, 128-143; JSphInOutVel.cpp:410-416)."""
    d = np.array([[f32(p[i] * p[i]), p[i], f32(1)] for i in range(3)], f32)
    det = f32(d[0, 0] * d[1, 1] * d[2, 2] + d[0, 1] * d[1, 2] * d[2, 0] + d[0, 2] * d[1, 0] * d[2, 1]
              - d[2, 0] * d[1, 1] * d[0, 2] - d[2, 1] * d[1, 2] * d[0, 0] - d[2, 2] * d[1, 0] * d[0, 1])
    inv = np.zeros((3, 3), f32)
    if det:
        inv[0, 0] = (d[1, 1] * d[2, 2] - d[1, 2] * d[2, 1]) / det
        inv[0, 1] = -(d[0, 1] * d[2, 2] - d[0, 2] * d[2, 1]) / det
        inv[0, 2] = (d[0, 1] * d[1, 2] - d[0, 2] * d[1, 1]) / det
        inv[1, 0] = -(d[1, 0] * d[2, 2] - d[1, 2] * d[2, 0]) / det
        inv[1, 1] = (d[0, 0] * d[2, 2] - d[0, 2] * d[2, 0]) / det
        inv[1, 2] = -(d[0, 0] * d[1, 2] - d[0, 2] * d[1, 0]) / det
        inv[2, 0] = (d[1, 0] * d[2, 1] - d[1, 1] * d[2, 0]) / det
        inv[2, 1] = -(d[0, 0] * d[2, 1] - d[0, 1] * d[2, 0]) / det
        inv[2, 2] = (d[0, 0] * d[1, 1] - d[0, 1] * d[1, 0]) / det
    return np.array([f32(inv[r, 0] * v[0] + inv[r, 1] * v[1] + inv[r, 2] * v[2]) for r in range(3)], f32)


def _read_zsurf(z, ele) -> None:
    """JSphInOutZsurf::ReadXml for the fixed mode (JSphInOutZsurf.cpp:100-124)."""
    E = _error()
    z.zsurfmode, z.inputzsurf, z.removezsurf = ZSURF_UNDEFINED, FLT_MAX, False
    xele = ele.find("imposezsurf")
    if xele is None:
        return
    try:
        mode = int(xele.get("mode"))
    except (TypeError, ValueError):
        raise E(f"Inlet/outlet zone {z.id}: imposezsurf mode is missing or not valid.") from None
    if mode in (1, 2):
        raise E(f"Inlet/outlet zone {z.id}: imposezsurf mode={mode} "
                f"({'variable' if mode == 1 else 'calculated'} zsurf) is not supported by this core.")
    if mode != 0:
        raise E(f"Inlet/outlet zone {z.id}: imposezsurf mode={mode}: Value is not valid.")
    z.zsurfmode = ZSURF_FIXED
    z.removezsurf = _rbool(xele, "remove", "value", "imposezsurf", True, False)
    _check_names(xele, "remove zsurf zbottom", "imposezsurf")
    z.inputzsurf = _rfloat(xele, "zsurf", "value", "imposezsurf")


def _read_zone(zid: int, ele, case, messages: list):
    """JSphInOutZone::ReadXml (JSphInOutZone.cpp:180-276) and CheckConfig (:128-149)."""
    E = _error()
    dp, sim2d, posy = case.dp, bool(case.data2d), float(case.data2d_posy)
    mapmin, mapmax = (np.asarray(v, np.float64) for v in case.map_limits())
    z = _Zone()
    z.id = zid
    for old in ("userefilling", "convertfluid"):
        if ele.find(old) is not None:
            raise E(f"Inlet/outlet zone {zid}: <{old}> is not supported by current inlet/outlet version.")
    _check_names(ele, "refilling inputtreatment layers zone2d zone3d imposevelocity imposerhop imposezsurf",
                 "inoutzone")
    z.inputtreatment = _ruint(ele, "inputtreatment", "value", "inoutzone")
    if z.inputtreatment not in (0, 1, 2):
        raise E(f"Inlet/outlet zone {zid}: inputtreatment value={z.inputtreatment} is not valid.")
    z.refilling = _ruint(ele, "refilling", "value", "inoutzone")
    if z.refilling == 2:
        raise E(f"Inlet/outlet zone {zid}: refilling value=2 (advanced refilling) is not supported by this core.")
    if z.refilling not in (0, 1):
        raise E(f"Inlet/outlet zone {zid}: refilling value={z.refilling} is not valid.")
    z.layers = _ruint(ele, "layers", "value", "inoutzone")
    if z.layers < 1:
        raise E(f"Inlet/outlet zone {zid}: layers: Minumum number of layers is 1.")
    if z.layers > 250:
        raise E(f"Inlet/outlet zone {zid}: layers: Maximum number of layers is 250.")
    # -- points (JSphInOutPoints::CreatePoints)
    zname = "zone2d" if sim2d else "zone3d"
    lis = ele.find(zname)
    if lis is None:
        raise E(f"Inlet/outlet zone {zid}: <{zname}> is missing.")
    z.direction = np.zeros(3)
    z.points = None
    for ch in lis:
        cmd = ch.tag
        if not isinstance(cmd, str) or not cmd or cmd[0] == "_":
            continue
        if z.points is not None:
            raise E("Only one description zone is allowed for inlet/outlet points.")
        if cmd == "particles":
            raise E(f"Inlet/outlet zone {zid}: <particles mkfluid=\"{ch.get('mkfluid')}\"> (points from fluid "
                    "particles) is not supported by this core.")
        if cmd == "circle" and not sim2d:
            raise E(f"Inlet/outlet zone {zid}: <circle> is not supported by this core.")
        if cmd == "line" and sim2d:
            _create_line(z, ch, dp, posy)
        elif cmd == "box" and not sim2d:
            _create_box(z, ch, dp)
        else:
            raise E(f"Inlet/outlet zone {zid}: the element <{cmd}> of <{zname}> is not valid.")
    # CheckPoints (JSphInOutPoints.cpp:587-634): one layer more, the real limit
    if sim2d and z.direction[1] != 0:
        raise E(f"Inlet/outlet zone {zid}: Direction.y is not zero.")
    if not z.direction.any():
        raise E(f"Inlet/outlet zone {zid}: Direction vector is zero.")
    if z.points is None or not len(z.points):
        raise E(f"Inlet/outlet zone {zid}: There are not defined points.")
    for c in range(z.layers + 1):
        ps = z.points - z.direction * float(dp * c)
        bad = ~((mapmin < ps).all(axis=1) & (ps < mapmax).all(axis=1))
        if bad.any():
            e = ps[np.flatnonzero(bad)[0]]
            raise E("Point for inlet conditions with position (%g,%g,%g) is outside the domain." % tuple(e))
    z.zoneposmin, z.zoneposmax = z.points.min(axis=0), z.points.max(axis=0)
    # LoadDomain (JSphInOutZone.cpp:154-175)
    nd = 4 if sim2d else 8
    z.boxlimitmin = z.ptdom[:nd].min(axis=0).astype(f32)
    z.boxlimitmax = z.ptdom[:nd].max(axis=0).astype(f32)
    if sim2d:
        z.boxlimitmin[1] = f32(posy - dp * .1)
        z.boxlimitmax[1] = f32(posy + dp * .1)
    z.ptplane = z.ptdom[8].copy()
    u = _unit(z.direction)
    z.plane = np.array([u[0], u[1], u[2], -u[0] * z.ptplane[0] - u[1] * z.ptplane[1] - u[2] * z.ptplane[2]]).astype(f32)
    z.nptinit = len(z.points)
    _read_velocity(z, ele)
    _read_zsurf(z, ele)
    xele = ele.find("imposerhop")
    z.rhopmode = RHOP_CONSTANT
    if xele is not None:
        try:
            mode = int(xele.get("mode"))
        except (TypeError, ValueError):
            raise E(f"Inlet/outlet zone {zid}: imposerhop mode is missing or not valid.") from None
        if mode not in (0, 1, 2):
            raise E(f"Inlet/outlet zone {zid}: imposerhop mode={mode}: Value is not valid.")
        z.rhopmode = (RHOP_CONSTANT, RHOP_HYDROSTATIC, RHOP_EXTRAPOLATED)[mode]
        for old in ("zsurf", "zbottom"):
            if ele.find(old) is not None:
                raise E(f"Inlet/outlet zone {zid}: <{old}> is not supported by current inlet/outlet version.")
        _check_names(xele, "", "imposerhop")
    # initial valid points according to zsurf (JSphInOutZone.cpp:263-266)
    if z.zsurfmode == ZSURF_UNDEFINED or z.refilling == 0 or z.inputzsurf == FLT_MAX:
        z.pointsinit = np.ones(z.nptinit, bool)
    else:
        z.pointsinit = z.points[:, 2].astype(f32) <= f32(z.inputzsurf)
    z.npartinit = int(z.pointsinit.sum()) * z.layers
    z.inputcheck = bool(z.removezsurf or z.inputtreatment != 0)
    # CheckConfig
    b, rf, it = z.velbehaviour, z.refilling, z.inputtreatment
    warn = lambda t: messages.append(f"*** WARNING: Inlet/outlet {zid}: {t}")  # noqa: E731
    if rf == 0 and z.removezsurf:
        warn("If RemoveZsurf==true then RefillingMode==SimpleFull is equivalent to SimpleZsurf.")
    if b == VELB_UNKNOWN:
        warn("Velocity limits are unknown and RefillingMode==SimpleFull/SimpleZsurf is invalid for reverse flows.")
    if b == VELB_REVERSE:
        raise E(f"Inlet/outlet {zid}: RefillingMode==SimpleFull/SimpleZsurf is invalid for reverse flows.")
    if it in (0, 2) and b == VELB_OUTLET:
        raise E(f"Inlet/outlet {zid}: InputTreatment=={'Free' if it == 0 else 'Remove'} is invalid for outlet flows.")
    if it == 1 and b == VELB_INLET:
        warn("InputTreatment==Convert is not recommended for inlet flows.")
    if it in (0, 2) and b == VELB_UNKNOWN:
        warn(f"InputTreatment=={'Free' if it == 0 else 'Remove'} is not recommended for undefined flows since it is "
             "invalid for outlet flows.")
    if z.rhopmode == RHOP_HYDROSTATIC and z.zsurfmode == ZSURF_UNDEFINED:
        raise E(f"Inlet/outlet {zid}: Z-Surface is undefined for hydrostatic density calculation.")
    if z.velmode == VELM_EXTRAPOLATED:
        warn("VelocityMode==Extrapolated is not recommended for inlet (or reverse) flows.")
    # GetConfigZone / GetConfigUpdate (JSphInOutZone.cpp:288-318)
    z.cfgzone = z.velprofile | z.velmode | z.rhopmode | (CHECKINPUT_MASK if z.inputcheck else 0)
    z.cfgupdate = ((REFILLSPFULL_MASK if rf == 0 else 0) | (REMOVEINPUT_MASK if it == 2 else 0) |
                   (REMOVEZSURF_MASK if z.removezsurf else 0) | (CONVERTINPUT_MASK if it == 1 else 0))
    z.width = _f(dp * z.layers)
    return z


def _free_domain(zones, freecentre, mapmin, mapmax, sim2d: bool):
    """JSphInOut::ComputeFreeDomain (JSphInOut.cpp:368-450), in float as there."""
    E = _error()
    if freecentre is None:
        fc = ((np.asarray(mapmax) + np.asarray(mapmin)) / 2).astype(f32)
    else:
        fc = np.asarray(freecentre, f32)
    nz = len(zones)
    zol = np.full((nz, 3), f32(FLT_MAX), f32)
    for ci, z in enumerate(zones):
        for a in range(3):
            zol[ci, a] = z.boxlimitmin[a] if fc[a] <= z.boxlimitmin[a] else (
                z.boxlimitmax[a] if fc[a] >= z.boxlimitmax[a] else f32(FLT_MAX))
        if zol[ci, 0] == f32(FLT_MAX) and zol[ci, 2] == f32(FLT_MAX) and (sim2d or zol[ci, 1] == f32(FLT_MAX)):
            raise E("FreeCentre position (%g,%g,%g) is within the inout zone %d. FreeCentre must be changed in XML "
                    "file." % (fc[0], fc[1], fc[2], ci))
    nsel = 2 if sim2d else 3
    axis_of = {1: 0, 2: 2, 3: 1}  # the reference tries X, then Z, then Y
    bestsize = -FLT_MAX
    bestmin = bestmax = None
    sel = [0] * nz
    dmin = [None] * (nz + 1)
    dmax = [None] * (nz + 1)
    dmin[0], dmax[0] = np.asarray(mapmin).astype(f32), np.asarray(mapmax).astype(f32)
    ci = 0
    while True:
        if sel[ci] < nsel:
            sel[ci] += 1
            pmin, pmax = dmin[ci].copy(), dmax[ci].copy()
            a = axis_of[sel[ci]]
            if zol[ci, a] != f32(FLT_MAX):
                if zol[ci, a] <= fc[a]:
                    pmin[a] = max(pmin[a], zol[ci, a])
                else:
                    pmax[a] = min(pmax[a], zol[ci, a])
                ss = (pmax - pmin).astype(f32)
                size = float(f32(ss[0] * ss[2]) if sim2d else f32(f32(ss[0] * ss[1]) * ss[2]))
                if size > bestsize:
                    if ci + 1 == nz:
                        bestsize, bestmin, bestmax = size, pmin, pmax
                    else:
                        ci += 1
                        sel[ci] = 0
                        dmin[ci], dmax[ci] = pmin, pmax
        else:
            sel[ci] = 0
            if ci > 0:
                ci -= 1
            else:
                break
    return fc, bestmin, bestmax


def load_inout(node, case, messages: list) -> dict:
    """The ``<inout>`` element of a loaded case (its constants, map limits and particles are
    known) -> the dict ``XmlCase.inout``.  Appends the reference's warnings to `messages`."""
    E = _error()
    if node.find("userefilling") is not None:
        raise E("Inlet/outlet: <userefilling> is not supported by current inlet/outlet version.")
    _check_names(node, "memoryresize useboxlimit determlimit extrapolatemode refillingrate inoutzone", "inout")
    io = {}
    io["memoryresize0"] = _rfloat(node, "memoryresize", "size0", "inout", True, 2.0)
    if io["memoryresize0"] < 0:
        raise E("Value of memoryresize.size0 lower than zero is invalid.")
    # (size: the growth of the arrays during a run, which this core does not do; checked only)
    if _rfloat(node, "memoryresize", "size", "inout", True, 4.0) < 0:
        raise E("Value of memoryresize.size lower than zero is invalid.")
    io["determlimit"] = _rfloat(node, "determlimit", "value", "inout", True, 1e+3)
    # (the reference's CPU solver raises mode 1 to 2; its GPU solver and this core keep it)
    io["extrapolatemode"] = min(3, max(1, _ruint(node, "extrapolatemode", "value", "inout", True, 1)))
    io["useboxlimit"] = _rbool(node, "useboxlimit", "value", "inout", True, True)
    ub = node.find("useboxlimit")
    freecentre = None
    if ub is not None and ub.find("freecentre") is not None:
        freecentre = [_rfloat(ub, "freecentre", a, "useboxlimit") for a in "xyz"]
    if any(abs(g) > 0 for g in case.gravity[:2]):
        messages.append("*** WARNING: Only gravity in Z (0,0,%g) is used in inlet/outlet code (e.g.: hydrostatic "
                        "density or water elevation calculation)." % case.gravity[2])
    zones = []
    for ele in node.findall("inoutzone"):
        if not _active(ele):
            continue
        if len(zones) >= MAXZONES:
            raise E("Maximum number of inlet/outlet zones has been reached.")
        zones.append(_read_zone(len(zones), ele, case, messages))
    if not zones:
        raise E("Inlet/outlet: no active <inoutzone> was found.")
    mapmin, mapmax = case.map_limits()
    sim2d = bool(case.data2d)
    fc, flmin, flmax = _free_domain(zones, freecentre, mapmin, mapmax, sim2d)
    io["freecentre"], io["freelimitmin"], io["freelimitmax"] = fc, flmin, flmax
    # CoefHydro (JSphInOut.cpp:536), in float as CSP holds the constants
    io["coefhydro"] = float(f32(f32(f32(case.rhop0) * f32(-f32(case.gravity[2]))) / f32(case.cteb)))
    npfull = sum(z.nptinit * z.layers for z in zones)
    io["npresizeplus0"] = int(f32(io["memoryresize0"]) * f32(npfull))
    # -- initial inout particles (JSphInOutZone::LoadInitialParticles, JSphInOut::LoadInitPartsData)
    idmax = int(case.idp.max())
    pos, code = [], []
    for ci, z in enumerate(zones):
        for layer in range(z.layers):
            d = z.direction * (-case.dp * layer)
            pos.append(z.points[z.pointsinit] + d)
        code.append(np.full(z.npartinit, CODE_TYPE_FLUID_INOUT + ci, np.uint16))
    pos = np.concatenate(pos).reshape(-1, 3)
    code = np.concatenate(code)
    n = len(pos)
    vel = np.zeros((n, 3), f32)
    io["init"] = dict(idp=np.arange(idmax + 1, idmax + 1 + n, dtype=np.uint32), pos=np.ascontiguousarray(pos),
                      code=code, vel=vel, rhop=np.full(n, f32(1000), f32))
    io["zones"] = [dict(id=z.id, layers=z.layers, refilling=z.refilling, inputtreatment=z.inputtreatment,
                        direction=z.direction, ptplane=z.ptplane, plane=z.plane, width=z.width,
                        cfgzone=z.cfgzone, cfgupdate=z.cfgupdate, velmode=z.velmode, velprofile=z.velprofile,
                        veldata=z.veldata, velbehaviour=z.velbehaviour, rhopmode=z.rhopmode,
                        zsurfmode=z.zsurfmode, zsurf=z.inputzsurf, removezsurf=z.removezsurf,
                        boxlimitmin=z.boxlimitmin, boxlimitmax=z.boxlimitmax, ptdom=z.ptdom,
                        zoneposmin=z.zoneposmin, zoneposmax=z.zoneposmax, nptinit=z.nptinit,
                        npartinit=z.npartinit, points=z.points, pointsinit=z.pointsinit) for z in zones]
    io["outignore"] = _check_proximity(case, io["init"]["pos"], messages)
    return io


def _check_proximity(case, newpos: np.ndarray, messages: list) -> np.ndarray:
    """JSphInOut::InitCheckProximity (JSphInOut.cpp:704-775): the indices of the case's fluid
    particles within 0.8 dp of an initial inout particle (they start as CODE_OUTIGNORE); a
    boundary or another inout particle that close is an error."""
    E = _error()
    dist = case.dp * 0.8
    allpos = np.concatenate([np.asarray(case.pos, np.float64), newpos])
    n0 = len(case.pos)
    # cells of size dist from the inout particles' corner: a particle can only be close to an
    # inout particle of its own or a neighbouring cell
    lo = newpos.min(axis=0) - 2 * dist
    cells = np.floor((allpos - lo) / dist).astype(np.int64)
    span = int(cells.max()) + 3

    def key(c):
        return ((c[:, 0] + 1) * span + (c[:, 1] + 1)) * span + (c[:, 2] + 1)

    inbox = (cells >= -1).all(axis=1)
    newkeys = np.unique(key(cells[n0:]))
    cand = np.zeros(len(allpos), bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                cand |= inbox & np.isin(key(cells + np.array([dx, dy, dz])), newkeys)
    near = np.zeros(len(allpos), bool)
    d2max = dist * dist
    for q in np.flatnonzero(cand):
        d = newpos - allpos[q]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        if q >= n0:
            d2[q - n0] = np.inf  # not itself
        near[q] = bool((d2 <= d2max).any())  # JSimpleNeigs.cpp:205
    nfluid = int(near[case.npb:n0].sum())
    nbound = int(near[:case.npb].sum())
    ninout = int(near[n0:].sum())
    if nbound + ninout:
        raise E("There are inout fluid or boundary particles too close to inout particles. Check VTK file "
                "CfgInOut_ErrorParticles.vtk with excluded particles.")
    if nfluid:
        messages.append("*** WARNING: %u fluid particles were excluded since they are too close to inout particles. "
                        "Check VTK file CfgInOut_ExcludedParticles.vtk" % nfluid)
    return np.flatnonzero(near[:n0]).astype(np.int64)
