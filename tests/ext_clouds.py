"""Off-lattice clouds for the Laminar+SPS / shifting interaction (csrc/sph_ext.hip) and a
cell-free reference of it, on top of tests/clouds.py.

The CPU oracle refuses ViscoTreatment 2 and every shifting mode, so the reference here is
written from the semantics of JSphCpu.cpp:631-822 (InteractionForcesFluid with
tvisco = VISCO_LaminarSPS and / or shift = true) and :929-954 (ComputeSpsTau), not from the
HIP kernel; its noise floor is its own float32 evaluation (as tests/dem_clouds.brute_ft).

* ``make``       the clouds of clouds.make plus two new ones:
                 symwall    the sym cloud and a dense boundary patch touching y = 0 under its
                            first-row fluid: a 6-cell (9 half-cell) range of one boundary row of
                            the first rows in y holds more than 208 particles, so the
                            [record, image] layout of the ordered bound pass needs more than
                            ExtCap = 416 records and is drained in segments;
                 mixedwall  the blob cloud with explicit codes: half of the boundary patch
                            below the blob MOVING (at rest, no motion program), half fixed
                            (case order fixed, moving, fluid), for ShiftMode NoFixed
* ``brute_ext``  one interaction over ALL pairs in float64, or in float32 (every pair term in
                 float32 with dr the float of the double difference, summed sequentially in
                 float32 p1 major / p2 ascending): ar, ace and its terms, viscdt, the velocity
                 gradients, tau, the shifting sums and the frozen set
* ``e32``        the distance of the float32 evaluation from the float64 one per quantity

A helper module, not a conftest.
"""
from __future__ import annotations

import copy

import numpy as np

import clouds
from dualsphysics_multilayer_amd.case import CODE_TYPE_FIXED, CODE_TYPE_FLUID, DamBreakCase

CODE_TYPE_MOVING = 0x0800
EXTCAP = {1: 416, 2: 312}  # csrc/sph_ext.hip ExtCap<TVISCO>: staged records per segment
NEW = ("symwall", "mixedwall")
# seeds for which the added particles bring no pair inside clouds.SHELL (tests/test_ext_clouds_cpu.py)
SEEDS = {"symwall": 15, "mixedwall": 12}


class _CodedCase(DamBreakCase):
    """A DamBreakCase copy whose particle codes travel to the solver."""

    explicit_codes = True

    @property
    def code(self):
        return self._code


# symwall's patch, in cells of 2h: inside the cell row (cy 0, cz 0) and the half-cell row
# (cy 0, cz 1), 4 cells (8 half-cells) long in x, below the sym cloud's dense first-row fluid
# (x 3.3-5.7, y < 0.5, z 2.0-2.5 and the first-row fluid from z = 1)
_SYMWALL_PATCH = ([3.4, 1e-3, 0.55], [5.6, 0.45, 0.95], 330)


def make(name, small=False, seed=None, **kw):
    """clouds.make for its names; symwall and mixedwall as described in the module docstring."""
    if name not in NEW:
        return clouds.make(name, small=small, seed=seed, **kw)
    seed = SEEDS[name] if seed is None else seed
    mk = {k: kw.pop(k) for k in ("dp", "vamp", "rhoamp") if k in kw}
    dp = mk.pop("dp", clouds.DP)
    coefh = float(kw.get("coefh", 1.0))
    kw.setdefault("celldomfixed", True)
    src = "sym" if name == "symwall" else "blob"
    bound_pos, fluid_pos, lo, hi = clouds._points(src, clouds.SEEDS[src], coefh, dp, False)
    base = clouds._base(dp, name == "symwall", tuple(sorted(kw.items())))
    cs = clouds._cell(coefh, dp)
    code = None
    if name == "symwall":
        a, b, n = _SYMWALL_PATCH
        patch = clouds._box(np.random.default_rng(seed), n, a, b) * cs
        bound_pos = np.concatenate([bound_pos, patch])
    else:
        # the blob's patch (x 3.0-5.0 cells, z 1.3-2.0) split at x = 4 cells: the moving half last
        x, z = bound_pos[:, 0] / cs, bound_pos[:, 2] / cs
        moving = (z > 1.2) & (x >= 4.0)
        bound_pos = np.concatenate([bound_pos[~moving], bound_pos[moving]])
        code = np.full(len(bound_pos) + len(fluid_pos), CODE_TYPE_FLUID, np.uint16)
        code[:len(bound_pos)] = CODE_TYPE_FIXED
        code[len(bound_pos) - int(moving.sum()):len(bound_pos)] = CODE_TYPE_MOVING
    c = clouds.cloud_case(base, bound_pos, fluid_pos, seed + 1000, lo, hi, **mk)
    c._cloud_key = ("ext-" + name, seed, coefh, dp, False)
    if code is not None:
        c.__class__ = _CodedCase
        c._code = code
    return c


def plain(case, **changes):
    """The same particles as a case of other options (e.g. shift_mode = 0 for the oracle),
    without explicit codes."""
    c = copy.copy(case)
    if isinstance(c, _CodedCase):
        c.__class__ = DamBreakCase
    for k, v in changes.items():
        setattr(c, k, v)
    return c


def codes(case):
    return np.asarray(case.code, np.uint16)


# ----------------------------------------------------------------------------------------
def sps_tau(K, grad, rho, T=np.float64):
    """ComputeSpsTau (JSphCpu.cpp:929-954): grad [n][6] -> tau [n][6]."""
    g = grad.astype(T)
    smag, blin = T(np.float32(K["spssmag"])), T(np.float32(K["spsblin"]))
    xx, xy, xz, yy, yz, zz = (g[:, k] for k in range(6))
    pow1 = xx * xx + yy * yy + zz * zz
    prr = pow1 + pow1 + xy * xy + xz * xz + yz * yz
    visc_sps = smag * np.sqrt(prr)
    div_u = xx + yy + zz
    sps_k = T(2.0 / 3.0) * visc_sps * div_u
    sumsps = -(sps_k + blin * prr)
    two = visc_sps + visc_sps
    one_rho2 = T(1) / rho.astype(T)
    return np.stack([one_rho2 * (two * xx + sumsps), one_rho2 * (visc_sps * xy), one_rho2 * (visc_sps * xz),
                     one_rho2 * (two * yy + sumsps), one_rho2 * (visc_sps * yz), one_rho2 * (two * zz + sumsps)],
                    axis=1).astype(T)


def brute_ext(case, K, ddt, tau=None, dtype=np.float64):
    """One Interaction_Forces of a single-phase case with Laminar+SPS viscosity and / or
    shifting over all pairs, in the case's particle order (index = idp).  `tau` [np][6]: the
    stress tensor the pairs read (a previous call's; default zero; bound rows 0).  Returns ar
    (continuity + DDT by the rules of clouds.brute), ace = ace_press + ace_visc (artificial
    or laminar) + ace_sps, viscdt and viscdt_sens, grad [np][6] and the tau it gives
    (Laminar+SPS), shift [np][4] (the sums over every pair, meaningful for a particle that is
    not frozen) and frozen (per the case's ShiftMode), amb_ddt / amb_frozen (fluid particles
    with a BOUND neighbour inside clouds.SHELL: their DDT switch / frozen flag hangs on the
    last bit of r^2), amb_any (any neighbour inside the shell)."""
    T = dtype
    f = lambda k: T(np.float32(K[k]))  # noqa: E731
    tvisco, smode = int(case.tvisco), int(case.shift_mode)
    sym = bool(getattr(case, "symmetry", False))
    assert not (sym and tvisco == 2), "Symmetry with Laminar+SPS is refused by the core"
    P = clouds.pairs(case, K)
    n, npb = case.np, case.npb
    i, j = P["i"], P["j"]
    fi, fj = i >= npb, j >= npb
    amb_any = np.zeros(n, bool)
    amb_any[i[P["shell"] & fi]] = True
    amb_b = np.zeros(n, bool)
    amb_b[i[P["shell"] & fi & ~fj]] = True
    use = P["real"] & (fi | fj)
    i, j, fi, fj, im = i[use], j[use], fi[use], fj[use], P["image"][use]
    dr = P["dr"][use].astype(np.float32).astype(T) if T is np.float32 else P["dr"][use]
    drx, dry, drz = dr[:, 0], dr[:, 1], dr[:, 2]
    rr2 = drx * drx + dry * dry + drz * drz
    rad = np.sqrt(rr2)
    vel, rho = case.vel.astype(T), case.rhop.astype(T)
    press = clouds.pressure(case, K).astype(T)
    v2 = vel[j].copy()
    v2[im, 1] = -v2[im, 1]
    dvx, dvy, dvz = vel[i, 0] - v2[:, 0], vel[i, 1] - v2[:, 1], vel[i, 2] - v2[:, 2]
    rho1, rho2 = rho[i], rho[j]
    h, eta2, cbar = f("kernelh"), f("eta2"), T(np.float32(K["cs0"]))
    cubic = int(K["kernel"]) == 1
    if cubic:
        q = rad / h
        far = rad > h
        w1 = T(2) - q
        fac = np.where(far, f("cub_c2") * w1 * w1 / rad, (f("cub_c1") * q + f("cub_d1") * q * q) / rad).astype(T)
        wab = np.where(far, f("cub_a24") * w1 * w1 * w1,
                       f("cub_a2") * (T(1) + (T(0.75) * q - T(1.5)) * q * q)).astype(T)
    else:
        q = rad / h
        w1 = T(1) - T(0.5) * q
        fac = (f("bwen") * q * w1 * w1 * w1 / rad).astype(T)
    frx, fry, frz = fac * drx, fac * dry, fac * drz
    m2 = np.where(fj, f("massfluid"), f("massbound")).astype(T)
    ones = np.ones(len(i), bool)

    def acc(w, mask=ones):
        """Sum per p1: float64 by bincount, float32 sequentially in pair order."""
        if T is np.float32:
            out = np.zeros(n, np.float32)
            np.add.at(out, i[mask], w[mask].astype(np.float32))
            return out
        return np.bincount(i[mask], weights=w[mask], minlength=n)

    def acc3(wx, wy, wz, mask):
        return np.stack([acc(wx, mask), acc(wy, mask), acc(wz, mask)], axis=1)

    # continuity: fluid p1 with every p2, bound p1 with fluid p2
    ar_cont = acc(m2 * (dvx * frx + dvy * fry + dvz * frz) * (rho1 / rho2))
    # momentum (fluid p1)
    prs = (press[i] + press[j]) / (rho1 * rho2)
    if cubic:
        fab = wab * f("cub_od_wdeltap")
        fab = fab * fab
        fab = fab * fab
        t1 = press[i] / (rho1 * rho1) * np.where(press[i] > 0, T(0.01), T(-0.2))
        t2 = press[j] / (rho2 * rho2) * np.where(press[j] > 0, T(0.01), T(-0.2))
        prs = prs + fab * (t1 + t2)
    p_vpm = (-prs * m2).astype(T)
    ace_press = acc3(p_vpm * frx, p_vpm * fry, p_vpm * frz, fi)
    dot = drx * dvx + dry * dvy + drz * dvz
    dot3 = drx * frx + dry * fry + drz * frz
    re = rr2 + eta2
    dot_rr2 = dot / re
    visco = np.where(fj, f("visco"), T(np.float32(K["visco"]) * np.float32(K["viscoboundfactor"]))).astype(T)
    grad = np.zeros((n, 6), T)
    ace_sps = np.zeros((n, 3), T)
    if tvisco == 1:
        pi_visc = ((-visco * cbar * (h * dot_rr2) / ((rho1 + rho2) * T(0.5))) * m2).astype(T)
        ace_visc = acc3(-pi_visc * frx, -pi_visc * fry, -pi_visc * frz, fi & (dot < 0))
    else:
        temp = T(4) * visco / (re * (rho1 + rho2))
        vtemp = (m2 * temp * dot3).astype(T)
        ace_visc = acc3(vtemp * dvx, vtemp * dvy, vtemp * dvz, fi)
        t = np.zeros((n, 6), T) if tau is None else np.asarray(tau).astype(T)
        assert not t[:npb].any()
        ts = t[i] + np.where(fj[:, None], t[j], T(0))
        xx, xy, xz, yy, yz, zz = (ts[:, k] for k in range(6))
        ace_sps = acc3(m2 * (xx * frx + xy * fry + xz * frz), m2 * (xy * frx + yy * fry + yz * frz),
                       m2 * (xz * frx + yz * fry + zz * frz), fi)
        volp2 = -m2 / rho2
        ux, uy, uz = dvx * volp2, dvy * volp2, dvz * volp2
        # each of xy, xz, yz takes two terms per pair, in the reference's order
        g = [ux * frx, None, None, uy * fry, None, uz * frz]
        grad[:, 0], grad[:, 3], grad[:, 5] = acc(g[0], fi), acc(g[3], fi), acc(g[5], fi)
        if T is np.float32:
            for k, (a, b) in ((1, (ux * fry, uy * frx)), (2, (ux * frz, uz * frx)), (4, (uy * frz, uz * fry))):
                out = np.zeros(n, np.float32)
                idx = np.repeat(i[fi], 2)
                w = np.stack([a[fi], b[fi]], axis=1).astype(np.float32).ravel()
                np.add.at(out, idx, w)
                grad[:, k] = out
        else:
            grad[:, 1], grad[:, 2], grad[:, 4] = acc(ux * fry + uy * frx, fi), acc(ux * frz + uz * frx, fi), \
                acc(uy * frz + uz * fry, fi)
    # viscdt: the largest dot/(r^2+eta^2) of any interacting pair, and its conditioning
    viscdt = float(max(dot_rr2.max(), 0.0)) if len(dot_rr2) else 0.0
    sens = 0.0
    if viscdt > 0:
        top = dot_rr2 >= viscdt * (1.0 - 1e-5)
        sens = float(((np.abs(dvx) + np.abs(dvy) + np.abs(dvz)) / np.abs(dot) +
                      2.0 * (np.abs(drx) + np.abs(dry) + np.abs(drz)) / re)[top].max())
    # density diffusion (clouds.brute)
    delta = np.zeros(n, T)
    off = np.zeros(n, bool)
    kd = f("ddtkh") * cbar
    if ddt == 1:
        delta = acc((kd * (rho1 / rho2 - T(1)) / re * dot3 * m2).astype(T), fi & fj)
    elif ddt in (2, 3):
        rh = T(1) + f("ddtgz") * drz
        drhop = f("rhopzero") * np.power(rh, T(1) / f("gamma")) - f("rhopzero")
        delta = -acc((kd * ((rho2 - rho1) - drhop) / re * dot3 * m2 / rho2).astype(T), fi & fj)
    if ddt in (1, 2):
        off[i[fi & ~fj]] = True
    ar = (ar_cont + np.where(off, T(0), delta)).astype(T)
    # shifting (:743-750): the sums over every pair of a fluid p1; frozen per ShiftMode
    shift = np.zeros((n, 4), T)
    frozen = np.zeros(n, bool)
    if smode:
        mr = (m2 / rho2).astype(T)
        shift[:, 0], shift[:, 1], shift[:, 2] = acc(mr * frx, fi), acc(mr * fry, fi), acc(mr * frz, fi)
        shift[:, 3] = -acc(mr * dot3, fi)
        if smode == 1:
            frozen[i[fi & ~fj]] = True
        elif smode == 2:
            fixed = (codes(case).astype(np.int64) & 0x1800) == CODE_TYPE_FIXED
            frozen[i[fi & ~fj & fixed[j]]] = True
    ace = (ace_press + ace_visc + ace_sps).astype(T)
    out = dict(ar=ar, ace=ace, ace_press=ace_press, ace_visc=ace_visc, ace_sps=ace_sps, ar_cont=ar_cont, delta=delta,
               ddt_off=off, viscdt=viscdt, viscdt_sens=sens, grad=grad, shift=shift, frozen=frozen,
               amb_ddt=amb_b & (ddt in (1, 2)), amb_frozen=amb_b & (smode in (1, 2)), amb_any=amb_any, amb=amb_b)
    if tvisco == 2:
        out["tau"] = sps_tau(K, grad, rho, T)
        out["tau"][:npb] = 0
    return out


def e32(r64, r32, free=None):
    """Distance of the float32 evaluation from the float64 one: ar, ace, tau, shift (over the
    `free` particles) as max |d| / max |float64 array|, viscdt relative."""
    def rel(a, b):
        m = np.abs(a).max()
        return float(np.abs(b.astype(np.float64) - a).max() / m) if m > 0 else 0.0

    out = dict(ar=rel(r64["ar"], r32["ar"]), ace=rel(r64["ace"], r32["ace"]),
               viscdt=abs(r32["viscdt"] - r64["viscdt"]) / r64["viscdt"] if r64["viscdt"] > 0 else 0.0)
    if "tau" in r64:
        out["tau"] = rel(r64["tau"], r32["tau"])
    if free is not None:
        out["shift"] = rel(r64["shift"][free], r32["shift"][free])
    return out
