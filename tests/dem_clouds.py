"""An off-lattice cloud with floating bodies, and restatements of the two things RigidAlgorithm 0
and 2 add to Interaction_Forces:

* ``dem``      JSphCpu::InteractionForcesDEM (JSphCpu.cpp:828-925) per floating particle, over the
               solver's own cells in the reference's order (bound cells, then fluid cells; z, y, x
               ascending), in float64 or in float32 with the reference's operation order;
* ``brute_ft`` the pair sums of InteractionForcesFluid / -Bound (DDT none) over all pairs in float64
               or float32, with the floating particles' masses and the `compute` rule of FTMODE_Ext
               (JSphCpu.cpp:594,705) or of FTMODE_Sph.

The cloud: a fixed slab, a moving block, three floating blobs of different materials that reach into
each other and into both boundary blocks, fluid in between, and a few placed particles that give the
cases a random cloud may miss (``facts`` lists and counts them).  A helper module, not a conftest.
"""
from __future__ import annotations

import copy

import numpy as np

import clouds
from dualsphysics_multilayer_amd.case import DamBreakCase

FIXED, MOVING, FLOATING, FLUID = 0x0, 0x800, 0x1000, 0x1800
DP = clouds.DP
# material per block code: (Young_Modulus, PoissonRatio, Kfric, Restitution_Coefficient)
MATERIAL = {FIXED: (2.1e9, 0.30, 0.45, 0.70), MOVING: (6.9e8, 0.30, 0.15, 0.60),
            FLOATING | 0: (3.0e8, 0.35, 0.40, 0.80), FLOATING | 1: (1.1e9, 0.25, 0.25, 0.55),
            FLOATING | 2: (5.0e8, 0.40, 0.60, 0.65)}
RHO_BODY = (500.0, 800.0, 1200.0)


def make(ftmode_rigid=2, cellmode=1, seed=31):
    """The cloud as a case with RigidAlgorithm `ftmode_rigid` (0, 1 or 2)."""
    rng = np.random.default_rng(seed)
    cs = clouds._cell(1.0, DP)
    nc = np.array([6.0, 4.0, 4.0])
    eps = 1e-3
    per_cell = (cs / DP) ** 3

    def box(n, a, b):
        return rng.uniform(np.asarray(a, float), np.asarray(b, float), (int(n), 3)) * cs

    fixed = box(0.5 * per_cell * 6 * 4 * 0.7, [eps, eps, eps], [6 - eps, 4 - eps, 0.7])
    moving = box(0.5 * per_cell * 0.6 * 4 * 2, [eps, eps, 0.7], [0.6, 4 - eps, 2.7])
    # blob 0 rests on the fixed slab and touches the moving block, blob 1 overlaps blob 0's top and
    # the slab, blob 2 is clear of the boundary and touches blob 1; all denser than the lattice
    blobs = [box(260, [0.5, 1.0, 0.62], [2.0, 2.6, 1.5]), box(240, [1.9, 1.2, 0.64], [3.2, 2.8, 1.7]),
             box(200, [3.1, 1.5, 1.5], [4.2, 2.6, 2.6])]
    # placed particles (cell units), appended to blob 2 / fixed:
    #  A, B: a contact along x only with velocities along x only (zero tangential velocity)
    #  C, D: a candidate pair with equal velocities (vn = 0)
    #  E:    a fast particle 1.4 Dp above a fixed one F and in contact with nothing
    #  G:    a particle of blob 2 with only its own block around it (H next to it)
    d = DP / cs
    A = np.array([3.6, 0.5, 3.0])
    E = np.array([2.5, 3.5, 1.0 + 1.4 * d])
    placed_f2 = np.array([A, [5.3, 3.2, 3.3], [5.3 + 0.3 * d, 3.2, 3.3 + 0.5 * d], E,
                          [5.5, 1.6, 2.2], [5.5 + 0.8 * d, 1.6, 2.2]])
    placed_fixed = np.array([A + [0.6 * d, 0, 0], [2.5, 3.5, 1.0]])
    placed_f1 = np.array([[5.3, 3.2 + 1.2 * d, 3.3]])  # D: candidate of C, 1.2 Dp away, in blob 1
    blobs[2] = np.concatenate([blobs[2], placed_f2 * cs])
    blobs[1] = np.concatenate([blobs[1], placed_f1 * cs])
    fixed = np.concatenate([fixed, placed_fixed * cs])
    fluid = box(0.5 * per_cell * 6 * 4 * 3, [eps, eps, 0.7], [6 - eps, 4 - eps, 4 - eps])
    # no fluid within the support radius of E: its speed stays out of the SPH viscosity dt
    fluid = fluid[np.sqrt(((fluid - E * cs) ** 2).sum(axis=1)) > 1.1 * cs]
    base = DamBreakCase(DP, tdensity=0, cellmode=cellmode, celldomfixed=True)
    bound = np.concatenate([fixed, moving])
    rest = np.concatenate(blobs + [fluid])
    c = clouds.cloud_case(base, bound, rest, seed + 1, np.zeros(3), nc * cs, vamp=0.05)
    nfx, nmv = len(fixed), len(moving)
    nb = [len(b) for b in blobs]
    code = np.full(c.np, FLUID, np.uint16)
    code[:nfx] = FIXED
    code[nfx:c.npb] = MOVING
    c.vel[nfx:c.npb] = rng.uniform(-0.5, 0.5, (nmv, 3)).astype(np.float32)
    o = c.npb
    nft = sum(nb)
    c.vel[o:o + nft] = rng.uniform(-1.0, 1.0, (nft, 3)).astype(np.float32)
    c.floatings = []
    for k, n in enumerate(nb):
        code[o:o + n] = FLOATING | k
        massp = RHO_BODY[k] * DP ** 3
        c.floatings.append(dict(idbegin=o, count=n, massbody=massp * n, masspart=massp,
                                center=tuple(c.pos[o:o + n].mean(axis=0)), inertia=(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                linvelini=(0, 0, 0), angvelini=(0, 0, 0), translationfree=(1, 1, 1),
                                rotationfree=(1, 1, 1), mkbound=2 + k))
        o += n
    # the placed particles' velocities
    i2 = c.npb + nb[0] + nb[1] + nb[2] - len(placed_f2)  # A, C, (helper), E, G, H
    iD = c.npb + nb[0] + nb[1] - 1
    iB, iF = nfx - 2, nfx - 1
    c.vel[i2] = (-0.7, 0, 0)      # A moves along x towards B (at rest)
    c.vel[i2 + 1] = c.vel[iD] = (0.3, -0.2, 0.1)  # C, D: dv = 0
    c.vel[i2 + 2] = c.vel[i2 + 1]
    c.vel[i2 + 3] = (0, 0, -60.0)  # E falls fast on F, 1.4 Dp below: a candidate, no contact
    c.placed = dict(A=i2, B=iB, C=i2 + 1, D=iD, E=i2 + 3, F=iF, G=i2 + 4, H=i2 + 5)
    c._code = code
    c.has_bodies = True
    c.explicit_codes = True
    c.ftpause = 0.0
    c.rigidalgorithm = ftmode_rigid
    c.ftmode = 1 if ftmode_rigid == 1 else 2
    c.use_dem = ftmode_rigid == 2
    c.demdtforce0 = 0.0
    f32 = np.float32
    c.demdata = []
    for tav, (young, poisson, kfric, restitu) in MATERIAL.items():
        k = tav & 0x7ff
        isft = (tav & 0x1800) == FLOATING
        c.demdata.append(dict(code=tav, mass=float(f32(c.floatings[k]["massbody"])) if isft else 0.0,
                              massp=float(f32(c.floatings[k]["masspart"] if isft else base.case_def()["massbound"])),
                              tau=float((f32(1) - f32(poisson) * f32(poisson)) / f32(young)), kfric=float(f32(kfric)),
                              restitu=float(f32(restitu))))
    c._cloud_key = ("ftcloud", seed, cellmode)
    return as_case(c)


# DamBreakCase.code is a property of the class: the cloud carries its own codes
class _Case(DamBreakCase):
    @property
    def code(self):
        return self._code


def as_case(c):
    """`c` as an instance whose `code` is the cloud's (SphGpuSingle reads case.code)."""
    out = copy.copy(c)
    out.__class__ = _Case
    return out


# ----------------------------------------------------------------------------------------
def cells_of(case, K):
    scell = float(np.float32(K["scell"]))
    cc = np.floor((case.pos - np.asarray(K["map_realposmin"])) / scell).astype(np.int64)
    return cc, np.asarray(K["dom_cells"], np.int64)


def candidates(case, K):
    """Per floating particle p1 (case index): its candidates p2 (not fluid, another block) as
    (indices in the reference's order, from_bound_cells flags)."""
    code = case._code.astype(np.int64)
    tav = code & 0x1fff
    cc, nc = cells_of(case, K)
    div = int(K["scelldiv"])
    key = (cc[:, 2] * nc[1] + cc[:, 1]) * nc[0] + cc[:, 0]
    nonfluid = np.flatnonzero((code & 0x1800) != FLUID)
    out = {}
    for p1 in np.flatnonzero((code & 0x1800) == FLOATING):
        d = np.abs(cc[nonfluid] - cc[p1]).max(axis=1)
        sel = nonfluid[(d <= div) & (tav[nonfluid] != tav[p1])]
        isbound = sel < case.npb
        # bound cells first, then fluid cells; cells z, y, x ascending; the case order inside a cell
        order = np.lexsort((sel, key[sel], ~isbound))
        out[int(p1)] = (sel[order], isbound[order])
    return out


def dem(case, K, dtforce, dtype=np.float64):
    """(dace [np][3], demdt, ncontact [np], demvisc_max [np]) of InteractionForcesDEM."""
    T = dtype
    dem = {d["code"]: d for d in case.demdata}
    tav = case._code.astype(np.int64) & 0x1fff
    dp = T(np.float32(K["dp"]))
    pos, vel = case.pos, case.vel.astype(T)
    dace = np.zeros((case.np, 3), T)
    ncont = np.zeros(case.np, np.int64)
    visc = np.zeros(case.np, T)
    demdt = T(0)
    pi = T(np.float32(np.pi))
    for p1, (cand, isb) in candidates(case, K).items():
        if not len(cand):
            continue
        d1 = dem[int(tav[p1])]
        m1, t1, k1, r1, mp1 = (T(np.float32(d1[k])) for k in ("mass", "tau", "kfric", "restitu", "massp"))
        ace = np.zeros(3, T)
        vmax = T(0)
        for p2, bnd in zip(cand, isb):
            d2 = dem[int(tav[p2])]
            m2, t2, k2, r2 = (T(np.float32(d2[k])) for k in ("mass", "tau", "kfric", "restitu"))
            dr = (pos[p1] - pos[p2]).astype(np.float32).astype(T)  # float(posp1.x-pos[p2].x)
            rr2 = dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2]
            rad = np.sqrt(rr2)
            nu = m1 / T(2) if bnd else m1 * m2 / (m1 + m2)
            kn = T(4) / (T(3) * (t1 + t2)) * np.sqrt(dp / T(4))
            dv = vel[p1] - vel[p2]
            n = dr / rad
            vn = dv[0] * n[0] + dv[1] * n[1] + dv[2] * n[2]
            with np.errstate(divide="ignore"):
                dv_ = T(0.2) / (T(3.21) * (np.power(nu / kn, T(0.4)) * np.power(np.abs(vn), T(-0.2))) / T(40))
            vmax = max(vmax, dv_)
            over = T(1) * dp - rad
            if over > 0:
                ncont[p1] += 1
                eij = (r1 + r2) / T(2)
                le = np.log(eij)
                gn = -(T(2) * le * np.sqrt(nu * kn)) / np.sqrt(pi + le * le)
                rep = kn * np.power(over, T(1.5))
                fn = rep - gn * np.power(over, T(0.25)) * vn
                acef = fn / mp1
                ace = ace + acef * n
                dvt = dv - vn * n
                vt = np.sqrt(dvt[0] * dvt[0] + dvt[1] * dvt[1] + dvt[2] * dvt[2])
                t = dvt / vt if vt != 0 else np.zeros(3, T)
                ft_elast = T(2) * (kn * T(np.float32(dtforce)) - gn) * vt / T(7)
                kf = (k1 + k2) / T(2)
                ft = kf * fn * np.tanh(T(8) * vt)
                ft = ft if ft < ft_elast else ft_elast
                ace = ace + (ft / mp1) * t
        visc[p1] = vmax
        if ace.any():
            dace[p1] = ace
            demdt = max(demdt, vmax)
    return dace, demdt, ncont, visc


def facts(case, K, K_other):
    """What the cloud holds, counted from the cloud itself (K, K_other: the derived constants with
    full and half cells)."""
    cand = candidates(case, K)
    cand2 = candidates(case, K_other)
    dace, demdt, ncont, visc = dem(case, K, 1e-4)
    code = case._code.astype(np.int64)
    tav = code & 0x1fff
    dp = float(np.float32(K["dp"]))
    both = two = own = differ = 0
    for p1, (c, isb) in cand.items():
        dr = (case.pos[p1] - case.pos[c]).astype(np.float32).astype(np.float64)
        touch = np.sqrt((dr * dr).sum(axis=1)) < dp
        both += bool((touch & isb).any() and (touch & ~isb).any())
        two += len(set(tav[c[touch]])) >= 2
        own += len(c) == 0
        differ += bool(ncont[p1] and set(c) != set(cand2[p1][0]))
    contact = ncont > 0
    P = case.placed
    quiet = (ncont == 0) & (visc > 0)
    return dict(both=both, two_blocks=two, own_block_only=own, candidates_differ=differ,
                contacts=int(ncont.sum()), contacting=int(contact.sum()),
                visc_quiet_max=float(visc[quiet].max()) if quiet.any() else 0.0,
                visc_contact_max=float(visc[contact].max()), demdt=float(demdt), placed=P, ncont=ncont, visc=visc)


# ----------------------------------------------------------------------------------------
def brute_ft(case, K, ext, dtype=np.float64):
    """ar, ace (DDT none, Wendland, artificial viscosity) over all pairs with the floating particles'
    masses; ext: the `compute` rule of FTMODE_Ext.  float32: every pair term in float32, summed
    sequentially in float32 in the order of clouds.pairs (p1 major, p2 ascending)."""
    T = dtype
    f = lambda k: T(np.float32(K[k]))  # noqa: E731
    P = clouds.pairs(case, K)
    n, npb = case.np, case.npb
    use = P["real"]
    i, j = P["i"][use], P["j"][use]
    code = case._code.astype(np.int64)
    ft = (code & 0x1800) == FLOATING
    bi, bj = i < npb, j < npb
    keep = ~(bi & bj)
    skipped = (bi & ft[j]) | (ft[i] & (bj | ft[j]))
    if ext:
        keep &= ~skipped
    nskipped = int((skipped & ~(bi & bj)).sum())
    i, j, bi, bj = i[keep], j[keep], bi[keep], bj[keep]
    dr = (case.pos[i] - case.pos[j]).astype(np.float32).astype(T)
    rr2 = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]
    rad = np.sqrt(rr2)
    h = f("kernelh")
    q = rad / h
    w1 = T(1) - T(0.5) * q
    fac = f("bwen") * q * w1 * w1 * w1 / rad
    massp = np.zeros(n, T)
    massp[:npb] = f("massbound")
    massp[npb:] = f("massfluid")
    for k, b in enumerate(case.floatings):
        massp[code == (FLOATING | k)] = T(np.float32(b["masspart"]))
    m2 = np.where(bi, np.where(ft[j], massp[j], f("massfluid")), massp[j]).astype(T)
    m2 = np.where(~bi & bj, f("massbound"), m2).astype(T)
    vel, rho = case.vel.astype(T), case.rhop.astype(T)
    press = clouds.pressure(case, K).astype(T)
    dv = vel[i] - vel[j]
    fr = fac[:, None] * dr
    ar_t = m2 * (dv[:, 0] * fr[:, 0] + dv[:, 1] * fr[:, 1] + dv[:, 2] * fr[:, 2]) * (rho[i] / rho[j])
    prs = (press[i] + press[j]) / (rho[i] * rho[j])
    p_vpm = -prs * m2
    dot = dr[:, 0] * dv[:, 0] + dr[:, 1] * dv[:, 1] + dr[:, 2] * dv[:, 2]
    dot_rr2 = dot / (rr2 + f("eta2"))
    visco = np.where(bj, T(np.float32(K["visco"]) * np.float32(K["viscoboundfactor"])), f("visco")).astype(T)
    pi_visc = np.where(dot < 0, (-visco * T(np.float32(K["cs0"])) * (h * dot_rr2) / ((rho[i] + rho[j]) * T(0.5))) * m2,
                       T(0)).astype(T)
    ace_t = np.where(bi[:, None], T(0), (p_vpm - pi_visc)[:, None] * fr).astype(T)
    ar = np.zeros(n, T)
    ace = np.zeros((n, 3), T)
    np.add.at(ar, i, ar_t.astype(T))
    np.add.at(ace, i, ace_t)
    visc_t = np.where(~bi | ~bj, dot_rr2, T(0))
    return dict(ar=ar, ace=ace, nskipped=nskipped, viscdt=float(max(visc_t.max(), 0)))


def make_acemax(cellmode=1, seed=47):
    """A small cloud for AceMax: the floating particle P holds the pair-sum maximum of |ace| (it is compressed,
    with one fluid particle Q 0.7 Dp away and no other within 1.6 Dp) and a fixed particle B touches P from the side its acceleration
    points to, with the overlap at which the Hertz force equals that acceleration: the contact lowers
    |ace| of P, and the maximum over the final accelerations is below the pair sums' maximum.  Returns
    (case, index of P, its float64 pair-sum acceleration)."""
    rng = np.random.default_rng(seed)
    cs = clouds._cell(1.0, DP)
    nc = np.array([6.0, 4.0, 4.0])
    eps = 1e-3

    def box(n, a, b):
        return rng.uniform(np.asarray(a, float), np.asarray(b, float), (int(n), 3)) * cs

    P = np.array([2.5, 2.0, 2.0]) * cs
    Q = P + np.array([0.45, -0.35, 0.4]) * DP  # 0.7 Dp: where the kernel gradient is largest
    fixed0 = box(80, [eps, eps, eps], [6 - eps, 4 - eps, 0.7])
    body = np.concatenate([box(5, [4.2, 1.0, 2.6], [5.0, 3.0, 3.4]), P[None]])
    fluid = box(700, [eps, eps, 0.7], [6 - eps, 4 - eps, 4 - eps])
    # thinned: no other pair of particles closer than 0.4 Dp, so that P's pair is the closest by far
    dd = np.sqrt(((fluid[:, None, :] - fluid[None, :, :]) ** 2).sum(axis=2)) + np.triu(np.full((len(fluid),) * 2, 1e9))
    fluid = fluid[dd.min(axis=1) > 0.4 * DP]
    for other in (body[:-1], fixed0):
        fluid = fluid[np.sqrt(((fluid[:, None, :] - other[None, :, :]) ** 2).sum(axis=2)).min(axis=1) > 0.4 * DP]
    fluid = np.concatenate([fluid[np.sqrt(((fluid - P) ** 2).sum(axis=1)) > 1.6 * DP], Q[None]])
    base = DamBreakCase(DP, tdensity=0, cellmode=cellmode, celldomfixed=True)

    def build(fixed):
        c = clouds.cloud_case(base, fixed, np.concatenate([body, fluid]), seed + 1, np.zeros(3), nc * cs, vamp=0.05,
                              rhoamp=0.002)
        # P compressed: the pressure term of its pair with Q (the last particle) dominates every other sum
        c.rhop[c.npb + len(body) - 1] = np.float32(1.25 * base.rhop0)
        code = np.full(c.np, FLUID, np.uint16)
        code[: c.npb] = FIXED
        code[c.npb:c.npb + len(body)] = FLOATING
        c.vel[c.npb:c.npb + len(body)] = 0
        massp = RHO_BODY[0] * DP ** 3
        c.floatings = [dict(idbegin=c.npb, count=len(body), massbody=massp * len(body), masspart=massp,
                            center=tuple(body.mean(axis=0)), inertia=(1, 0, 0, 0, 1, 0, 0, 0, 1), linvelini=(0, 0, 0),
                            angvelini=(0, 0, 0), translationfree=(1, 1, 1), rotationfree=(1, 1, 1), mkbound=1)]
        c._code = code
        c.has_bodies = c.explicit_codes = True
        c.ftpause, c.rigidalgorithm, c.ftmode, c.use_dem, c.demdtforce0 = 0.0, 2, 2, True, 0.0
        f32 = np.float32
        c.demdata = []
        for tav in (FIXED, FLOATING):
            young, poisson, kfric, restitu = MATERIAL[tav]
            isft = tav == FLOATING
            c.demdata.append(dict(code=tav, mass=float(f32(massp * len(body))) if isft else 0.0,
                                  massp=float(f32(massp if isft else base.case_def()["massbound"])),
                                  tau=float((f32(1) - f32(poisson) * f32(poisson)) / f32(young)),
                                  kfric=float(f32(kfric)), restitu=float(f32(restitu))))
        c._cloud_key = ("acemax", seed, cellmode, len(fixed))
        return as_case(c)

    from dualsphysics_multilayer_amd.core import case_derive

    c0 = build(fixed0)
    K = case_derive(c0.case_def())
    ip = c0.npb + len(body) - 1
    a_p = brute_ft(c0, K, True)["ace"][ip]
    mag = float(np.sqrt((a_p * a_p).sum()))
    d = {x["code"]: x for x in c0.demdata}
    kn = 4.0 / (3.0 * (d[FIXED]["tau"] + d[FLOATING]["tau"])) * np.sqrt(DP / 4.0)
    over = (mag * d[FLOATING]["massp"] / kn) ** (2.0 / 3.0)
    assert 0 < over < 0.5 * DP
    B = P + a_p / mag * (DP - over)  # the contact pushes P along (P - B), against a_p
    c = build(np.concatenate([fixed0, B[None]]))
    # the same velocities and densities as without B (B at rest, at the reference density)
    n0 = c0.npb
    c.vel = np.ascontiguousarray(np.concatenate([c0.vel[:n0], np.zeros((1, 3), np.float32), c0.vel[n0:]]))
    c.rhop = np.ascontiguousarray(np.concatenate([c0.rhop[:n0], np.float32([base.rhop0]), c0.rhop[n0:]]))
    return c, ip + 1, a_p
