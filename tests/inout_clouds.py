"""Off-lattice clouds with one inlet/outlet zone, and the ghost-node extrapolation in numpy.

A helper beside ``clouds.py``: a seeded jittered block of 16 x 10 x 8 fluid particles (2-D twin:
16 x 1 x 8) with a density noise of 1 % and random velocities, and one zone of 4 layers behind
its +x face (320 inout particles; 32 in 2-D) whose velocity and density are extrapolated.

* ``make``    the cloud as a case with ``inout`` (the dict of XmlCase.inout, built by hand) for
              an extrapolate mode and a determlimit
* ``extrap``  Interaction_InOutExtrap (JSphCpu_InOut.cpp:55-237) restated in numpy for every
              initial inout particle: the sums over the fluid within 2h of its ghost node (the
              particle mirrored in the zone's plane), the determinant of the correction matrix,
              the first-order mirror back when |det| >= determlimit, else the zeroth-order
              values.  ``sums`` / ``matrix`` / ``kernel`` are the number formats of the pair
              sums, the matrix and the kernel values: all float64 is the reference of the tests,
              and the formats of a mode (1: float32, float32; 2: float32, float64; 3: float64,
              float64; the kernel always float32, FunSphKernel.h:226-234) give that mode's own
              rounding error

A helper module, not a conftest: nothing here changes how tests are collected.
"""
from __future__ import annotations

import numpy as np

from dualsphysics_multilayer_amd.case import PeriodicChannelCase
from dualsphysics_multilayer_amd.core import case_derive

DP = 0.02
NX, NY, NZ, LAYERS = 16, 10, 8, 4
JITTER = 0.15  # of dp: the fluid stays more than 0.8 dp from the inout particles
FLT_MAX = float(np.finfo(np.float32).max)
MODE_FORMATS = {1: (np.float32, np.float32), 2: (np.float32, np.float64), 3: (np.float64, np.float64)}


def make(two_d=False, mode=1, determlimit=1e-3, seed=7):
    ny = 1 if two_d else NY
    base = PeriodicChannelCase(DP, 2, 2, 2, 1, {}, data2d=two_d)
    rng = np.random.default_rng(seed + (100 if two_d else 0))
    k, j, i = np.meshgrid(np.arange(NZ), np.arange(ny), np.arange(NX), indexing="ij")
    fluid = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64) * DP
    jit = rng.uniform(-JITTER, JITTER, fluid.shape) * DP
    if two_d:
        jit[:, 1] = 0.0
    fluid += jit
    # a few boundary particles out of every support (the solver holds boundary particles first)
    bound = np.array([[-10 * DP, 0.0, -10 * DP], [-11 * DP, 0.0, -10 * DP]])
    c = base
    c.pos = np.ascontiguousarray(np.concatenate([bound, fluid]))
    c.npb, c.np = len(bound), len(c.pos)
    c.idp = np.arange(c.np, dtype=np.uint32)
    c.vel = np.zeros((c.np, 3), np.float32)
    c.vel[c.npb:] = rng.uniform(-1.0, 1.0, (len(fluid), 3)).astype(np.float32)
    if two_d:
        c.vel[:, 1] = 0.0
    c.rhop = (c.rhop0 * (1.0 + rng.uniform(-0.01, 0.01, c.np))).astype(np.float32)
    lo = np.array([-13 * DP, -3 * DP, -13 * DP])
    hi = np.array([(NX + LAYERS + 3) * DP, (ny + 3) * DP, (NZ + 4) * DP])
    c.map_limits = lambda: (lo, hi)
    # the zone: points one dp beyond the last fluid column, direction -x, the plane between them
    jj, kk = np.meshgrid(np.arange(ny), np.arange(NZ), indexing="xy")
    pts = np.stack([np.full(jj.size, NX * DP), jj.T.ravel() * DP, kk.T.ravel() * DP], axis=1)
    f32 = np.float32
    direction = np.array([-1.0, 0.0, 0.0])
    xpl = NX * DP - DP / 2
    zone = dict(id=0, layers=LAYERS, direction=direction, plane=np.array([-1, 0, 0, xpl], f32),
                width=float(f32(DP * LAYERS)), cfgzone=0x08 | 0x20 | 0x80, cfgupdate=0x02 | 0x10,
                veldata=np.zeros((2, 4), f32), zsurf=FLT_MAX,
                boxlimitmin=np.array([xpl, lo[1], lo[2]], f32), boxlimitmax=np.array([hi[0], hi[1], hi[2]], f32),
                points=pts, pointsinit=np.ones(len(pts), bool), nptinit=len(pts), npartinit=len(pts) * LAYERS)
    init_pos = np.concatenate([pts + direction * (-DP * layer) for layer in range(LAYERS)])
    c.inout = dict(zones=[zone], useboxlimit=True, extrapolatemode=mode, determlimit=float(f32(determlimit)),
                   codenewpart=0x1801, freelimitmin=lo.astype(f32), freelimitmax=hi.astype(f32), npresizeplus0=0,
                   init=dict(pos=init_pos, idp=np.arange(c.np, c.np + len(init_pos), dtype=np.uint32)))
    c.two_d = two_d
    return c


def extrap(case, sums=np.float64, matrix=np.float64, kernel=np.float64):
    """(vel [n][3], rhop [n], det [n], first [n]) of the initial inout particles: the extrapolated
    values, the determinant and whether the first-order branch was taken."""
    K = case_derive(case.case_def())
    S, M, KT = sums, matrix, kernel
    two_d = case.two_d
    zone = case.inout["zones"][0]
    pl = zone["plane"].astype(np.float64)
    dirf = zone["direction"].astype(np.float32).astype(np.float64)
    h, awen, bwen = KT(K["kernelh"]), KT(K["awen"]), KT(K["bwen"])
    mass = S(K["massfluid"])
    ks2 = S(np.float32(K["kernelsize2"]))
    fpos = case.pos[case.npb:]
    fvel = case.vel[case.npb:]
    frho = case.rhop[case.npb:]
    ppos = case.inout["init"]["pos"]
    n = len(ppos)
    nd = 3 if two_d else 4
    vel, rho, dets, first = np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros(n, bool)
    determlimit = float(case.inout["determlimit"])
    for p in range(n):
        p1 = ppos[p]
        displane = abs((pl[0] * p1[0] + pl[1] * p1[1] + pl[2] * p1[2] + pl[3]) / np.sqrt(pl[0] ** 2 + pl[1] ** 2 + pl[2] ** 2)) * 2
        node = p1 + displane * dirf
        dr = (node - fpos).astype(S)
        rr2 = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]
        sel = (rr2 <= ks2) & (rr2 >= S(1e-18))
        dr, r2 = dr[sel], rr2[sel]
        rad = np.sqrt(r2.astype(KT))
        qq = rad / h
        wqq1 = KT(1) - KT(0.5) * qq
        wqq2 = wqq1 * wqq1
        fac = (bwen * qq * wqq2 * wqq1 / rad).astype(S)
        wab = (awen * (qq + qq + KT(1)) * wqq2 * wqq2).astype(S)
        fr = fac[:, None] * dr
        v2 = fvel[sel].astype(S)
        vol = mass / frho[sel].astype(S)
        rhop = (mass * wab).sum(dtype=S)
        grho = (mass * fr).sum(axis=0, dtype=S)
        vwab, vfr = wab * vol, fr * vol[:, None]
        velp = (vwab[:, None] * v2).sum(axis=0, dtype=S)
        gvel = np.array([[(vfr[:, j] * v2[:, c]).sum(dtype=S) for j in range(3)] for c in range(3)], S)  # [comp][d/dx_j]
        ax = (0, 2) if two_d else (0, 1, 2)
        A = np.zeros((nd, nd), M)
        A[0, 0] = vwab.astype(M).sum(dtype=M)
        for cj, j in enumerate(ax):
            A[0, 1 + cj] = (dr[:, j] * vwab).astype(M).sum(dtype=M)
            A[1 + cj, 0] = vfr[:, j].astype(M).sum(dtype=M)
            for ck, k in enumerate(ax):
                A[1 + cj, 1 + ck] = (dr[:, k] * vfr[:, j]).astype(M).sum(dtype=M)
        det = np.linalg.det(A.astype(np.float64)) if M is np.float64 else _det(A)
        dets[p] = float(det)
        dpos = (p1 - node).astype(S)
        if abs(float(det)) >= determlimit:
            first[p] = True
            inv = np.linalg.inv(A.astype(np.float64)).astype(M)
            b = np.concatenate([[rhop], grho[list(ax)]]).astype(M)
            r = (inv @ b).astype(S)
            rho[p] = float(r[0] - (r[1:] * dpos[list(ax)]).sum(dtype=S))
            for c in ax:
                b = np.concatenate([[velp[c]], gvel[c][list(ax)]]).astype(M)
                r = (inv @ b).astype(S)
                vel[p, c] = float(r[0] - (r[1:] * dpos[list(ax)]).sum(dtype=S))
        elif A[0, 0] > 0:
            rho[p] = float(M(rhop) / A[0, 0])
            for c in ax:
                vel[p, c] = float(M(velp[c]) / A[0, 0])
    return vel, rho, dets, first


def _det(A):
    """The determinant in the matrix's own format (Laplace expansion, as the reference's)."""
    n = len(A)
    if n == 1:
        return A[0, 0]
    t = A.dtype.type(0)
    for j in range(n):
        minor = np.delete(np.delete(A, 0, axis=0), j, axis=1)
        t = t + A.dtype.type((-1) ** j) * A[0, j] * _det(minor)
    return t
