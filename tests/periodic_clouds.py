"""Off-lattice clouds in a periodic box, and their explicit-image extension in numpy.

A helper beside ``clouds.py`` (imported, never edited): seeded random particle sets in a box
that is periodic in X, in X and Y with a Y offset on the X period, and in all three axes.

* ``make``         the named periodic cloud as a case (``peri_active`` and the offsets set;
                   the map limits are the REAL map, the period)
* ``run_periodic`` JSphCpuSingle::RunPeriodic restated in numpy: the duplicates of a particle
                   set in the reference's order (type, axis, block of new duplicates before the
                   originals, ascending index, +inc before -inc)
* ``extended``     the cloud with its duplicates as ORDINARY particles of a case without
                   periodic boundaries whose map is Map_PosMin/Max: boundary originals, boundary
                   duplicates, fluid originals, fluid duplicates.  A solver that knows nothing of
                   periodicity computes on it what the periodic solver must compute for the
                   originals, and ``clouds.brute`` on it is the float64 reference.
* ``image_counts`` neighbours of every original by the minimum-image rule (all 27 combinations
                   of the three periods), independent of the duplicate lists

A helper module, not a conftest: nothing here changes how tests are collected.
"""
from __future__ import annotations

import copy
import functools

import numpy as np

import clouds

NAMES = ("x", "xy", "xyz")
# periodic axes (PeriActive bits) and the box in cells of 2h: no multiple of a cell, more than
# two cells (a particle never sees its own image), several blocks of 256 particles
_SPEC = {
    "x": dict(active=1, nc=(5.3, 4.4, 4.0), bound=True),
    "xy": dict(active=3, nc=(5.3, 4.6, 4.0), bound=True),
    "xyz": dict(active=7, nc=(4.3, 3.6, 3.7), bound=False),
}
# seeds for which clouds.brute leaves no pair inside its SHELL on the extended cloud
# (tests/test_periodic.py asserts it)
SEEDS = {"x": 31, "xy": 32, "xyz": 33}
OFFSET_DP = 3.0  # XPeriodicIncY of the xy cloud, in dp


@functools.lru_cache(maxsize=None)
def _points(name, seed, coefh, dp):
    spec = _SPEC[name]
    rng = np.random.default_rng(seed)
    cs = clouds._cell(coefh, dp)
    per_cell = (cs / dp) ** 3
    nc = np.array(spec["nc"], np.float64)
    eps = 1e-3
    zs = nc[2] / 5.0

    def poisson(dens, a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return clouds._box(rng, rng.poisson(dens * per_cell * np.prod(b - a)), a, b)

    # periodic axes are filled from face to face (the period is the map), the others keep a margin
    lo_p = np.where([(spec["active"] >> i) & 1 for i in range(3)], 0.0, eps)
    hi_p = np.where([(spec["active"] >> i) & 1 for i in range(3)], nc, nc - eps)
    if spec["bound"]:
        fluid = poisson(0.4, [lo_p[0], lo_p[1], zs], hi_p)
        bound = poisson(0.3, lo_p, [hi_p[0], hi_p[1], zs])
    else:
        fluid = poisson(0.4, lo_p, hi_p)
        bound = poisson(0.3, [1.0, 1.0, 1.0], [1.8, 1.8, 1.8])
    lo, hi = np.zeros(3), nc * cs
    bound, fluid = bound * cs, fluid * cs
    # strictly inside the real map (cloud_case asserts it), faces included up to one ulp
    for a in (bound, fluid):
        np.clip(a, np.nextafter(lo, hi), np.nextafter(hi, lo), out=a)
        a.setflags(write=False)
    return bound, fluid, lo, hi


def make(name, seed=None, dp=clouds.DP, vamp=1.0, rhoamp=0.02, shift=None, **kw):
    """The named periodic cloud; kw are DamBreakCase constants.  shift: a vector added to every
    position, wrapped back into the box by the periods (the same physical system)."""
    seed = SEEDS[name] if seed is None else seed
    coefh = float(kw.get("coefh", 1.0))
    bound, fluid, lo, hi = _points(name, seed, coefh, dp)
    kw.setdefault("celldomfixed", True)
    base = clouds._base(dp, False, tuple(sorted(kw.items())))
    c = clouds.cloud_case(base, bound, fluid, seed + 1000, lo, hi, vamp=vamp, rhoamp=rhoamp)
    spec = _SPEC[name]
    c.peri_active = spec["active"]
    c.peri_xinc = (0.0, OFFSET_DP * dp if name == "xy" else 0.0, 0.0)
    c.peri_yinc = (0.0, 0.0, 0.0)
    c.peri_zinc = (0.0, 0.0, 0.0)
    c._cloud_key = ("peri", name, seed, coefh, dp, None if shift is None else tuple(shift))
    if shift is not None:
        c.pos = wrap(c.pos + np.asarray(shift, np.float64), lo, hi, periods(c))
    return c


def periods(case):
    """Peri?inc with the own-axis component derived (-MapRealSize, JSph.cpp:2067-2069); rows of
    axes that are not periodic are None."""
    lo, hi = case.map_limits()
    out = []
    for ax, inc in enumerate((case.peri_xinc, case.peri_yinc, case.peri_zinc)):
        if not (case.peri_active >> ax) & 1:
            out.append(None)
            continue
        v = np.array(inc, np.float64)
        v[ax] = -(hi[ax] - lo[ax])
        out.append(v)
    return out


def wrap(pos, lo, hi, incs):
    """JSphCpu::UpdatePos's wrap (JSphCpu.cpp:1254-1271) of positions outside the real map."""
    pos = np.array(pos, np.float64)
    d = pos - lo
    size = hi - lo
    for ax in range(3):
        if incs[ax] is None:
            continue
        low, high = d[:, ax] < 0, d[:, ax] >= size[ax]
        d[low] -= incs[ax]
        d[high] += incs[ax]
    return d + lo


def map_pos(case, K):
    """Map_PosMin / Map_PosMax: the real map widened by KernelSize on each periodic axis."""
    lo, hi = (np.array(v, np.float64) for v in case.map_limits())
    ks = float(np.float32(K["kernelsize"]))
    for ax in range(3):
        if (case.peri_active >> ax) & 1:
            lo[ax] -= ks
            hi[ax] += ks
    return lo, hi


def run_periodic(pos, npb, incs, mapmin, mapmax):
    """The duplicates RunPeriodic makes of `pos` (boundary = the first npb): per type (bound,
    fluid) the arrays (src index into pos, displaced position, axes crossed) in creation order."""
    out = []
    n = len(pos)
    for lo_i, hi_i in ((0, npb), (npb, n)):
        src = np.zeros(0, np.int64)
        dpos = np.zeros((0, 3))
        nax = np.zeros(0, np.int64)
        o_src, o_pos = np.arange(lo_i, hi_i, dtype=np.int64), pos[lo_i:hi_i]
        for ax in range(3):
            if incs[ax] is None:
                continue
            c_src = np.concatenate([src, o_src])          # block 0: the new duplicates, block 1: the originals
            c_pos = np.concatenate([dpos, o_pos])
            c_nax = np.concatenate([nax, np.zeros(len(o_src), np.int64)])
            both = np.stack([c_pos + incs[ax], c_pos - incs[ax]], axis=1)  # +inc before -inc
            ok = ((mapmin <= both) & (both < mapmax)).all(axis=2)
            src = np.concatenate([src, np.repeat(c_src, 2)[ok.ravel()]])
            dpos = np.concatenate([dpos, both.reshape(-1, 3)[ok.ravel()]])
            nax = np.concatenate([nax, np.repeat(c_nax + 1, 2)[ok.ravel()]])
        out.append((src, dpos, nax))
    return out


_EXT = {}


def extended(case, K):
    """(ext_case, orig, info): the explicit-image cloud as a case WITHOUT periodic boundaries over
    Map_PosMin/Max; orig = the indices (= idp) of the original particles in it, in the order of
    `case`; info = duplicate counts (bound, fluid, per face, corner images)."""
    key = getattr(case, "_cloud_key", None)
    mapmin, mapmax = map_pos(case, K)
    incs = periods(case)
    # (the duplicate lists depend on the positions and h alone and are cached; the case around
    # them carries this case's other constants: cell mode, DDT, kernel)
    if key is None or key not in _EXT:
        dup = run_periodic(case.pos, case.npb, incs, mapmin, mapmax)
        if key is not None:
            _EXT[key] = dup
    else:
        dup = _EXT[key]
    (bs, bp, bn), (fs, fp, fn) = dup
    src = np.concatenate([np.arange(case.npb), bs, np.arange(case.npb, case.np), fs])
    e = copy.copy(case)
    e.pos = np.ascontiguousarray(np.concatenate([case.pos[:case.npb], bp, case.pos[case.npb:], fp]))
    e.vel = np.ascontiguousarray(case.vel[src])
    e.rhop = np.ascontiguousarray(case.rhop[src])
    e.npb, e.np = case.npb + len(bs), len(src)
    e.idp = np.arange(e.np, dtype=np.uint32)
    e._map = (mapmin, mapmax)
    e.peri_active = 0
    e.peri_xinc = e.peri_yinc = e.peri_zinc = (0.0, 0.0, 0.0)
    e._cloud_key = None if key is None else ("ext",) + key
    orig = np.concatenate([np.arange(case.npb), np.arange(e.npb, e.npb + case.np - case.npb)])
    lo, hi = case.map_limits()
    alld = np.concatenate([bp, fp])
    faces = {}
    for ax in range(3):
        if incs[ax] is not None:
            faces[ax] = (int((alld[:, ax] < lo[ax]).sum()), int((alld[:, ax] >= hi[ax]).sum()))
    info = dict(nbound=len(bs), nfluid=len(fs), faces=faces, corner=int((np.concatenate([bn, fn]) >= 2).sum()),
                src=src)
    return e, orig, info


def image_counts(case, K):
    """Real pairs [fluid-fluid, fluid-bound, bound-fluid] of the periodic cloud by the minimum-image
    rule: p1 an original, p2 any original displaced by k xinc + l yinc + m zinc, k, l, m in
    {-1, 0, 1} (a period is longer than 2 KernelSize: no further image can be a neighbour)."""
    ks2 = float(np.float32(K["kernelsize2"]))
    incs = periods(case)
    rng = [(-1, 0, 1) if v is not None else (0,) for v in incs]
    pos, npb = case.pos, case.npb
    fl = np.arange(case.np) >= npb
    counts = np.zeros(3, np.int64)
    for k in rng[0]:
        for l in rng[1]:
            for m in rng[2]:
                sh = sum(c * v for c, v in zip((k, l, m), incs) if v is not None)
                sh = np.zeros(3) if isinstance(sh, int) else sh
                d = pos[:, None, :] - (pos[None, :, :] + sh)
                r2 = np.einsum("ijk,ijk->ij", d, d)
                real = (r2 <= ks2) & (r2 >= clouds.ALMOSTZERO)
                counts[0] += (real & fl[:, None] & fl[None, :]).sum()
                counts[1] += (real & fl[:, None] & ~fl[None, :]).sum()
                counts[2] += (real & ~fl[:, None] & fl[None, :]).sum()
    return counts
