"""Clouds for the candidate rounds and test groups of the tiled interaction (CellMode=full),
built on tests/clouds.py.

The tiled kernel tests a lane's 3-cell window in groups of 32 records, the last group only
as far as the longest window of the wave reaches (in blocks of 8), and drains rounds of 128
candidates per window.  Which path a window takes depends on its length alone, so the
clouds here are chosen for their window lengths:

* ``even``   a uniform random cloud at the lattice density: windows around 125, on both
             sides of 128 within one wave;
* ``patch``  the same with a patch at 1.6 times that density (windows around 200) and, inside
             the patch, a core of one cell at ten times the density: the only way to windows
             beyond 384 (three rounds) and to neighbour rows longer than one TCAP segment,
             which a density of 1.6 (67 per cell, 400 in the 6 staged cells) never reaches.

``windows`` lists, per fluid item and drain unit, what each lane's windows are, following
the item build (csrc/sph_items.hpp), lane_order (csrc/sph_tiled.hpp) and run_pass
(csrc/sph_interaction_tiled.hpp).

A helper module, not a conftest: nothing here changes how tests are collected.
"""
from __future__ import annotations

import functools

import numpy as np

import clouds

TB, TCAP, TMAXCELLS = clouds.TB, clouds.TCAP, 4
NAMES = ("even", "patch")
SEEDS = {"even": 21, "patch": 22}
NC = (10, 4, 4)  # cells of 2h


@functools.lru_cache(maxsize=None)
def _points(name, seed, coefh, dp):
    rng = np.random.default_rng(seed)
    cs = clouds._cell(coefh, dp)
    per_cell = (cs / dp) ** 3
    nc = np.array(NC, np.float64)
    eps = 1e-3
    ext = nc - eps
    zs = nc[2] / 5.0

    def poisson(dens, a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return clouds._box(rng, rng.poisson(dens * per_cell * np.prod(b - a)), a, b)

    e0 = np.full(3, eps)
    fluid = [poisson(1.0, [eps, eps, zs], ext)]
    bound = [poisson(0.15, e0, [ext[0], ext[1], zs])]
    if name == "patch":
        fluid.append(poisson(0.6, [3.0, 1.0, 1.5], [7.0, 3.0, 3.5]))
        fluid.append(poisson(9.0, [5.0, 2.0, 2.0], [6.0, 3.0, 3.0]))
    lo, hi = np.zeros(3), nc * cs
    bound_pos = np.concatenate(bound) * cs
    fluid_pos = np.concatenate(fluid) * cs
    for a in (bound_pos, fluid_pos, lo, hi):
        a.setflags(write=False)
    return bound_pos, fluid_pos, lo, hi


def make(name, seed=None, dp=clouds.DP, **kw):
    """The named cloud as a case; kw are DamBreakCase constants (tdensity, cellmode, ...)."""
    seed = SEEDS[name] if seed is None else seed
    coefh = float(kw.get("coefh", 1.0))
    bound_pos, fluid_pos, lo, hi = _points(name, seed, coefh, dp)
    kw.setdefault("celldomfixed", True)
    base = clouds._base(dp, False, tuple(sorted(kw.items())))
    c = clouds.cloud_case(base, bound_pos, fluid_pos, seed + 1000, lo, hi)
    c._cloud_key = ("round_" + name, seed, coefh, dp, False)
    return c


def named_case(name, coefh=1.0, cellmode=1, tdensity=2):
    """A cloud by name, or "dam": a small dam break (dp 0.03) on its lattice."""
    if name == "dam":
        from dualsphysics_multilayer_amd.case import DamBreakCase

        return DamBreakCase(0.03, coefh=coefh, cellmode=cellmode, tdensity=tdensity)
    return make(name, coefh=coefh, cellmode=cellmode, tdensity=tdensity)


def child(name, coefh, cellmode, out):
    """One process of the hook comparison (the library reads SPH_TILE_FULL once per process):
    one interaction, then 25 steps, saved to `out`."""
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    g = SphGpuSingle(named_case(name, float(coefh), int(cellmode)), device=0)
    i = g.interaction()
    g.Run(25)
    g.sync()
    p = g.particles()
    arrays = {"p_" + k: np.asarray(v) for k, v in p.items() if isinstance(v, np.ndarray)}
    np.savez(out, ar=i["ar"], ace=i["ace"], maxima=np.array([i["viscdtmax"], i["velmax"], i["acemax"]], np.float64),
             **arrays)
    g.close()


def windows(case, K):
    """Per fluid item, kind of neighbour row (0 fluid, 1 bound) and tile_unit call of
    run_pass (CellMode=full): a dict with
      item, n (particles of the item), kind, unit,
      wave  [n]  the wave (0/1) of each particle, particles in lane order,
      la, lb [n] the lengths of the lane's two windows (lb = 0 for a single row),
      segn       records in the staged segment,
      atend [n]  the lane's last non-empty window ends on the segment's last record.
    Particles of one cell in the case's order (the order inside a cell changes neither a
    window nor an item's cells)."""
    c, nc = clouds._cells(case, K)
    assert int(K["scelldiv"]) == 1
    ncx, ncy, ncz = (int(v) for v in nc)
    scell = float(np.float32(K["scell"]))
    rel = case.pos - np.asarray(K["map_realposmin"]) - c * scell
    npb = case.npb
    pre = {}
    for kind, sl in ((0, slice(npb, None)), (1, slice(0, npb))):
        hist = np.zeros((ncz, ncy, ncx), np.int64)
        np.add.at(hist, (c[sl, 2], c[sl, 1], c[sl, 0]), 1)
        pre[kind] = np.concatenate([np.zeros((ncz, ncy, 1), np.int64), hist.cumsum(axis=2)], axis=2)
    cf, relf = c[npb:], rel[npb:]
    order = np.lexsort((cf[:, 0], cf[:, 1], cf[:, 2]))
    cf, relf = cf[order], relf[order]
    rowkey = cf[:, 1] + ncy * cf[:, 2]
    hs = 0.5 * scell
    UNITS = ((-1, -1), (-1, 1), (-1, 0), (0, -1), (0, 0))  # (dza, dya)
    out = []
    item = 0
    for key in np.unique(rowkey):
        idx = np.nonzero(rowkey == key)[0]
        cy, cz = int(key % ncy), int(key // ncy)
        pr = pre[0][cz, cy]
        p, pend, cc = 0, int(pr[ncx]), 0
        while p < pend:
            while pr[cc + 1] <= p:
                cc += 1
            q = int(min(p + TB, pend, pr[min(cc + TMAXCELLS, ncx)]))
            e = cc
            while pr[e + 1] < q:
                e += 1
            sel = idx[p:q]
            low = np.abs(relf[sel, 1] - hs) + np.abs(relf[sel, 2] - hs) < hs
            lane = np.concatenate([np.nonzero(low)[0], np.nonzero(~low)[0]])
            sel = sel[lane]
            n = len(sel)
            wave = np.arange(n) // 64
            xa, xb = max(cc - 1, 0), min(e + 1, ncx - 1)
            lxa, lxb = np.maximum(cf[sel, 0] - 1, 0), np.minimum(cf[sel, 0] + 1, ncx - 1)
            for kind in (0, 1):
                for u, (dza, dya) in enumerate(UNITS):
                    rs, re, ls, le = [0, 0], [0, 0], [np.zeros(n, np.int64)] * 2, [np.zeros(n, np.int64)] * 2
                    for k in range(2 if u < 4 else 1):
                        z, y = cz + (-dza if k else dza), cy + (-dya if k else dya)
                        if z < 0 or z >= ncz or y < 0 or y >= ncy:
                            continue
                        r = pre[kind][z, y]
                        rs[k], re[k], ls[k], le[k] = int(r[xa]), int(r[xb + 1]), r[lxa], r[lxb + 1]
                    n0, n1 = re[0] - rs[0], re[1] - rs[1]
                    if n0 + n1 == 0:
                        continue
                    base = dict(item=item, n=n, kind=kind, unit=u, wave=wave)
                    if n0 + n1 <= TCAP:
                        la = (le[0] - ls[0]) if n0 else np.zeros(n, np.int64)
                        lb = (le[1] - ls[1]) if n1 else np.zeros(n, np.int64)
                        wa1 = ls[0] - rs[0] + la
                        wb1 = n0 + ls[1] - rs[1] + lb
                        atend = np.where(lb > 0, wb1 == n0 + n1, (la > 0) & (wa1 == n0 + n1))
                        out.append(dict(base, la=la, lb=lb, segn=n0 + n1, atend=atend))
                    else:
                        for k in range(2):
                            for seg in range(rs[k], re[k], TCAP):
                                segn = min(TCAP, re[k] - seg)
                                w0 = np.maximum(ls[k], seg) - seg
                                w1 = np.maximum(w0, np.minimum(le[k], seg + segn) - seg)
                                out.append(dict(base, la=w1 - w0, lb=np.zeros(n, np.int64), segn=segn,
                                                atend=(w1 > w0) & (w1 == segn)))
            item += 1
            p = q
    return out


if __name__ == "__main__":
    import sys

    child(*sys.argv[1:5])
