"""Gauges on the GPU (csrc/sph_gauge.hip through the C-ABI and the run driver).

  * kernel against brute force — dam break dp 0.05 after 25 steps (full / half cells, Verlet /
    Symplectic): sph_solver_measure of ~200 gauges against a NumPy evaluation over EVERY fluid
    particle of the downloaded state, float32 pair terms as the reference forms them, float64
    sums.  Tolerance 16 * 2^-24 * sum|term| per component (the float pair term is ~10
    operations whose rounding and contraction may differ; the sums are double); MaxZ and the
    out-of-domain zeros are exact; two calls give identical bits.
  * against the reference — the four fixture cases of tests/golden/gauges through CaseRun:
    header, row count and configuration columns equal, times within the dt-trace tolerance
    (1e-5 relative) plus the print quantum, every value within 10x the stored fast-vs-strict
    floor of its column plus half a unit of its sixth printed digit.
  * device resident — run(60) as one batch and one drain = 60 x run(1), bitwise.
  * overflow, refusals, and PARTs that do not change with gauges.
"""
import glob
import os

import numpy as np
import pytest

from test_gauges import CASES, GDIR, case_dir, load_case, load_meta, read_golden

from dualsphysics_multilayer_amd.case import DamBreakCase
from dualsphysics_multilayer_amd.gauges import csv_name

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 16.0 * 2.0 ** -24


def gpu(case):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    return SphGpuSingle(case, device=0)


def gdef(type_, **kw):
    g = dict(type=type_, output=True, computestart=0.0, computeend=1e9, computedt=0.0, outputstart=0.0, outputend=1e9,
             outputdt=0.0, point0=[0.0] * 3, point2=[0.0] * 3, pointdir=[0.0] * 3, pointnp=0, masslimit=0.0,
             height=0.0, distlimit=0.0, code=0)
    g.update(kw)
    return g


def line(p0, p2, n, masslimit):
    """An SWL gauge of n + 1 points (PointNp = n) from p0 to p2."""
    d = [(b - a) / n for a, b in zip(p0, p2)] if n else [0.0] * 3
    return gdef("swl", point0=list(p0), point2=list(p2), pointdir=d, pointnp=n, masslimit=masslimit)


def gauge_set(k):
    """~200 gauges on the dam break dp 0.05 (tank 1.6 x 0.65 x 0.4, fluid after 25 steps about
    x <= 0.42, z <= 0.3)."""
    rng = np.random.default_rng(7)
    lo = np.array(k["map_realposmin"])
    hi = lo + np.array(k["map_realsize"])
    ml = float(F32(k["massfluid"]) * F32(0.5))
    gs = []
    for p in rng.uniform([0.03, 0.03, 0.03], [0.45, 0.62, 0.33], (150, 3)):  # in and around the fluid
        gs.append(gdef("velocity", point0=p.tolist()))
    for p in ([1.2, 0.3, 0.3], [0.9, 0.5, 0.1], [1.55, 0.1, 0.35]):  # empty cells
        gs.append(gdef("velocity", point0=p))
    tiny = 1e-9
    for cx in (0, 1):  # the corner cells of the domain and points on its edges
        for cy in (0, 1):
            for cz in (0, 1):
                c = [(hi[a] - tiny) if s else (lo[a] + tiny) for a, s in enumerate((cx, cy, cz))]
                gs.append(gdef("velocity", point0=c))
    gs.append(gdef("velocity", point0=[float(lo[0]), 0.3, 0.1]))   # on the lower limit: inside
    gs.append(gdef("velocity", point0=[0.05, float(lo[1]) + tiny, 0.05]))
    for p in ([5.0, 0.3, 0.15], [0.2, -3.0, 0.1], [0.2, 0.3, float(hi[2])], [float(lo[0]) - 1e-6, 0.3, 0.1],
              [float("nan"), 0.3, 0.1]):  # outside (the upper limit is outside)
        gs.append(gdef("velocity", point0=p))
    gs.append(line((0.2, 0.3, 0.06), (0.2, 0.3, 0.44), 63, ml))      # vertical, 64 points
    gs.append(line((0.11, 0.13, 0.06), (0.9, 0.5, 0.4), 64, ml))     # oblique, 65 points
    gs.append(line((0.06, 0.3, 0.1), (1.5, 0.3, 0.1), 149, ml))      # horizontal, 150 points
    gs.append(line((0.31, 0.4, 0.2), (0.31, 0.4, 0.2), 0, ml))       # one point
    gs.append(line((0.1, 0.3, 0.1), (0.3, 0.3, 0.1), 20, ml))        # all wet
    gs.append(line((1.0, 0.3, 0.3), (1.4, 0.3, 0.35), 30, ml))       # all dry
    gs.append(line((0.38, 0.2, 0.4), (0.38, 0.2, 0.05), 33, ml))     # downwards: dry, then wet
    gs.append(gdef("maxz", point0=[0.3, 0.335, 0.0], height=float(F32(0.4)), distlimit=float(F32(0.045))))
    # a short line: with half cells its cell box ends below the top of the fluid
    gs.append(gdef("maxz", point0=[0.2, 0.21, 0.0], height=float(F32(0.05)), distlimit=float(F32(0.03))))
    gs.append(gdef("force", code=0))
    return gs


def wendland(k, rr2):
    """GetKernelWendland_Wab and _Fac in float32 (FunSphKernel.h:206-222)."""
    h, awen, bwen = F32(k["kernelh"]), F32(k["awen"]), F32(k["bwen"])
    rad = np.sqrt(rr2)
    qq = rad / h
    wqq = qq + qq + F32(1)
    wqq1 = F32(1) - F32(0.5) * qq
    wqq2 = wqq1 * wqq1
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = bwen * qq * wqq1 * wqq1 * wqq1 / rad
    return awen * wqq * wqq2 * wqq2, fac


def pair_sums(k, fl, pts):
    """Per point: float64 sums of the float32 terms wab*vel (3) and wab*massfluid, and of
    their magnitudes, over every fluid particle."""
    mf, ks2 = F32(k["massfluid"]), F32(k["kernelsize2"])
    out, mag = np.zeros((len(pts), 4)), np.zeros((len(pts), 4))
    for i, p in enumerate(pts):
        dr = (p[None, :] - fl["pos"]).astype(F32)
        rr2 = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]
        m = (rr2 <= ks2) & (rr2 >= F32(1e-18))
        if not m.any():
            continue
        wab, _ = wendland(k, rr2[m])
        wab = wab * (mf / fl["rhop"][m])
        terms = np.concatenate([wab[:, None] * fl["vel"][m], (wab * mf)[:, None]], axis=1)
        out[i] = terms.astype(np.float64).sum(axis=0)
        mag[i] = np.abs(terms).astype(np.float64).sum(axis=0)
    return out, mag


def press(k, rho):
    """ComputePress in float32, the power rounded once from double (gamma = 7 by squaring)."""
    assert k["gamma"] == 7.0
    x = (rho / F32(k["rhopzero"])).astype(np.float64)
    x2 = x * x
    x4 = x2 * x2
    pw = ((x * x2) * x4).astype(F32)
    return F32(k["cteb"]) * (pw - F32(1))


def brute_force(k, p, npb):
    """The force gauge on every boundary particle from every fluid particle."""
    fl = p["idp"] >= npb
    bp, bq = p["pos"][~fl], p["rhop"][~fl]
    fp, fq = p["pos"][fl], p["rhop"][fl]
    mf, ks2 = F32(k["massfluid"]), F32(k["kernelsize2"])
    pf = press(k, fq)
    tot, mag = np.zeros(3), np.zeros(3)
    for i in range(len(bp)):
        dr = (bp[i][None, :] - fp).astype(F32)
        rr2 = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]
        m = (rr2 <= ks2) & (rr2 >= F32(1e-18))
        if not m.any():
            continue
        _, fac = wendland(k, rr2[m])
        fr = fac[:, None] * dr[m]
        p1 = press(k, bq[i:i + 1])[0]
        prs = (p1 + pf[m]) / (bq[i] * fq[m])
        terms = (-prs * mf)[:, None] * fr
        tot += terms.astype(np.float64).sum(axis=0)
        mag += np.abs(terms).astype(np.float64).sum(axis=0)
    mb = F32(k["massbound"])
    return tot.astype(F32) * mb, mag * float(mb)


def swl_expected(g, masses, mtol, pts):
    """JGaugeSwl::CalculeCpuT on the brute-force masses: (surface, tolerance per component)."""
    ml = F32(g["masslimit"])
    d = np.array(g["pointdir"])
    mpre, ipre = F32(0), -1
    for cp in range(g["pointnp"] + 1):
        mass = F32(masses[cp])
        # the scan is only decided when no mass sits within its tolerance of MassLimit
        assert abs(float(mass) - float(ml)) > mtol[cp] + 2.0 ** -24 * float(mass), "mass too close to MassLimit"
        if mass > ml:
            mpre, ipre = mass, cp
        if mass < ml and mpre:
            den = float(mass) - float(mpre)
            fxm1 = (ml - mpre) / (mass - mpre) - F32(1)
            df = (mtol[ipre] * abs(float(ml) - float(mass)) + mtol[cp] * abs(float(ml) - float(mpre))) / den ** 2
            df += 4 * 2.0 ** -24 * (abs(float(fxm1)) + 2)
            pos = pts[cp] + d * float(fxm1)
            return pos.astype(F32), np.abs(d) * df + 2.0 ** -23 * np.abs(pos)
    pos = np.array(g["point0"]) + d * (float(g["pointnp"]) if mpre else 0.0)
    return pos.astype(F32), 2.0 ** -23 * np.abs(pos)


@pytest.mark.parametrize("cellmode,step", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_kernels_match_brute_force(cellmode, step):
    from dualsphysics_multilayer_amd.core import case_derive

    case = DamBreakCase(0.05, cellmode=cellmode, step_algorithm=step)
    k = case_derive(case.case_def())
    s = gpu(case)
    gs = gauge_set(k)
    s.set_gauges(gs, 4096)
    s.run(25)
    s.sync()
    got = s.measure()
    again = s.measure()
    assert got.tobytes() == again.tobytes()
    assert np.all(got["time"] == s.stats()["time"]) and np.array_equal(got["gauge"], np.arange(len(gs)))
    p = s.particles()
    fluid = p["idp"] >= case.npb
    fl = {key: p[key][fluid] for key in ("pos", "vel", "rhop")}
    lo = np.array(k["map_realposmin"])
    hi = lo + np.array(k["map_realsize"])
    scell = float(F32(k["scell"]))
    nvel = nout = nwet = 0
    for gi, g in enumerate(gs):
        v = got["v"][gi]
        p0 = np.array(g["point0"])
        if g["type"] == "velocity":
            if not (np.all(p0 >= lo) and np.all(p0 < hi)):  # PointIsOut (NaN included): exact zeros
                assert np.all(v == 0) and not np.any(np.signbit(v)), (gi, v)
                nout += 1
                continue
            ref, mag = pair_sums(k, fl, p0[None, :])
            assert np.all(np.abs(v - ref[0, :3]) <= EPS * mag[0, :3] + 2.0 ** -24 * np.abs(ref[0, :3])), (gi, v, ref[0])
            nvel += mag[0, 3] > 0
        elif g["type"] == "swl":
            pts = [p0.copy()]
            for _ in range(g["pointnp"]):
                pts.append(pts[-1] + np.array(g["pointdir"]))  # ptpos = ptpos + PointDir
            pts = np.array(pts)
            ref, mag = pair_sums(k, fl, pts)
            exp, tol = swl_expected(g, ref[:, 3], EPS * mag[:, 3], pts)
            assert np.all(np.abs(v - exp) <= tol), (gi, v, exp, tol)
            nwet += ref[:, 3].max() > g["masslimit"]
        elif g["type"] == "maxz":
            # every fluid particle of the gauge's cell box (GetInteractionCellsMaxZ: the z cells
            # from the line's foot - ncel to its top + ncel), float32 horizontal distance
            dl = F32(g["distlimit"])
            ncel = int(np.ceil(dl / F32(k["scell"])))
            cz = int((p0[2] - lo[2]) / scell)
            cz2 = int((p0[2] + g["height"] - lo[2]) / scell)
            pc = ((fl["pos"][:, 2] - lo[2]) / scell).astype(np.int64)
            drx, dry = (p0[0] - fl["pos"][:, 0]).astype(F32), (p0[1] - fl["pos"][:, 1]).astype(F32)
            rr2 = drx * drx + dry * dry
            m = (rr2 <= dl * dl) & (pc >= max(cz - ncel, 0)) & (pc < min(cz2 + ncel + 1, k["dom_cells"][2]))
            assert m.any()
            exp = max(F32(fl["pos"][m, 2].max()), F32(lo[2]))
            assert v[0] == exp and v[1] == 0 and v[2] == 0, (gi, v, exp)
        else:
            ref, mag = brute_force(k, p, case.npb)
            assert np.all(np.abs(v - ref) <= EPS * mag + 2.0 ** -23 * np.abs(ref)), (v, ref, mag)
            assert np.linalg.norm(ref) > 50  # the water column's weight on the walls, not noise
    assert nvel > 100 and nout == 5 and nwet >= 5


def run_case(name, tmp_path, dirout, with_gauges=True, nsteps=None, save=False, **kw):
    from dualsphysics_multilayer_amd.run import CaseRun

    def strip(x):
        i, j = x.index("<special>"), x.index("</special>") + len("</special>")
        return x[:i] + x[j:]

    c = load_case(name, tmp_path, None if with_gauges else strip)
    m = load_meta(name)
    r = CaseRun(c, str(dirout), nsteps_break=nsteps or m["nsteps"], sv_all_steps=True, sv_pos_double=True, save=save,
                log=lambda s: None, **kw)
    try:
        r.run()
    finally:
        r.close()
    return c


@pytest.mark.parametrize("name", CASES)
def test_csv_files_match_the_reference(name, tmp_path):
    out = tmp_path / "out"
    c = run_case(name, tmp_path, out)
    m = load_meta(name)
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GDIR, name, "Gauges*.csv")))
    assert sorted(f for f in os.listdir(out) if f.startswith("Gauges")) == files
    bad = []
    for g in c.gauges:
        fn = csv_name(g)
        head, gold = read_golden(name, fn)
        with open(out / fn) as fh:
            lines = fh.read().split("\n")
        mine = [ln.split(";") for ln in lines[1:] if ln]
        assert lines[0] == head and len(mine) == len(gold), fn
        cols = head.split(";")
        nval = {"velocity": 3, "swl": 3, "maxz": 1, "force": 4}[g["type"]]
        worst = {}
        for a, b in zip(mine, gold):
            assert a[1 + nval:] == b[1 + nval:], (fn, a, b)  # the configuration columns
            ta, tb = float(a[0]), float(b[0])
            assert abs(ta - tb) <= 1e-5 * tb + 1.0001e-6, (fn, a[0], b[0])
            for cidx in range(1, 1 + nval):
                va, vb = float(a[cidx]), float(b[cidx])
                big = max(abs(va), abs(vb))
                half = 0.5 * 10.0 ** (np.floor(np.log10(big)) - 5) if big > 0 else 0.0
                tol = 10.0 * m["noise"][fn][cols[cidx]] + half
                d = abs(va - vb)
                if cols[cidx] not in worst or d - tol > worst[cols[cidx]][0] - worst[cols[cidx]][1]:
                    worst[cols[cidx]] = [d, tol]  # the row closest to (or furthest past) its tolerance
                if d > tol * (1 + 1e-9):
                    bad.append((fn, cols[cidx], b[0], va, vb, tol))
        print("%s %s: largest |difference| (its tolerance) " % (name, fn) +
              ", ".join("%s %.3g (%.3g)" % (kk, vv[0], vv[1]) for kk, vv in worst.items()))
    assert not bad, bad[:10]


def test_one_batch_is_sixty_single_steps():
    from dualsphysics_multilayer_amd.core import case_derive

    case = DamBreakCase(0.05)
    gs = gauge_set(case_derive(case.case_def()))[::9] + [gdef("force", code=0)]
    gs[1]["computedt"] = 0.002
    gs[2]["outputdt"] = 0.003
    a, b = gpu(case), gpu(case)
    a.set_gauges(gs, 4096)
    b.set_gauges(gs, 4096)
    a.run(60)
    ra = a.gauge_records()
    for _ in range(60):
        b.run(1)
    rb = b.gauge_records()
    assert len(ra) > 60 * (len(gs) - 2) and ra.tobytes() == rb.tobytes()
    assert np.all(np.diff(ra["time"]) >= 0) and len(a.gauge_records()) == 0
    # in a step the records come in gauge order
    same = np.diff(ra["time"]) == 0
    assert np.all(np.diff(ra["gauge"].astype(np.int64))[same] > 0)


def test_overflow_sets_the_flag_and_keeps_the_earlier_records():
    case = DamBreakCase(0.05)
    gs = [gdef("velocity", point0=[0.2, 0.3, 0.1 + 0.01 * i]) for i in range(7)]
    big, small = gpu(case), gpu(case)
    big.set_gauges(gs, 4096)
    small.set_gauges(gs, 10)
    big.run(5)
    small.run(5)
    small.sync()  # not fatal: no error is raised
    full = big.gauge_records()
    assert len(full) == 42 and not big.gauge_overflow()
    assert small.gauge_overflow() and small.stats()["error_flags"] == 64
    kept = small.gauge_records()
    assert len(kept) == 10 and kept.tobytes() == full[:10].tobytes()
    # the run itself went on unchanged
    assert small.stats()["time"] == big.stats()["time"] and small.stats()["nstep"] == 5


def test_refusals():
    from dualsphysics_multilayer_amd.core import SphError, SphSlabGroup, slab_partition

    case = DamBreakCase(0.05)
    gs = [gdef("velocity", point0=[0.2, 0.3, 0.1])]
    s = gpu(case)
    with pytest.raises(SphError, match="fixed or moving") as e:
        s.set_gauges([gdef("force", code=0x1000)], 64)
    assert e.value.status == 7
    with pytest.raises(SphError, match="no gauges"):
        s.gauge_records()
    s.run(1)
    with pytest.raises(SphError, match="before the first step") as e:
        s.set_gauges(gs, 64)
    assert e.value.status == 3
    grp = SphSlabGroup(case, slab_partition(case, 2))
    with pytest.raises(SphError, match="slabs") as e:
        grp.members[0].set_gauges(gs, 64)
    assert e.value.status == 7
    grp.close()


def test_parts_do_not_change_with_gauges(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    run_case("dambreak_verlet", tmp_path / "a", tmp_path / "a" / "out", with_gauges=True, nsteps=12, save=True)
    run_case("dambreak_verlet", tmp_path / "b", tmp_path / "b" / "out", with_gauges=False, nsteps=12, save=True)
    parts = sorted(f for f in os.listdir(tmp_path / "b" / "out") if f.startswith("Part_"))
    assert len(parts) == 14 and not [f for f in os.listdir(tmp_path / "b" / "out") if f.startswith("Gauges")]
    for fn in parts:
        with open(tmp_path / "a" / "out" / fn, "rb") as fa, open(tmp_path / "b" / "out" / fn, "rb") as fb:
            assert fa.read() == fb.read(), fn
