"""Generate the fixtures of the inlet/outlet zones by running the REFERENCE solver (build
container only: needs the binaries of ``make -C oracle`` and ``make -C oracle strict``).

The cases come from the product's own generator (case.py InOutChannelCase, written with the
project's .bi4 writer): that the reference loads and runs them is the check that they are well
formed.

tests/golden/bi4/inout_<variant>/
  CaseInOut.xml / .bi4   the case; 3d_verlet_ddt2_extrap_half is a run of the case in
                         inout_3d_verlet_ddt2_extrap
  ref.npz                the reference run (-nsteps:N -svsteps:1 -saveposdouble:1): PART 0 and the
                         PARTs at the kept steps (s<k>_idp/pos/vel/rhop, sorted by idp; s<k>_time;
                         s<k>_nout = particles excluded up to it), every PART's time (times),
                         particle count (nps) and largest idp (idmaxs), noise_<k> = [dpos, dvel,
                         drho] between the fast-math and the strict build at the kept steps, and
                         for EVERY step guard[k] = the smallest distance of a particle to the inlet
                         plane or to a zone's far face and noisepos[k] = the position noise there;
                         case_np, column (particles of one inlet column), removed_input /
                         removed_zsurf (fluid particles that vanished on entering the zone with
                         inputtreatment 2 / on entering the other zone above its zsurf with
                         `remove`, told from the PART before: outside every zone there, inside
                         one a step later), map_posmin / map_posmax
Asserted here (and again by tests/test_inout.py from ref.npz alone):
  * by the last kept step at least two whole columns were created and as many particles removed;
    with inputtreatment 2 and `remove` at least one particle was removed by each;
  * at every step guard[k] > 100 noisepos[k], and both builds hold the same idp set at the kept
    steps: which particles exist does not depend on rounding.
Usage: python tests/golden/make_inout.py [variant]
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import load_dump  # noqa: E402

from dualsphysics_multilayer_amd.case import InOutChannelCase  # noqa: E402
from dualsphysics_multilayer_amd.core import read_part  # noqa: E402
from dualsphysics_multilayer_amd.xmlcase import load_case  # noqa: E402

DP = 0.02
D2 = dict(dp=DP, nx=40, ny=1, nz=16, depth=12, vel0=(3.5, 0.0, 0.0), data2d=True)
# Velocities: a variant's velocity is the one of a small scan (2.0 ... 2.6 m/s; the refilling case's
# fluid 0.5 ... 1.5 m/s) at which the run keeps the guard rule below by a factor > 100 (the rule
# is fixed, the velocity is what gives way).  In the refilling case the fluid starts slower
# (0.9 m/s) than the zones' particles move: the top layer, which has no inlet particles behind it
# (zsurf lies one layer below), slumps back over the inlet plane and is removed by the inlet's
# inputtreatment 2, while the layer entering the outlet above zsurf is removed by `remove`.
D3 = dict(dp=DP, nx=24, ny=10, nz=8, depth=5, vel0=(2.5, 0.0, 0.0))
EXTRAP3 = dict(D3, step_algorithm=1, tdensity=2, determlimit=1e-3,
               zones=[dict(inputtreatment=0, velocity=(2.5,), rhop=2), dict(inputtreatment=1, velocity=None, rhop=2)])
# variant: (case arguments, solver options, kept steps, the case directory it shares or None)
VARIANTS = {
    "2d_verlet_ddt3_fixed": (dict(D2, step_algorithm=1, tdensity=3, zones=[
        dict(inputtreatment=0, velocity=(3.5,), rhop=1, zsurf=12.5 * DP),
        dict(inputtreatment=1, velocity=(-3.5,), rhop=1, zsurf=12.5 * DP)]), [], (1, 75, 150), None),
    "2d_symplectic_ddt1_extrap": (dict(D2, step_algorithm=2, tdensity=1, determlimit=1e+3, zones=[
        dict(inputtreatment=0, velocity=(3.5,), rhop=2),
        dict(inputtreatment=1, velocity=None, rhop=2)]), [], (1, 75, 150), None),
    "3d_verlet_ddt2_extrap": (EXTRAP3, [], (1, 75, 150), None),
    "3d_verlet_ddt2_extrap_half": (EXTRAP3, ["-cellmode:half"], (1, 75, 150), "3d_verlet_ddt2_extrap"),
    "3d_verlet_ddt2_refill1": (dict(D3, vel0=(0.9, 0.0, 0.0), step_algorithm=1, tdensity=2, useboxlimit=True, zones=[
        dict(refilling=1, inputtreatment=2, velocity=(1.5, 2.2, 2.5, DP, 3 * DP, 5 * DP), rhop=1, zsurf=4.5 * DP,
             remove=True),
        dict(refilling=1, inputtreatment=1, velocity=(-2.5,), rhop=1, zsurf=4.5 * DP, remove=True)]),
        [], (1, 75, 150), None),
}
COMMON = ["-svsteps:1", "-nortimes:1", "-saveposdouble:1", "-sv:binx", "-svres:0", "-ompthreads:4"]
NSTEPS_MAX = 150
NP_MAX = 2500


def run_ref(exe, case, out, nsteps, opts):
    subprocess.check_call([os.path.join(REF, exe), case, out, "-nsteps:%d" % nsteps] + COMMON + opts,
                          stdout=subprocess.DEVNULL)


def dump(out, part, fn):
    subprocess.check_call([os.path.join(REF, "partdump_ref"), out, str(part), fn], stdout=subprocess.DEVNULL)
    t, idp, pos, vel, rho = load_dump(fn)
    o = np.argsort(idp, kind="stable")
    return t, idp[o], pos[o], vel[o], rho[o]


def zone_distance(zone, pos):
    """Depth of the positions behind the zone's plane (positive inside the zone), in double."""
    pl = np.asarray(zone["plane"], np.float64)
    return -(pos @ pl[:3] + pl[3])


def in_zone(zone, pos):
    """JSphInOutZone::InZone with the box limits, on float positions as there."""
    ps = pos.astype(np.float32)
    pl = zone["plane"]
    inbox = ((zone["boxlimitmin"] <= ps) & (ps <= zone["boxlimitmax"])).all(axis=1)
    return inbox & (pl[0] * ps[:, 0] + pl[1] * ps[:, 1] + pl[2] * ps[:, 2] + pl[3] < 0)


def make(name, cargs, opts, keep, shared):
    case = InOutChannelCase(**cargs)
    out_dir = os.path.join(HERE, "bi4", "inout_" + name)
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    tmp = tempfile.mkdtemp(prefix="inout_")
    try:
        path = case.write(tmp)
        if shared is None:
            for ext in (".xml", ".bi4"):
                shutil.copy(path + ext, out_dir)
        x = load_case(path)
        zones = x.inout["zones"]
        assert case.np + len(x.inout["init"]["idp"]) <= NP_MAX
        nsteps = keep[-1]
        assert nsteps <= NSTEPS_MAX and len(keep) == 3
        outs = {}
        for exe, tag in (("DualSPHysics5.2CPU_ref", "fast"), ("DualSPHysics5.2CPU_strict", "strict")):
            outs[tag] = os.path.join(tmp, "out_" + tag)
            run_ref(exe, path, outs[tag], nsteps, opts)
        arrays, times, nps, idmaxs, guard, noisepos, nout = {}, [], [], [], [], [], 0
        removed_input = removed_zsurf = 0
        fn = os.path.join(tmp, "p.bin")
        hdr = None
        prev = None
        for part in range(0, nsteps + 1):
            t, idp, pos, vel, rho = dump(outs["fast"], part, fn)
            _, ids, poss, vels, rhos = dump(outs["strict"], part, fn)
            times.append(t)
            nps.append(len(idp))
            idmaxs.append(int(idp.max()))
            hdr, _ = read_part(os.path.join(outs["fast"], "Part_%04u.bi4" % part))
            nout += int(hdr["nout"]) if part > 0 else 0
            common, ia, ib = np.intersect1d(idp, ids, return_indices=True)
            noisepos.append(np.abs(pos[ia] - poss[ib]).max())
            # the inlet plane and both zones' far faces (at the outlet plane a particle is only converted)
            din, dout = zone_distance(zones[0], pos), zone_distance(zones[1], pos)
            guard.append(min(np.abs(din).min(), np.abs(din - zones[0]["width"]).min(),
                             np.abs(dout - zones[1]["width"]).min()))
            if prev is not None:
                # What left since the last PART.  A PART holds no codes: a particle that was outside
                # every zone there and whose position a step later (pos + vel dt) lies inside one was
                # normal fluid that entered it.  Removed by the input treatment: it entered a zone
                # with inputtreatment 2; removed by zsurf: it entered a zone without inputtreatment 2
                # but with `remove`, above zsurf.
                gone = ~np.isin(prev[0], idp)
                p0 = prev[1][gone]
                p1 = p0 + prev[2][gone].astype(np.float64) * (t - times[-2])
                outside = np.ones(len(p0), bool)
                for z in zones:
                    outside &= ~in_zone(z, p0)
                for z in zones:
                    entered = outside & in_zone(z, p1)
                    if z["cfgupdate"] & 4:
                        removed_input += int(entered.sum())
                    elif z["cfgupdate"] & 8:
                        removed_zsurf += int((entered & (p1[:, 2].astype(np.float32) > np.float32(z["zsurf"]))).sum())
            prev = (idp, pos, vel)
            if part == 0 or part in keep:
                arrays.update({"s%d_idp" % part: idp, "s%d_pos" % part: pos, "s%d_vel" % part: vel,
                               "s%d_rhop" % part: rho, "s%d_time" % part: np.float64(t),
                               "s%d_nout" % part: np.int64(nout)})
                assert np.array_equal(idp, ids), "the strict build holds other particles at step %d" % part
                arrays["noise_%d" % part] = np.array([np.abs(pos - poss).max(), np.abs(vel - vels).max(),
                                                      np.abs(rho.astype(np.float64) - rhos).max()])
        guard, noisepos = np.array(guard), np.array(noisepos)
        column = int(zones[0]["npartinit"]) // int(zones[0]["layers"])
        created = idmaxs[-1] - idmaxs[0]
        removed = nps[0] + created - nps[-1]
        print(name, "np0", nps[0], "created", created, "column", column, "removed", removed, "nout", nout,
              "removed_input", removed_input, "removed_zsurf", removed_zsurf, "guard min", guard.min(),
              "noisepos max", noisepos.max(), "worst ratio", (guard / np.maximum(noisepos, 1e-300)).min())
        assert created >= 2 * column, created
        assert removed >= 2 * column, removed
        if zones[0]["cfgupdate"] & 4:
            assert removed_input >= 1
        if any(z["cfgupdate"] & 8 for z in zones):
            assert removed_zsurf >= 1
        assert (guard > 100 * noisepos).all(), (guard / np.maximum(noisepos, 1e-300)).min()
        arrays.update(times=np.array(times), nps=np.array(nps), idmaxs=np.array(idmaxs), guard=guard,
                      noisepos=noisepos, case_np=np.int64(case.np), column=np.int64(column),
                      removed_input=np.int64(removed_input), removed_zsurf=np.int64(removed_zsurf),
                      map_posmin=np.array(hdr["map_posmin"]), map_posmax=np.array(hdr["map_posmax"]))
        np.savez_compressed(os.path.join(out_dir, "ref.npz"), **arrays)
        print(name, "ok", {f: os.path.getsize(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))})
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for k, v in VARIANTS.items():
        if only is None or k == only:
            make(k, *v)
