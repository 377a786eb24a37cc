"""Generate the fixtures of the periodic boundaries by running the REFERENCE solver (build
container only: needs the binaries of ``make -C oracle`` and ``make -C oracle strict``).

The cases come from the product's own generator (case.py PeriodicChannelCase, written with the
project's .bi4 writer): that the reference loads and runs them is the check that they are well
formed.

tests/golden/bi4/periodic_<variant>/
  CasePeriodic.xml / .bi4     the case (initial velocities in the .bi4); x_verlet_ddt2_half and
                              x_verlet_ddt2_restart are runs of the case in periodic_x_verlet_ddt2
  [Part_%04u.bi4]             restart variant: the reference's PART the restart begins from
  ref.npz                     the reference run (-nsteps:N -svsteps:1 -saveposdouble:1): PARTs at
                              the kept steps (sorted by idp), s<k>_nout = particles excluded up to
                              it, every PART time, noise_<k> = [dpos, dvel, drho] between the
                              fast-math and the strict build, and from the reference's PART header
                              map_posmin / map_posmax (MapRealPosMin/Max), peri_mode and
                              peri_xinc / peri_yinc / peri_zinc; restart variant: partbegin
Asserted here (and again by tests/test_periodic.py from ref.npz alone): by the last kept step at
least 20 fluid particles jumped by about one period between kept PARTs, in the two-axis case at
least 5 on each axis.
Usage: python tests/golden/make_periodic.py [variant]
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

from dualsphysics_multilayer_amd.case import PeriodicChannelCase  # noqa: E402
from dualsphysics_multilayer_amd.core import read_part  # noqa: E402

DP = 0.02
CHANNEL = dict(dp=DP, nx=24, ny=10, nz=8, depth=5, peri={"XPeriodicIncZ": 0}, vel0=(2.0, 0.0, 0.0), ywalls=True,
               step_algorithm=1, tdensity=2)
# variant: (case arguments, solver options, kept steps, restart PART or None)
VARIANTS = {
    "x_verlet_ddt2": (CHANNEL, [], (1, 30, 60), None),
    "x_verlet_ddt2_half": (CHANNEL, ["-cellmode:half"], (1, 30, 60), None),
    "xy_incy_symplectic_ddt1": (dict(dp=DP, nx=24, ny=20, nz=6, depth=4,
                                     peri={"XPeriodicIncY": 3 * DP, "YPeriodicIncZ": 0}, vel0=(1.5, 1.0, 0.0),
                                     step_algorithm=2, tdensity=1), [], (2, 30, 60), None),
    # (a step moves a particle 0.02 h at most, whatever its speed: 100 steps for two columns)
    "x_2d_verlet_ddt3": (dict(dp=DP, nx=40, ny=1, nz=16, depth=12, peri={"XPeriodicIncZ": 0}, vel0=(3.5, 0.0, 0.0),
                              data2d=True, step_algorithm=1, tdensity=3), [], (1, 50, 100), None),
    "x_verlet_ddt2_restart": (CHANNEL, [], (40,), 25),
}
COMMON = ["-svsteps:1", "-nortimes:1", "-saveposdouble:1", "-sv:binx", "-svres:0", "-ompthreads:4"]


def run_ref(exe, case, out, nsteps, opts):
    subprocess.check_call([os.path.join(REF, exe), case, out, "-nsteps:%d" % nsteps] + COMMON + opts,
                          stdout=subprocess.DEVNULL)


def dump(out, part, fn):
    subprocess.check_call([os.path.join(REF, "partdump_ref"), out, str(part), fn], stdout=subprocess.DEVNULL)
    t, idp, pos, vel, rho = load_dump(fn)
    o = np.argsort(idp, kind="stable")
    return t, idp[o], pos[o], vel[o], rho[o]


def make(name, cargs, opts, keep, k0):
    case = PeriodicChannelCase(**cargs)
    assert case.np <= 5000
    out_dir = os.path.join(HERE, "bi4", "periodic_" + name)
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    tmp = tempfile.mkdtemp(prefix="periodic_")
    try:
        path = case.write(tmp)
        if cargs is not CHANNEL or name == "x_verlet_ddt2":  # the other runs of case 1 read its files
            for ext in (".xml", ".bi4"):
                shutil.copy(path + ext, out_dir)
        nsteps = keep[-1]
        outs = {}
        if k0 is None:
            first = 0
            for exe, tag in (("DualSPHysics5.2CPU_ref", "fast"), ("DualSPHysics5.2CPU_strict", "strict")):
                outs[tag] = os.path.join(tmp, "out_" + tag)
                run_ref(exe, path, outs[tag], nsteps, opts)
        else:
            # run A to PART k0, then both builds restarted from A's PART k0
            first = k0
            a = os.path.join(tmp, "a")
            run_ref("DualSPHysics5.2CPU_ref", path, a, k0, opts)
            shutil.copy(os.path.join(a, "Part_%04u.bi4" % k0), out_dir)
            for exe, tag in (("DualSPHysics5.2CPU_ref", "fast"), ("DualSPHysics5.2CPU_strict", "strict")):
                outs[tag] = os.path.join(tmp, "out_" + tag)
                run_ref(exe, path, outs[tag], nsteps - k0, opts + ["-partbegin:%d" % k0, a])
        arrays, times, nout = {}, [], 0
        fn = os.path.join(tmp, "p.bin")
        hdr = None
        for part in range(first, nsteps + 1):
            t, idp, pos, vel, rho = dump(outs["fast"], part, fn)
            times.append(t)
            hdr, _ = read_part(os.path.join(outs["fast"], "Part_%04u.bi4" % part))
            nout += int(hdr["nout"]) if part > first else 0
            if part in keep:
                arrays.update({"s%d_idp" % part: idp, "s%d_pos" % part: pos, "s%d_vel" % part: vel,
                               "s%d_rhop" % part: rho, "s%d_time" % part: np.float64(t),
                               "s%d_nout" % part: np.int64(nout)})
                _, ids, poss, vels, rhos = dump(outs["strict"], part, fn)
                assert np.array_equal(idp, ids), "strict build excluded other particles"
                # a particle within rounding of a periodic face may be wrapped by one build only:
                # compare positions modulo the periods
                d = pos - poss
                size = np.array(hdr["map_posmax"]) - np.array(hdr["map_posmin"])
                for ax in range(3):
                    if (hdr["peri_mode"] >> ax) & 1:
                        assert not (np.abs(d[:, ax]) > 0.5 * size[ax]).any(), "builds wrapped different particles"
                arrays["noise_%d" % part] = np.array([np.abs(d).max(), np.abs(vel - vels).max(),
                                                      np.abs(rho.astype(np.float64) - rhos).max()])
        size = np.array(hdr["map_posmax"]) - np.array(hdr["map_posmin"])
        wrapped = [set(), set(), set()]
        for a_, b_ in zip(keep[:-1], keep[1:]):
            d = arrays["s%d_pos" % b_] - arrays["s%d_pos" % a_]
            for ax in range(3):
                if (hdr["peri_mode"] >> ax) & 1:
                    wrapped[ax] |= set(arrays["s%d_idp" % a_][np.abs(d[:, ax]) > 0.5 * size[ax]].tolist())
        if k0 is None:
            assert len(wrapped[0] | wrapped[1] | wrapped[2]) >= 20, [len(w) for w in wrapped]
            if bin(hdr["peri_mode"]).count("1") == 2:
                assert min(len(wrapped[ax]) for ax in range(3) if (hdr["peri_mode"] >> ax) & 1) >= 5
        arrays.update(times=np.array(times), first=np.int64(first), map_posmin=np.array(hdr["map_posmin"]),
                      map_posmax=np.array(hdr["map_posmax"]), peri_mode=np.int64(hdr["peri_mode"]),
                      peri_xinc=np.array(hdr["peri_xinc"]), peri_yinc=np.array(hdr["peri_yinc"]),
                      peri_zinc=np.array(hdr["peri_zinc"]))
        if k0 is not None:
            arrays["partbegin"] = np.int64(k0)
        np.savez_compressed(os.path.join(out_dir, "ref.npz"), **arrays)
        print(name, "ok np", case.np, "wrapped", [len(w) for w in wrapped], "nout", nout, "noise",
              arrays["noise_%d" % nsteps], "peri", hdr["peri_mode"], hdr["peri_xinc"], hdr["peri_yinc"],
              {f: os.path.getsize(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))})
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for k, v in VARIANTS.items():
        if only is None or k == only:
            make(k, *v)
