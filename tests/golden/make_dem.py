"""Generate the fixtures of the DEM collisions of floating bodies (RigidAlgorithm 2, and the
collision-free RigidAlgorithm 0) by running the REFERENCE solver (build container only: needs the
binaries of ``make -C oracle`` and ``make -C oracle strict``).

tests/golden/bi4/dem_<variant>/
  CaseBlocks*.xml / .bi4 / Blocks_Materials.xml   case.py BlocksCase: a tank, a shallow pool and three
                                    floating boxes (one dropped on the floor, one thrown at the third)
  ref.npz                           the reference run (-nsteps:N -svsteps:1 -saveposdouble:1): PARTs at
                                    the kept steps (sorted by idp), every PART time, demdtforce of every
                                    PART header, noise_<k> = [dpos, dvel, drho] between the fast-math and
                                    the strict build, meta = [step algorithm, DensityDT, cell mode] of the
                                    command line (0: the case's own), contacts = [float-bound, float-float]
                                    pairs closer than Dp at the kept steps (asserted >= 1 each; the
                                    float-float one in 3-D), margin: how far the same case with
                                    RigidAlgorithm=1 lies from the fixture at the last kept step in
                                    parity tolerances max(10 noise, floor) (asserted > 100)
Usage: python tests/golden/make_dem.py [variant]
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
from make_forcing import FLOOR, dump, run_ref  # noqa: E402

from dualsphysics_multilayer_amd.case import BlocksCase  # noqa: E402
from dualsphysics_multilayer_amd.core import read_part  # noqa: E402

KEEP = (5, 30, 60)
# variant: (BlocksCase arguments, solver options)
VARIANTS = {
    "verlet_ddt2": (dict(), []),
    "symplectic_ddt1": (dict(), ["-symplectic", "-ddt:1"]),
    "verlet_ddt2_half": (dict(), ["-cellmode:half"]),
    "verlet_ddt3_2d": (dict(data2d=True, nx=40), ["-ddt:3"]),
    # collision-free: the dropped box would leave through the floor, so it sinks slowly instead
    "free_verlet_ddt2": (dict(rigidalgorithm=0, velini=((0.0, 0.0, -0.6), (2.0, 0.0, 0.0), (0.0, 0.0, 0.0))), []),
}


def contacts(case, idp, pos):
    """[float-bound, float-float] pairs closer than Dp among particles of different blocks."""
    block = np.full(case.np, -1)
    block[: case.nfixed] = 0
    o = case.nfixed
    for c, b in enumerate(case.boxes):
        block[o:o + len(b)] = c + 1
        o += len(b)
    blk = block[idp]
    ft = np.flatnonzero(blk > 0)
    nb = np.flatnonzero(blk >= 0)
    d = np.sqrt(((pos[ft][:, None, :] - pos[nb][None, :, :]) ** 2).sum(axis=2))
    hit = (d < case.dp) & (blk[ft][:, None] != blk[nb][None, :])
    return np.array([int((hit & (blk[nb][None, :] == 0)).sum()), int((hit & (blk[nb][None, :] > 0)).sum()) // 2])


def make(name, kw, opts):
    case = BlocksCase(**kw)
    cname = "CaseBlocks2D" if case.data2d else "CaseBlocks"
    nsteps = KEEP[-1]
    out_dir = os.path.join(HERE, "bi4", "dem_" + name)
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    tmp = tempfile.mkdtemp(prefix="dem_")
    try:
        case.write(tmp, cname)
        plain = os.path.join(tmp, "plain")  # the same case with RigidAlgorithm=1
        os.makedirs(plain)
        BlocksCase(**dict(kw, rigidalgorithm=1)).write(plain, cname)
        files = [cname + ".xml", cname + ".bi4", "Blocks_Materials.xml"]
        for f in files:
            shutil.copy(os.path.join(tmp, f), os.path.join(out_dir, f))
        outs = {}
        for exe, tag, cdir in (("DualSPHysics5.2CPU_ref", "fast", tmp), ("DualSPHysics5.2CPU_strict", "strict", tmp),
                               ("DualSPHysics5.2CPU_ref", "plain", plain)):
            outs[tag] = os.path.join(tmp, "out_" + tag)
            cwd = os.getcwd()
            os.chdir(cdir)  # the property file's path is relative to the working directory
            try:
                run_ref(exe, os.path.join(cdir, cname), outs[tag], nsteps, opts)
            finally:
                os.chdir(cwd)
        arrays, times, demdt = {}, [], []
        ncon = np.zeros(2, np.int64)
        fn = os.path.join(tmp, "p.bin")
        for part in range(nsteps + 1):
            t, idp, pos, vel, rho = dump(outs["fast"], part, fn)
            times.append(t)
            demdt.append(read_part(os.path.join(outs["fast"], "Part_%04d.bi4" % part))[0]["dem_dtforce"])
            if part in KEEP:
                arrays.update({"s%d_idp" % part: idp, "s%d_pos" % part: pos, "s%d_vel" % part: vel,
                               "s%d_rhop" % part: rho, "s%d_time" % part: np.float64(t)})
                _, ids, poss, vels, rhos = dump(outs["strict"], part, fn)
                assert np.array_equal(idp, ids), "strict build excluded other particles"
                arrays["noise_%d" % part] = np.array([np.abs(pos - poss).max(), np.abs(vel - vels).max(),
                                                      np.abs(rho.astype(np.float64) - rhos).max()])
                ncon = np.maximum(ncon, contacts(case, idp, pos))
        if case.rigidalgorithm == 2:
            assert ncon[0] >= 1, (name, "no float-bound contact at a kept step", ncon)
            assert case.data2d or ncon[1] >= 1, (name, "no float-float contact at a kept step", ncon)
            assert all(d > 0 for d in demdt), demdt
        _, idq, posq, velq, _ = dump(outs["plain"], nsteps, fn)
        assert np.array_equal(idp, idq), "the RigidAlgorithm=1 run excluded other particles"
        tol = [max(10.0 * float(arrays["noise_%d" % nsteps][i]), FLOOR[i]) for i in range(3)]
        margin = max(np.abs(pos - posq).max() / tol[0], np.abs(vel - velq).max() / tol[1])
        assert margin > 100, (name, margin)
        step = 2 if "-symplectic" in opts else 0
        ddt = ([int(o[5:]) for o in opts if o.startswith("-ddt:")] or [0])[0]
        cellmode = 2 if "-cellmode:half" in opts else 0
        arrays.update(times=np.array(times), demdtforce=np.array(demdt), meta=np.array([step, ddt, cellmode], np.float64),
                      margin=np.float64(margin), contacts=ncon)
        np.savez_compressed(os.path.join(out_dir, "ref.npz"), **arrays)
        print(name, "ok margin %.3g" % margin, "contacts", ncon, "noise", arrays["noise_%d" % nsteps], "times",
              [times[k] for k in KEEP], {f: os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)})
    finally:
        shutil.rmtree(tmp)


RST_PART, RST_KEEP = 30, (31, 45, 60)


def make_restart(name="restart_verlet_ddt2"):
    """The first variant restarted by the reference from its own PART 30 (after the first contact),
    so that DemDtForce comes from the file: Part_0030.bi4 + PartFloat.fbi4 are kept in the fixture."""
    case = BlocksCase()
    cname = "CaseBlocks"
    out_dir = os.path.join(HERE, "bi4", "dem_" + name)
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    tmp = tempfile.mkdtemp(prefix="dem_")
    cwd = os.getcwd()
    try:
        case.write(tmp, cname)
        plain = os.path.join(tmp, "plain")
        os.makedirs(plain)
        BlocksCase(rigidalgorithm=1).write(plain, cname)
        os.chdir(tmp)
        first = os.path.join(tmp, "out_first")
        run_ref("DualSPHysics5.2CPU_ref", os.path.join(tmp, cname), first, RST_PART, [])
        fn = os.path.join(tmp, "p.bin")
        _, idp0, pos0, _, _ = dump(first, RST_PART, fn)
        assert contacts(case, idp0, pos0).min() >= 1, "the restart PART lies before the first contact"
        for f in (cname + ".xml", cname + ".bi4", "Blocks_Materials.xml"):
            shutil.copy(os.path.join(tmp, f), os.path.join(out_dir, f))
        for f in ("Part_%04d.bi4" % RST_PART, "PartFloat.fbi4"):
            shutil.copy(os.path.join(first, f), os.path.join(out_dir, f))
        nsteps = RST_KEEP[-1] - RST_PART
        outs = {}
        for exe, tag, cdir in (("DualSPHysics5.2CPU_ref", "fast", tmp), ("DualSPHysics5.2CPU_strict", "strict", tmp),
                               ("DualSPHysics5.2CPU_ref", "plain", plain)):
            outs[tag] = os.path.join(tmp, "out_" + tag)
            os.chdir(cdir)
            run_ref(exe, os.path.join(cdir, cname), outs[tag], nsteps, ["-partbegin:%d" % RST_PART, first])
        os.chdir(cwd)
        h0 = read_part(os.path.join(first, "Part_%04d.bi4" % RST_PART))[0]
        assert h0["dem_dtforce"] > 0
        arrays = {}
        times, demdt = np.zeros(RST_KEEP[-1] + 1), np.zeros(RST_KEEP[-1] + 1)
        for part in range(RST_PART, RST_KEEP[-1] + 1):
            t, idp, pos, vel, rho = dump(outs["fast"], part, fn)
            times[part] = t
            demdt[part] = read_part(os.path.join(outs["fast"], "Part_%04d.bi4" % part))[0]["dem_dtforce"]
            if part in RST_KEEP:
                arrays.update({"s%d_idp" % part: idp, "s%d_pos" % part: pos, "s%d_vel" % part: vel,
                               "s%d_rhop" % part: rho, "s%d_time" % part: np.float64(t)})
                _, ids, poss, vels, rhos = dump(outs["strict"], part, fn)
                assert np.array_equal(idp, ids)
                arrays["noise_%d" % part] = np.array([np.abs(pos - poss).max(), np.abs(vel - vels).max(),
                                                      np.abs(rho.astype(np.float64) - rhos).max()])
        _, idq, posq, velq, _ = dump(outs["plain"], RST_KEEP[-1], fn)
        assert np.array_equal(idp, idq)
        last = RST_KEEP[-1]
        tol = [max(10.0 * float(arrays["noise_%d" % last][i]), FLOOR[i]) for i in range(3)]
        margin = max(np.abs(pos - posq).max() / tol[0], np.abs(vel - velq).max() / tol[1])
        assert margin > 100, (name, margin)
        arrays.update(times=times, demdtforce=demdt, meta=np.array([0, 0, 0], np.float64), margin=np.float64(margin),
                      partbegin=np.int64(RST_PART), demdtforce0=np.float64(h0["dem_dtforce"]))
        np.savez_compressed(os.path.join(out_dir, "ref.npz"), **arrays)
        print(name, "ok margin %.3g" % margin, "DemDtForce of the file", h0["dem_dtforce"], "first dt",
              times[RST_PART + 1] - times[RST_PART],
              {f: os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)})
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)


if __name__ == "__main__":
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for k, v in VARIANTS.items():
        if only is None or k == only:
            make(k, *v)
    if only in (None, "restart_verlet_ddt2"):
        make_restart()
