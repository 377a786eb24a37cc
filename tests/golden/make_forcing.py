"""Generate the fixtures of the imposed accelerations (<special><accinputs>, JDsAccInput) and
the damping zones (<special><damping>, JDsDamping) by running the REFERENCE solver (build
container only: needs the binaries of ``make -C oracle`` and ``make -C oracle strict``).

tests/golden/bi4/forcing_<variant>/
  Case*.xml / .bi4 [+ data files]   a committed case (the dam break of tests/golden/bi4, the
                                    flume of bi4/flume_verlet_ddt2) or gencase_ref's 2-D dam
                                    break, with a <special> block before </execution>
  ref.npz                           the reference run (-nsteps:N -svsteps:1 -saveposdouble:1):
                                    PARTs at the kept steps (sorted by idp), every PART time,
                                    noise_<k> = [dpos, dvel, drho] between the fast-math build
                                    and the strict build of the same sources, meta = [step
                                    algorithm, DensityDT] of the run's command line (0: the
                                    case's own), and margin: how far, at the last kept step,
                                    the same case WITHOUT the block lies from the fixture, in
                                    units of the parity tolerance max(10 noise, floor) (the
                                    larger of the position and velocity ratios; asserted
                                    > 100: a fixture the block does not move proves nothing)
Usage: python tests/golden/make_forcing.py [variant]
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
from make_golden import load_dump  # noqa: E402

FLOOR = (2e-10, 2e-7, 2.5e-3)  # tests/test_dtopt.py

DAMBREAK = ("bi4", "CaseDambreak", None)
FLUME = ("bi4/flume_verlet_ddt2", "CaseFlume", None)
DAMBREAK2D = (None, "CaseDambreak2D", ["0.04", None, "1", "2", "1.5", "CaseDambreak2D", "1", "2"])  # as make_gauges.py

ACC_LIN = """<accinputs>
<accinput mkfluid="0">
<acccentre x="0" y="0" z="0"/>
<globalgravity value="false"/>
<acctimes>
<timevalue time="0" linx="0" linz="0"/>
<timevalue time="0.01" linx="6" linz="-4"/>
<timevalue time="1" linx="6" linz="-4"/>
</acctimes>
</accinput>
</accinputs>
"""
# the window opens after the first kept step; the velocities are integrated from the first row
ACC_ANG = """<accinputs>
<accinput mkfluid="0">
<time start="%(tstart)s" end="10"/>
<acccentre x="0.8" y="0.1" z="0.05"/>
<globalgravity value="true"/>
<acctimesfile value="acc_ang.csv"/>
</accinput>
</accinputs>
"""
ACC_ANG_FILE = """# time;linx;liny;linz;angx;angy;angz
0;0;0;0;0;0;0
0.002;0.5;0;0;20;-60;10
0.02;1;0;0.5;30;-90;15
1;1;0;0.5;30;-90;15
"""
ACC_FLOAT = """<accinputs>
<accinput mkbound="3">
<acccentre x="0.65" y="0.15" z="0.1"/>
<globalgravity value="true"/>
<acctimes>
<timevalue time="0" linz="0" angy="0"/>
<timevalue time="0.005" linz="30" angy="200"/>
<timevalue time="1" linz="30" angy="200"/>
</acctimes>
</accinput>
<accinput mkfluid="0">
<acccentre x="0" y="0" z="0"/>
<globalgravity value="true"/>
<acctimes>
<timevalue time="0" linx="0"/>
<timevalue time="0.004" linx="-3" liny="1"/>
<timevalue time="1" linx="-3" liny="1"/>
</acctimes>
</accinput>
</accinputs>
"""
DAMP_PLANE = """<damping>
<dampingzone>
<limitmin x="0.15" y="0" z="0"/>
<limitmax x="0.4" y="0" z="0"/>
<overlimit value="0.3"/>
<redumax value="400"/>
</dampingzone>
</damping>
"""
# the <domain> points out of angular order (ComputeDomPlanes sorts 2-4 by their angle about 1)
DAMP_PLANE_DOM = """<damping>
<dampingzone>
<limitmin x="0.05" y="0" z="0"/>
<limitmax x="0.5" y="0" z="0"/>
<overlimit value="0.2"/>
<redumax value="800"/>
<factorxyz x="1" y="0.5" z="0.25"/>
<domain zmin="0" zmax="0.4">
<point1 x="0.0" y="0.06"/>
<point2 x="0.8" y="0.3"/>
<point3 x="0.8" y="0.06"/>
<point4 x="0.0" y="0.3"/>
</domain>
</dampingzone>
</damping>
"""
DAMP_BOX_CYL = """<damping>
<dampingbox>
<directions value="right,top"/>
<limitmin><pointini x="0" y="0" z="0"/><pointend x="0.25" y="0.65" z="0.15"/></limitmin>
<limitmax><pointini x="0" y="0" z="0"/><pointend x="0.45" y="0.65" z="0.35"/></limitmax>
<overlimit value="0.1"/>
<redumax value="300"/>
</dampingbox>
<dampingcylinder>
<point1 x="0.3" y="0.3" z="0"/>
<point2 x="0.3" y="0.3" z="1"/>
<limitmin radius="0.05"/>
<limitmax radius="0.2"/>
<overlimit value="0.05"/>
<redumax value="200"/>
<factorxyz x="1" y="1" z="0.5"/>
</dampingcylinder>
<dampingcylinder>
<point1 x="0.1" y="0" z="0.1"/>
<point2 x="0.5" y="0.65" z="0.3"/>
<limitmin radius="0.02"/>
<limitmax radius="0.15"/>
<overlimit value="0.05"/>
<redumax value="250"/>
</dampingcylinder>
</damping>
"""
ACC_DAMP_2D = """<accinputs>
<accinput mkfluid="0">
<acccentre x="2" y="0" z="1.5"/>
<globalgravity value="true"/>
<acctimes>
<timevalue time="0" linx="0" angy="0"/>
<timevalue time="0.005" linx="5" liny="2" angy="8"/>
<timevalue time="1" linx="5" liny="2" angy="8"/>
</acctimes>
</accinput>
</accinputs>
<damping>
<dampingzone>
<limitmin x="0.5" y="0" z="0"/>
<limitmax x="1.0" y="0" z="0"/>
<overlimit value="0.5"/>
<redumax value="300"/>
</dampingzone>
</damping>
"""

# variant: (case, solver options, kept steps, <special> body, data files, start of the inputs' time window or None)
VARIANTS = {
    "verlet_ddt2_acc_lin_nograv": (DAMBREAK, [], (1, 20, 60), ACC_LIN, {}, None),
    "symplectic_ddt1_acc_ang_file": (DAMBREAK, ["-symplectic", "-ddt:1"], (2, 30, 60), ACC_ANG % dict(tstart="0.004"),
                                     {"acc_ang.csv": ACC_ANG_FILE}, 0.004),
    "flume_verlet_ddt2_acc_float": (FLUME, [], (1, 20, 60), ACC_FLOAT, {}, None),
    "symplectic_ddt1_damp_plane": (DAMBREAK, ["-symplectic", "-ddt:1"], (1, 20, 60), DAMP_PLANE, {}, None),
    "flume_verlet_ddt2_damp_plane_dom": (FLUME, [], (1, 20, 60), DAMP_PLANE_DOM, {}, None),
    "verlet_ddt2_damp_box_cyl": (DAMBREAK, [], (1, 20, 60), DAMP_BOX_CYL, {}, None),
    "verlet_ddt2_acc_damp_2d": (DAMBREAK2D, [], (1, 20, 60), ACC_DAMP_2D, {}, None),
}


def run_ref(exe, case, out, nsteps, opts):
    subprocess.check_call([os.path.join(REF, exe), case, out, "-nsteps:%d" % nsteps, "-svsteps:1", "-nortimes:1",
                           "-saveposdouble:1", "-sv:binx", "-svres:0", "-ompthreads:4"] + opts,
                          stdout=subprocess.DEVNULL)


def dump(out, part, fn):
    subprocess.check_call([os.path.join(REF, "partdump_ref"), out, str(part), fn], stdout=subprocess.DEVNULL)
    t, idp, pos, vel, rho = load_dump(fn)
    o = np.argsort(idp, kind="stable")
    return t, idp[o], pos[o], vel[o], rho[o]


def make(name, case, opts, keep, block, files, tstart):
    base, cname, gen = case
    nsteps = keep[-1]
    assert len(keep) == 3 and nsteps <= 60
    out_dir = os.path.join(HERE, "bi4", "forcing_" + name)
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    tmp = tempfile.mkdtemp(prefix="forcing_")
    try:
        plain = os.path.join(tmp, "plain")  # the same case without the block
        os.makedirs(plain)
        if base is not None:
            for ext in (".xml", ".bi4"):
                shutil.copy(os.path.join(HERE, base, cname + ext), tmp)
        else:
            subprocess.check_call([os.path.join(REF, "gencase_ref")] + [tmp if a is None else a for a in gen],
                                  stdout=subprocess.DEVNULL)
        for ext in (".xml", ".bi4"):
            shutil.copy(os.path.join(tmp, cname + ext), plain)
        fx = os.path.join(tmp, cname + ".xml")
        xml = open(fx).read()
        assert "<special>" not in xml and xml.count("</execution>") == 1
        open(fx, "w").write(xml.replace("</execution>", "<special>\n" + block + "</special>\n</execution>"))
        for fn, body in files.items():
            open(os.path.join(tmp, fn), "w").write(body)
        for f in [cname + ".xml", cname + ".bi4"] + list(files):
            shutil.copy(os.path.join(tmp, f), os.path.join(out_dir, f))
        outs = {}
        for exe, tag, cdir in (("DualSPHysics5.2CPU_ref", "fast", tmp), ("DualSPHysics5.2CPU_strict", "strict", tmp),
                               ("DualSPHysics5.2CPU_ref", "plain", plain)):
            outs[tag] = os.path.join(tmp, "out_" + tag)
            run_ref(exe, os.path.join(cdir, cname), outs[tag], nsteps, opts)
        arrays, times = {}, []
        fn = os.path.join(tmp, "p.bin")
        for part in range(nsteps + 1):
            t, idp, pos, vel, rho = dump(outs["fast"], part, fn)
            times.append(t)
            if part in keep:
                arrays.update({"s%d_idp" % part: idp, "s%d_pos" % part: pos, "s%d_vel" % part: vel,
                               "s%d_rhop" % part: rho, "s%d_time" % part: np.float64(t)})
                _, ids, poss, vels, rhos = dump(outs["strict"], part, fn)
                assert np.array_equal(idp, ids), "strict build excluded other particles"
                arrays["noise_%d" % part] = np.array([np.abs(pos - poss).max(), np.abs(vel - vels).max(),
                                                      np.abs(rho.astype(np.float64) - rhos).max()])
        if tstart is not None:  # one kept step before the window, two inside
            assert times[keep[0]] < tstart <= times[keep[1] - 1], (times[keep[0]], tstart, times[keep[1] - 1])
        # the block is seen: the plain run leaves the fixture by > 100 tolerances at the last kept step
        _, idq, posq, velq, _ = dump(outs["plain"], nsteps, fn)
        assert np.array_equal(idp, idq), "the plain run excluded other particles"
        tol = [max(10.0 * float(arrays["noise_%d" % nsteps][i]), FLOOR[i]) for i in range(3)]
        margin = max(np.abs(pos - posq).max() / tol[0], np.abs(vel - velq).max() / tol[1])
        assert margin > 100, (name, margin)
        step = 2 if "-symplectic" in opts else 0
        ddt = ([int(o[5:]) for o in opts if o.startswith("-ddt:")] or [0])[0]
        arrays.update(times=np.array(times), meta=np.array([step, ddt], np.float64), margin=np.float64(margin))
        np.savez_compressed(os.path.join(out_dir, "ref.npz"), **arrays)
        print(name, "ok margin %.3g" % margin, "noise", arrays["noise_%d" % nsteps], "times",
              [times[k] for k in keep], sorted(os.listdir(out_dir)))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for k, v in VARIANTS.items():
        if only is None or k == only:
            make(k, *v)
