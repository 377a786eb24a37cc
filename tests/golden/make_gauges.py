"""Generate the gauge fixtures by running the REFERENCE solver (build container only: needs
the binaries of ``make -C oracle``; ``--noise`` also those of ``make -C oracle strict``).

A case (a committed one, or one written by gencase_ref) gets a ``<special><gauges>`` block in
its XML and runs ``DualSPHysics5.2CPU_ref -nsteps:N -svsteps:1 -saveposdouble:1``.

tests/golden/gauges/<case>/
  <Case>.xml            the case XML with the gauges
  [<Case>.bi4]          the particles, when the case is not one of tests/golden/bi4
  Gauges*.csv           the reference's gauge files (data the reference writes)
  meta.json             run options, the particle file, the step times (double, from the PART
                        headers; times[0] = 0) and, with --noise, per file and column the
                        largest difference between the fast-math and the strict build's CSVs

MaxZ is discontinuous in the particle positions: the generator asserts that at every stored
step no fluid particle's horizontal distance from a MaxZ line is within 10 % of its DistLimit.

Usage: python tests/golden/make_gauges.py [--noise] [case ...]
"""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "gauges")
sys.path.insert(0, ROOT)

EVERY_STEP = ('<default><computedt value="0"/><computetime start="0" end="10"/><output value="true"/>'
              '<outputdt value="0"/><outputtime start="0" end="10"/></default>\n')

# (a), (b): the 3-D dam break dp 0.05 (fluid x 0.05-0.4, y 0.05-0.6, z 0.05-0.3)
G_DAMBREAK = EVERY_STEP + """<velocity name="VelStep"><point x="0.2" y="0.3" z="0.15"/></velocity>
<velocity name="VelDt"><computedt value="0.002"/><point x="0.33" y="0.12" z="0.26"/></velocity>
<velocity name="VelOut"><point x="5" y="0.3" z="0.15"/></velocity>
<_velocity name="Skipped"><point x="0" y="0" z="0"/></_velocity>
<swl name="SwlV"><point0 x="0.21" y="0.31" z="0.06"/><point2 x="0.21" y="0.31" z="0.44"/><pointdp coefdp="0.5"/></swl>
<swl name="SwlH"><outputdt value="0.003"/><point0 x="0.1" y="0.3" z="0.12"/><point2 x="1.0" y="0.3" z="0.12"/>
<pointdp coefdp="0.5"/><masslimit coef="0.5"/></swl>
<maxz name="MaxZ"><point0 x="0.3" y="0.335" z="0"/><height value="0.4"/><distlimit coefdp="0.9"/></maxz>
<force name="Wall"><target mkbound="0"/></force>
"""
# (c): the 2-D dam break dp 0.04 (tank 4 x 3 m, water 1 x 2 m)
G_DAMBREAK2D = EVERY_STEP + """<velocity name="VelStep"><point x="0.5" y="0" z="1.0"/></velocity>
<swl name="SwlV"><point0 x="0.5" y="0" z="0.1"/><point2 x="0.5" y="0" z="2.9"/><pointdp coefdp="0.5"/></swl>
<swl name="SwlH"><point0 x="0.2" y="0" z="0.5"/><point2 x="3.5" y="0" z="0.5"/><pointdp coefdp="1"/></swl>
<maxz name="MaxZ"><point0 x="0.61" y="0" z="0"/><height value="2.9"/><distlimit coefdp="0.9"/></maxz>
<force name="Wall"><target mkbound="0"/></force>
"""
# (d): the flume (piston mkbound 1, flap mkbound 2, floating box): the force on the moving
# piston pins the order gauges -> motion
G_FLUME = EVERY_STEP + """<velocity name="VelStep"><point x="0.3" y="0.15" z="0.1"/></velocity>
<force name="Piston"><target mkbound="1"/></force>
<force name="Flap"><target mkbound="2"/></force>
<swl name="SwlV"><point0 x="0.4" y="0.15" z="0.03"/><point2 x="0.4" y="0.15" z="0.38"/><pointdp coefdp="0.5"/></swl>
"""

CASES = {
    # name: (base dir under tests/golden or None, case name, generator args, gauges, solver options, nsteps)
    "dambreak_verlet": ("bi4", "CaseDambreak", None, G_DAMBREAK, [], 60),
    "dambreak_sym_half": ("bi4", "CaseDambreak", None, G_DAMBREAK, ["-symplectic", "-cellmode:half"], 60),
    "dambreak2d_verlet": (None, "CaseDambreak2D", ["0.04", None, "1", "2", "1.5", "CaseDambreak2D", "1", "2"],
                          G_DAMBREAK2D, [], 60),
    "flume_verlet": ("bi4/flume_verlet_ddt2", "CaseFlume", None, G_FLUME, [], 60),
}


def insert_gauges(xml: str, gauges: str) -> str:
    block = "<special>\n<gauges>\n" + gauges + "</gauges>\n</special>\n"
    if "<special>" in xml:
        raise SystemExit("the case already has a <special> block")
    i = xml.index("</execution>")
    return xml[:i] + block + xml[i:]


def read_csv(path):
    lines = open(path).read().splitlines()
    head = lines[0].split(";")
    rows = [[float(v) for v in ln.split(";")] for ln in lines[1:] if ln]
    return head, np.array(rows, np.float64).reshape(len(rows), len(head))


def check_maxz(case, outdir, nsteps):
    """No fluid particle within 10 % of DistLimit of a MaxZ line's radius, at every stored step."""
    from dualsphysics_multilayer_amd.core import read_part

    fluid0 = min(b["begin"] for b in case.blocks if b["type"] == "fluid")
    for g in case.gauges:
        if g["type"] != "maxz":
            continue
        worst = np.inf
        for part in range(nsteps + 1):
            _, p = read_part(os.path.join(outdir, "Part_%04u.bi4" % part))
            pos = p["pos"][p["idp"] >= fluid0]
            d = np.hypot(pos[:, 0] - g["point0"][0], pos[:, 1] - g["point0"][1])
            worst = min(worst, np.abs(d - g["distlimit"]).min())
        assert worst > 0.1 * g["distlimit"], (
            "MaxZ gauge %s: a fluid particle comes within %g of DistLimit %g; choose another DistLimit"
            % (g["name"], worst, g["distlimit"]))
        print("  maxz %s: closest approach to DistLimit %.4g (limit %.4g)" % (g["name"], worst, 0.1 * g["distlimit"]))


def make(name, noise):
    from dualsphysics_multilayer_amd.core import read_part
    from dualsphysics_multilayer_amd.xmlcase import XmlCase

    base, cname, gen, gauges, opts, nsteps = CASES[name]
    tmp = tempfile.mkdtemp(prefix="gauges_")
    try:
        if base is not None:  # a committed case
            for ext in (".xml", ".bi4"):
                shutil.copy(os.path.join(HERE, base, cname + ext), tmp)
        else:
            args = [tmp if a is None else a for a in gen]
            subprocess.check_call([os.path.join(REF, "gencase_ref")] + args, stdout=subprocess.DEVNULL)
        xmlfile = os.path.join(tmp, cname + ".xml")
        xml = insert_gauges(open(xmlfile).read(), gauges)
        open(xmlfile, "w").write(xml)
        runs = [("DualSPHysics5.2CPU_ref", "out")] + ([("DualSPHysics5.2CPU_strict", "out_strict")] if noise else [])
        for exe, o in runs:
            subprocess.check_call([os.path.join(REF, exe), os.path.join(tmp, cname), os.path.join(tmp, o),
                                   "-nsteps:%d" % nsteps, "-svsteps:1", "-saveposdouble:1", "-sv:binx", "-svres:0"]
                                  + opts, stdout=subprocess.DEVNULL)
        out = os.path.join(tmp, "out")
        times = [float(read_part(os.path.join(out, "Part_%04u.bi4" % p))[0]["timestep"]) for p in range(nsteps + 1)]
        check_maxz(XmlCase(os.path.join(tmp, cname)), out, nsteps)
        dst = os.path.join(OUT, name)
        shutil.rmtree(dst, ignore_errors=True)
        os.makedirs(dst)
        shutil.copy(xmlfile, dst)
        if base is None:
            shutil.copy(os.path.join(tmp, cname + ".bi4"), dst)
        meta = dict(case=cname, bi4=(os.path.join(base, cname + ".bi4") if base else None), options=opts,
                    nsteps=nsteps, times=times, noise={})
        for fn in sorted(glob.glob(os.path.join(out, "Gauges*.csv"))):
            shutil.copy(fn, dst)
            head, rows = read_csv(fn)
            print("  %s: %d rows" % (os.path.basename(fn), len(rows)))
            if noise:
                heads, rowss = read_csv(os.path.join(tmp, "out_strict", os.path.basename(fn)))
                assert heads == head and rowss.shape == rows.shape, fn
                meta["noise"][os.path.basename(fn)] = {h: float(np.abs(rows[:, c] - rowss[:, c]).max())
                                                       for c, h in enumerate(head)}
        if not noise:
            del meta["noise"]
        json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
        print(name, "ok")
    finally:
        shutil.rmtree(tmp)


def main():
    args = sys.argv[1:]
    noise = "--noise" in args
    names = [a for a in args if not a.startswith("-")] or list(CASES)
    for n in names:
        make(n, noise)


if __name__ == "__main__":
    main()
