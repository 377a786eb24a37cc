"""Gauges without a GPU: the XML loader, the schedule, the CSV writer and the run driver's
batching.

Fixtures (tests/golden/make_gauges.py, written by the REFERENCE solver): per case the XML
with its <special><gauges>, the reference's Gauges*.csv and the step times (meta.json).
  * XML — the dam-break gauge set loads into the definitions the reference logs (PointNp,
    PointDir, MassLimit, DistLimit, inherited timings); invalid blocks raise CaseError;
  * schedule — a C++ program (tests/cpp/gauge_sched_host.cpp) walks the golden step times
    through the Update / SetTimeStep / Output functions of csrc/sph_gauge.hpp and must store
    exactly the rows of every golden CSV;
  * CSV writer — fed the rows parsed from a golden CSV it reproduces the file byte for byte;
  * batching — with a fake solver no batch exceeds the record capacity and every record is
    written once, in time order.
"""
import glob
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from dualsphysics_multilayer_amd._abi import GAUGE_RECORD_DTYPE
from dualsphysics_multilayer_amd.gauges import GaugeCsv, csv_name, max_batch
from dualsphysics_multilayer_amd.run import CaseRun
from dualsphysics_multilayer_amd.xmlcase import CaseError, XmlCase, swl_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GDIR = os.path.join(GOLD, "gauges")
CASES = sorted(os.path.basename(d) for d in glob.glob(os.path.join(GDIR, "*")) if os.path.isdir(d))


def load_meta(name):
    with open(os.path.join(GDIR, name, "meta.json")) as fh:
        return json.load(fh)


def case_dir(name, tmp_path, edit=None):
    """The golden case (XML with gauges + its particle file) in a directory of its own."""
    m = load_meta(name)
    d = tmp_path / name
    d.mkdir(exist_ok=True)
    with open(os.path.join(GDIR, name, m["case"] + ".xml")) as fh:
        xml = fh.read()
    (d / (m["case"] + ".xml")).write_text(edit(xml) if edit else xml)
    bi4 = os.path.join(GOLD, m["bi4"]) if m["bi4"] else os.path.join(GDIR, name, m["case"] + ".bi4")
    shutil.copy(bi4, d / (m["case"] + ".bi4"))
    return str(d / m["case"])


def load_case(name, tmp_path, edit=None):
    m = load_meta(name)
    ov = {}
    if "-symplectic" in m["options"]:
        ov["step_algorithm"] = 2
    if "-cellmode:half" in m["options"]:
        ov["cellmode"] = 2
    return XmlCase(case_dir(name, tmp_path, edit), **ov)


def read_golden(name, fn):
    with open(os.path.join(GDIR, name, fn)) as fh:
        lines = fh.read().split("\n")
    return lines[0], [ln.split(";") for ln in lines[1:] if ln]


def test_fixtures_present():
    assert CASES == ["dambreak2d_verlet", "dambreak_sym_half", "dambreak_verlet", "flume_verlet"]


def test_xml_gauges_of_the_dam_break(tmp_path):
    c = load_case("dambreak_verlet", tmp_path)
    g = {x["name"]: x for x in c.gauges}
    assert [x["name"] for x in c.gauges] == ["VelStep", "VelDt", "VelOut", "SwlV", "SwlH", "MaxZ", "Wall"]
    assert [x["type"] for x in c.gauges] == ["velocity"] * 3 + ["swl"] * 2 + ["maxz", "force"]
    # <default>: every step, output on, 0..10 s; VelDt / SwlH override one value each
    for x in c.gauges:
        assert (x["computestart"], x["computeend"], x["outputstart"], x["outputend"], x["output"]) == (0, 10, 0, 10, True)
    assert [x["computedt"] for x in c.gauges] == [0, 0.002, 0, 0, 0, 0, 0]
    assert [x["outputdt"] for x in c.gauges] == [0, 0, 0, 0, 0.003, 0, 0]
    assert g["VelDt"]["point0"] == [0.33, 0.12, 0.26]
    # JGaugeSwl::SetPoints: 0.38 m every 0.025 m -> 15.2 -> 16 intervals of 0.02375 m
    assert g["SwlV"]["pointnp"] == 16 and g["SwlV"]["pointdp"] == 0.025
    assert g["SwlV"]["pointdir"] == pytest.approx([0, 0, 0.38 / 16], abs=1e-16)
    assert g["SwlH"]["pointnp"] == 36 and g["SwlH"]["pointdir"] == pytest.approx([0.025, 0, 0], abs=1e-16)
    # MassLimit = 0.5 massfluid (3-D default and coef), in float
    assert g["SwlV"]["masslimit"] == g["SwlH"]["masslimit"] == float(np.float32(0.125) * np.float32(0.5))
    assert g["MaxZ"]["distlimit"] == float(np.float32(0.05 * float(np.float32(0.9))))
    assert g["MaxZ"]["height"] == float(np.float32(0.4)) and g["MaxZ"]["point0"] == [0.3, 0.335, 0.0]
    assert (g["Wall"]["mkbound"], g["Wall"]["code"], g["Wall"]["idbegin"], g["Wall"]["count"]) == (0, 0, 0, 1182)
    assert not c.explicit_codes


def test_xml_defaults_without_default_block(tmp_path):
    """No <default>: computedt = outputdt = TimeOut, 0 .. TimeMax, output off; 2-D MassLimit 0.4 massfluid."""
    def edit(x):
        i, j = x.index("<default>"), x.index("</default>") + len("</default>")
        return x[:i] + x[j:]
    c = load_case("dambreak2d_verlet", tmp_path, edit)
    for x in c.gauges:
        assert (x["computedt"], x["outputdt"], x["computestart"], x["computeend"], x["output"]) == (
            c.timeout, c.timeout, 0.0, c.timemax, False)
    swl = [x for x in c.gauges if x["type"] == "swl"][0]
    assert swl["masslimit"] == float(np.float32(c.massfluid) * np.float32(0.4))


def test_xml_force_targets_of_the_flume(tmp_path):
    c = load_case("flume_verlet", tmp_path)
    g = {x["name"]: x for x in c.gauges}
    assert (g["Piston"]["code"], g["Piston"]["idbegin"], g["Piston"]["count"]) == (0x800, 2205, 176)
    assert (g["Flap"]["code"], g["Flap"]["idbegin"], g["Flap"]["count"]) == (0x801, 2381, 176)


def test_swl_points():
    assert swl_points([0, 0, 0], [0, 0, 1.0], 0.3) == (4, [0.0, 0.0, 0.25])  # 3.33: remainder >= 10 % -> 4
    assert swl_points([0, 0, 0], [1.02, 0, 0], 0.5)[0] == 2                     # 0.02 < 0.05: stays 2
    assert swl_points([0, 0, 0], [0.1, 0, 0], 0.5)[0] == 1
    assert swl_points([1, 1, 1], [1, 1, 1], 0.5) == (0, [0.0, 0.0, 0.0])


@pytest.mark.parametrize("edit,match", [
    (lambda x: x.replace('<velocity name="VelDt">', '<velocity name="VelStep">'), "already exists"),
    (lambda x: x.replace("<maxz ", "<pressure ").replace("</maxz>", "</pressure>"), "is invalid"),
    (lambda x: x.replace('<target mkbound="0"/>', '<target mkbound="7"/>'), "unknown"),
    (lambda x: x.replace('<masslimit coef="0.5"/>', '<masslimit coef="0.5" value="1"/>'), "only one"),
    (lambda x: x.replace('<masslimit coef="0.5"/>', '<masslimit coef="-1"/>'), "masslimit"),
    (lambda x: x.replace('<distlimit coefdp="0.9"/>', ''), "distlimit"),
    (lambda x: x.replace('<point x="0.2" y="0.3" z="0.15"/>', ''), "point"),
    (lambda x: x.replace("</gauges>", "</gauges>\n<wavepaddles/>"), "wavepaddles"),
])
def test_xml_errors_raise(tmp_path, edit, match):
    with pytest.raises(CaseError, match=match):
        load_case("dambreak_verlet", tmp_path, edit)


def test_xml_force_on_a_floating_block_is_refused(tmp_path):
    with pytest.raises(CaseError, match="Only fixed or moving"):
        load_case("flume_verlet", tmp_path, lambda x: x.replace('<target mkbound="2"/>', '<target mkbound="3"/>'))


def test_xml_inactive_and_underscore_elements_are_skipped(tmp_path):
    c = load_case("dambreak_verlet", tmp_path, lambda x: x.replace('<maxz name="MaxZ">', '<maxz name="MaxZ" active="false">'))
    assert [x["name"] for x in c.gauges] == ["VelStep", "VelDt", "VelOut", "SwlV", "SwlH", "Wall"]


# ---- schedule ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sched_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sched") / "gauge_sched_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "gauge_sched_host.cpp"),
                           "-o", exe])
    return exe


@pytest.mark.parametrize("name", CASES)
def test_schedule_selects_the_golden_rows(name, sched_exe, tmp_path):
    c, m = load_case(name, tmp_path), load_meta(name)
    times = m["times"]
    assert len(times) == m["nsteps"] + 1 and times[0] == 0.0
    text = "%d %d\n" % (len(c.gauges), len(times))
    for g in c.gauges:
        text += " ".join(float(g[k]).hex() for k in ("computestart", "computeend", "computedt")) + " %d " % g["output"]
        text += " ".join(float(g[k]).hex() for k in ("outputstart", "outputend", "outputdt")) + "\n"
    text += "\n".join(float(t).hex() for t in times) + "\n"
    out = subprocess.run([sched_exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    for gi, g in enumerate(c.gauges):
        picked = ["%f" % times[int(k)] for k in out[gi].split()]
        _, rows = read_golden(name, csv_name(g))
        assert picked == [r[0] for r in rows], g["name"]


# ---- CSV writer ------------------------------------------------------------------------------
def records_of_golden(name, gauges):
    """The golden rows as the records the core would deliver (time, gauge, v[3]) in time order."""
    recs = []
    for gi, g in enumerate(gauges):
        _, rows = read_golden(name, csv_name(g))
        for r in rows:
            v = [float(x) for x in r[1:]]
            val = {"velocity": v[0:3], "swl": v[0:3], "maxz": [v[0], 0, 0], "force": v[1:4]}[g["type"]]
            recs.append((float(r[0]), gi, val))
    recs.sort(key=lambda r: (r[0], r[1]))
    return np.array([(t, gi, tuple(v)) for t, gi, v in recs], GAUGE_RECORD_DTYPE)


@pytest.mark.parametrize("name", CASES)
def test_csv_writer_reproduces_the_golden_files(name, tmp_path):
    c = load_case(name, tmp_path)
    recs = records_of_golden(name, c.gauges)
    out = tmp_path / "out"
    out.mkdir()
    w = GaugeCsv(c.gauges, str(out))
    for part in np.array_split(recs, 7):  # appended over several flushes, as at every PART
        w.add(part)
        w.flush()
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GDIR, name, "Gauges*.csv")))
    assert sorted(os.listdir(out)) == files
    for fn in files:
        with open(os.path.join(GDIR, name, fn), "rb") as a, open(out / fn, "rb") as b:
            gold, mine = a.read(), b.read()
        if not fn.startswith("GaugesForce"):
            assert gold == mine, fn
            continue
        # A force row prints |F| of the unrounded components, which its own 6-digit components
        # do not determine to the last digit: each is off by <= half a unit of its sixth digit,
        # so |F| recomputed from them is off by <= sqrt(3)/2 (< 1) units of the sixth digit of
        # the largest component (whose quantum is <= that of |F|).  Everything else is bytewise.
        la, lb = gold.decode().split("\n"), mine.decode().split("\n")
        assert len(la) == len(lb) and la[0] == lb[0], fn
        for x, y in zip(la[1:], lb[1:]):
            if x == y:
                continue
            cx, cy = x.split(";"), y.split(";")
            assert cx[:1] + cx[2:] == cy[:1] + cy[2:], (fn, x, y)
            quantum = 10.0 ** (np.floor(np.log10(float(cx[1]))) - 5)
            assert abs(float(cx[1]) - float(cy[1])) <= 1.001 * quantum, (fn, x, y)


def test_csv_force_magnitude_is_float_pointdist(tmp_path):
    """|F| = fgeo::PointDist of the float components (second column), printed as %g."""
    g = [dict(name="F", type="force", output=True)]
    w = GaugeCsv(g, str(tmp_path))
    w.add(np.array([(0.0005049, 0, (3.0, -4.0, 12.0)), (0.25, 0, (1e-3, 2e-3, -2e-3))], GAUGE_RECORD_DTYPE))
    w.flush()
    with open(tmp_path / "GaugesForce_F.csv") as fh:
        assert fh.read() == ("time [s];force [N];forcex [N];forcey [N];forcez [N]\n"
                             "0.000505;13;3;-4;12\n0.250000;0.003;0.001;0.002;-0.002\n")


# ---- batching ----------------------------------------------------------------------------------
class FakeSolver:
    """Steps of a fixed dt; every step stores one record per gauge with output (like the
    every-step gauges), in a buffer of `capacity` records that must never overflow."""

    def __init__(self, dt):
        self.dt, self.t, self.nstep = dt, 0.0, 0
        self.buf, self.batches, self.highwater = [], [], 0

    def set_gauges(self, gauges, capacity):
        self.gauges, self.capacity = gauges, capacity
        self._store()

    def _store(self):
        for gi, g in enumerate(self.gauges):
            if g["output"]:
                assert len(self.buf) < self.capacity, "gauge record buffer overflow"
                self.buf.append((self.t, gi, (float(self.nstep), 0.0, 0.0)))
        self.highwater = max(self.highwater, len(self.buf))

    def run(self, n):
        self.batches.append(n)
        for _ in range(n):
            self.t += self.dt
            self.nstep += 1
            self._store()

    Run = run

    def stats(self):
        return dict(time=self.t, nstep=self.nstep, np=1758, npb=1182, npbok=1182, nout=0, error_flags=0,
                    sym_dtpre=self.dt)

    def gauge_records(self):
        out, self.buf = np.array(self.buf, GAUGE_RECORD_DTYPE), []
        return out

    def close(self):
        pass


@pytest.mark.parametrize("capacity", [7, 25, 1 << 16])
def test_batches_fit_the_record_buffer(tmp_path, capacity):
    c = load_case("dambreak_verlet", tmp_path)
    c.timemax, c.timeout = 0.02, 0.01  # two output intervals of ~40 steps each
    nout = sum(1 for g in c.gauges if g["output"])
    assert nout == 7 and max_batch(capacity, c.gauges) == capacity // 7
    fake = FakeSolver(dt=c.dt_cap() * 0.5)
    out = tmp_path / "out"
    r = CaseRun(c, str(out), save=False, log=lambda s: None, gauge_capacity=capacity, solver=fake)
    r.run()
    assert max(fake.batches) <= capacity // nout and fake.highwater <= capacity
    if capacity >= 1 << 16:
        assert max(fake.batches) > 1  # a large buffer does not limit the batches
    assert not fake.buf  # everything drained
    for gi, g in enumerate(c.gauges):
        with open(out / csv_name(g)) as fh:
            rows = [ln.split(";") for ln in fh.read().split("\n")[1:] if ln]
        col = {"velocity": 1, "swl": 1, "maxz": 1, "force": 2}[g["type"]]
        # every step's record once, in step (= time) order
        assert [int(float(x[col])) for x in rows] == list(range(fake.nstep + 1)), g["name"]
        assert [float(x[0]) for x in rows] == sorted(float(x[0]) for x in rows)


def test_buffer_smaller_than_one_step_is_refused():
    with pytest.raises(ValueError, match="smaller than one step"):
        max_batch(3, [dict(output=True)] * 4)
    assert max_batch(3, [dict(output=False)] * 4) >= 1 << 30
