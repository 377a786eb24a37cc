"""Gauge output of a run: the reference's ``Gauges<Type>_<name>.csv`` files
(JGaugeVelocity/Swl/MaxZ/Force::SaveResults, JDsGaugeItem.cpp:277-298,491-513,696-717,937-959)
from the records the core takes on the device, and the batch size that keeps a batch's
records inside the device buffer.

Format (jcsv::JSaveCsv2 as the gauges configure it): ``;`` separator, the time printed as
``%f``, every other value as ``%g``, one line per stored result.
"""
from __future__ import annotations

import os

import numpy as np

TYPE_NAMES = {"velocity": "Vel", "swl": "SWL", "maxz": "MaxZ", "force": "Force"}  # JGaugeItem::GetNameType
HEADS = {
    "velocity": "time [s];velx [m/s];vely [m/s];velz [m/s];posx [m];posy [m];posz [m]",
    "swl": "time [s];swlx [m];swly [m];swlz [m];pos0x [m];pos0y [m];pos0z [m];pos2x [m];pos2y [m];pos2z [m]",
    "maxz": "time [s];zmax [m];posx [m];posy [m];posz [m]",
    "force": "time [s];force [N];forcex [N];forcey [N];forcez [N]",
}


def _g(v) -> str:
    return "%g" % float(v)


def _f3(p) -> list:
    return [_g(np.float32(c)) for c in p]  # ToTFloat3 of the configured points


def csv_name(gauge: dict) -> str:
    return "Gauges%s_%s.csv" % (TYPE_NAMES[gauge["type"]], gauge["name"])


def csv_line(gauge: dict, time: float, v) -> str:
    """One result of `gauge` (time, v[3] as the core records it) as the reference prints it."""
    t = gauge["type"]
    v = [np.float32(x) for x in v]
    out = ["%f" % time]
    if t == "velocity":
        out += [_g(x) for x in v] + _f3(gauge["point0"])
    elif t == "swl":
        out += [_g(x) for x in v] + _f3(gauge["point0"]) + _f3(gauge["point2"])
    elif t == "maxz":
        out += [_g(v[0])] + _f3(gauge["point0"])
    else:  # fgeo::PointDist(force) in float, then the components
        out += [_g(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2], dtype=np.float32))] + [_g(x) for x in v]
    return ";".join(out)


class GaugeCsv:
    """The CSV files of a case's gauges in one directory: records are held until flush()
    (the reference writes at every PART, JSph::SaveData -> JGaugeSystem::SaveResults)."""

    def __init__(self, gauges: list, dirout: str):
        self.gauges = gauges
        self.dirout = dirout
        self._pending = [[] for _ in gauges]
        self._started = [False] * len(gauges)

    def add(self, records) -> None:
        for r in records:
            gi = int(r["gauge"])
            self._pending[gi].append(csv_line(self.gauges[gi], float(r["time"]), r["v"]))

    def flush(self) -> None:
        for gi, lines in enumerate(self._pending):
            if not lines:
                continue
            path = os.path.join(self.dirout, csv_name(self.gauges[gi]))
            with open(path, "a" if self._started[gi] else "w", newline="\n") as f:
                if not self._started[gi]:
                    f.write(HEADS[self.gauges[gi]["type"]] + "\n")
                f.write("\n".join(lines) + "\n")
            self._started[gi] = True
            self._pending[gi] = []


def max_batch(capacity: int, gauges: list) -> int:
    """Most steps whose records surely fit an empty buffer of `capacity` records: every step
    stores at most one record per gauge with output."""
    per_step = sum(1 for g in gauges if g.get("output"))
    if per_step == 0:
        return 1 << 30
    if capacity < per_step:
        raise ValueError("the gauge record buffer (%d) is smaller than one step's records (%d)" % (capacity, per_step))
    return capacity // per_step
