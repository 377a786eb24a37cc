"""ctypes mirror of the POD structs in include/sphcore.h (ABI version: SPH_ABI_VERSION below)."""
from __future__ import annotations

import ctypes as C

import numpy as np

SPH_ABI_VERSION = 18

SPH_STATUS = {
    0: "SPH_OK",
    1: "SPH_ERR_ARG",
    2: "SPH_ERR_HIP",
    3: "SPH_ERR_STATE",
    4: "SPH_ERR_DT",
    5: "SPH_ERR_BOUNDOUT",
    6: "SPH_ERR_NOMEM",
    7: "SPH_ERR_UNSUPPORTED",
    8: "SPH_ERR_COMM",
}


SPH_BOUND_DBC, SPH_BOUND_MDBC = 1, 2
SPH_SLIP_VEL0, SPH_SLIP_NOSLIP, SPH_SLIP_FREESLIP = 1, 2, 3
SPH_RHEOLOGY_SINGLE, SPH_RHEOLOGY_NN = 1, 2
SPH_VELGRAD_FDA, SPH_VELGRAD_SPH = 1, 2
SPH_VISCO_ARTIFICIAL, SPH_VISCO_LAMINARSPS, SPH_VISCO_CONSTEQ = 1, 2, 3
SPH_SHIFT_NONE, SPH_SHIFT_NOBOUND, SPH_SHIFT_NOFIXED, SPH_SHIFT_FULL = 0, 1, 2, 3
SPH_MAXPHASES = 8
_CASEDEF_DEFAULTS = {"tboundary": SPH_BOUND_DBC, "slipmode": SPH_SLIP_VEL0, "mdbc_threshold": 0.0,
                     "rheology": SPH_RHEOLOGY_SINGLE, "velgrad": SPH_VELGRAD_FDA, "tvisco": SPH_VISCO_ARTIFICIAL,
                     "nphases": 0, "relaxation_dt": 0.2, "shift_mode": SPH_SHIFT_NONE, "mdbc_corrector": 0,
                     "shift_coef": -2.0, "shift_tfs": 0.0, "phases": (),
                     "data2d": 0, "pad2d": 0, "data2d_posy": 0.0, "dtallparticles": 0, "symmetry": 0,
                     "dtfixed": 0.0,
                     "peri_active": 0, "pad_peri": 0, "peri_xinc": (0.0, 0.0, 0.0), "peri_yinc": (0.0, 0.0, 0.0),
                     "peri_zinc": (0.0, 0.0, 0.0)}
SPH_TTAB_DTFIXED, SPH_TTAB_VISCO = 0, 1
SPH_FTMODE_NONE, SPH_FTMODE_SPH, SPH_FTMODE_EXT = 0, 1, 2  # TpFtMode (RigidAlgorithm 1 -> SPH, 0 and 2 -> EXT)


class SphPhaseDef(C.Structure):
    """One <nnphases><phase> (JSph::InitMultiPhase, JSph.cpp:3137-3215)."""
    _fields_ = [
        ("mkfluid", C.c_int32),
        ("phasetype", C.c_int32),
        ("rho", C.c_double),
        ("cs0", C.c_double),
        ("gamma", C.c_double),
        ("visco", C.c_double),
        ("tau_yield", C.c_double),
        ("tau_max", C.c_double),
        ("bi_multi", C.c_double),
        ("hbp_m", C.c_double),
        ("hbp_n", C.c_double),
    ]


class SphCaseDef(C.Structure):
    _fields_ = [
        ("dp", C.c_double),
        ("h", C.c_double),
        ("cteb", C.c_double),
        ("rhop0", C.c_double),
        ("gamma", C.c_double),
        ("massbound", C.c_double),
        ("massfluid", C.c_double),
        ("gravity", C.c_double * 3),
        ("cflnumber", C.c_double),
        ("step_algorithm", C.c_int),
        ("verlet_steps", C.c_int),
        ("kernel", C.c_int),
        ("tdensity", C.c_int),
        ("visco", C.c_double),
        ("viscoboundfactor", C.c_double),
        ("ddtvalue", C.c_double),
        ("coefdtmin", C.c_double),
        ("dtini", C.c_double),
        ("dtmin", C.c_double),
        ("rhopoutmin", C.c_double),
        ("rhopoutmax", C.c_double),
        ("map_realposmin", C.c_double * 3),
        ("map_realposmax", C.c_double * 3),
        ("cellmode", C.c_int),
        ("celldomfixed", C.c_int),
        ("npb", C.c_uint32),
        ("np", C.c_uint32),
        ("tboundary", C.c_int32),
        ("slipmode", C.c_int32),
        ("mdbc_threshold", C.c_double),
        ("rheology", C.c_int32),
        ("velgrad", C.c_int32),
        ("tvisco", C.c_int32),
        ("nphases", C.c_uint32),
        ("relaxation_dt", C.c_double),
        ("shift_mode", C.c_int32),
        ("mdbc_corrector", C.c_int32),
        ("shift_coef", C.c_double),
        ("shift_tfs", C.c_double),
        ("phases", SphPhaseDef * SPH_MAXPHASES),
        ("data2d", C.c_int32),
        ("pad2d", C.c_int32),
        ("data2d_posy", C.c_double),
        ("dtallparticles", C.c_int32),
        ("symmetry", C.c_int32),
        ("dtfixed", C.c_double),
        # periodic boundaries: PeriActive bits (1 X, 2 Y, 4 Z) and the XML's offsets
        ("peri_active", C.c_int32),
        ("pad_peri", C.c_int32),
        ("peri_xinc", C.c_double * 3),
        ("peri_yinc", C.c_double * 3),
        ("peri_zinc", C.c_double * 3),
    ]

    @classmethod
    def from_dict(cls, d: dict) -> "SphCaseDef":
        s = cls()
        for name, ctype in cls._fields_:
            if name not in d and name in _CASEDEF_DEFAULTS:
                v = _CASEDEF_DEFAULTS[name]
            else:
                v = d[name]
            if name == "phases":
                if len(v) > SPH_MAXPHASES:
                    raise ValueError("at most %d phases" % SPH_MAXPHASES)
                for i, ph in enumerate(v):
                    for k, x in ph.items():
                        setattr(s.phases[i], k, x)
                continue
            if isinstance(v, (tuple, list)):
                arr = getattr(s, name)
                for i, x in enumerate(v):
                    arr[i] = x
            else:
                setattr(s, name, v)
        return s


class SphConstants(C.Structure):
    _fields_ = [
        ("kernelh", C.c_float),
        ("kernelsize", C.c_float),
        ("kernelsize2", C.c_float),
        ("awen", C.c_float),
        ("bwen", C.c_float),
        ("cteb", C.c_float),
        ("gamma", C.c_float),
        ("rhopzero", C.c_float),
        ("ovrhopzero", C.c_float),
        ("massfluid", C.c_float),
        ("massbound", C.c_float),
        ("gravity", C.c_float * 3),
        ("eta2", C.c_float),
        ("ddtkh", C.c_float),
        ("ddtgz", C.c_float),
        ("visco", C.c_float),
        ("viscoboundfactor", C.c_float),
        ("rhopoutmin", C.c_float),
        ("rhopoutmax", C.c_float),
        ("scell", C.c_float),
        ("movlimit", C.c_float),
        ("pad0", C.c_float),
        ("cs0", C.c_double),
        ("cflnumber", C.c_double),
        ("dtini", C.c_double),
        ("dtmin", C.c_double),
        ("dp", C.c_double),
        ("tdensity", C.c_int),
        ("step_algorithm", C.c_int),
        ("verlet_steps", C.c_int),
        ("scelldiv", C.c_int),
        ("map_realposmin", C.c_double * 3),
        ("map_realsize", C.c_double * 3),
        ("dom_posmin", C.c_double * 3),
        ("dom_cells", C.c_uint32 * 3),
        ("dom_cellcode", C.c_uint32),
        ("tboundary", C.c_int32),
        ("slipmode", C.c_int32),
        ("mdbc_threshold", C.c_float),
        ("pad1", C.c_uint32),
        ("rheology", C.c_int32),
        ("velgrad", C.c_int32),
        ("tvisco", C.c_int32),
        ("shift_mode", C.c_int32),
        ("nphases", C.c_uint32),
        ("relaxation_dt", C.c_float),
        ("shift_coef", C.c_float),
        ("shift_tfs", C.c_float),
        ("phase_mass", C.c_float * SPH_MAXPHASES),
        ("phase_cteb", C.c_float * SPH_MAXPHASES),
        ("data2d", C.c_int32),
        ("pad3", C.c_int32),
        ("spssmag", C.c_float),
        ("spsblin", C.c_float),
        ("kernel", C.c_int32),
        ("cub_a1", C.c_float),
        ("cub_a2", C.c_float),
        ("cub_aa", C.c_float),
        ("cub_a24", C.c_float),
        ("cub_c1", C.c_float),
        ("cub_d1", C.c_float),
        ("cub_c2", C.c_float),
        ("cub_od_wdeltap", C.c_float),
        ("pad4", C.c_int32),
        ("dtallparticles", C.c_int32),
        ("symmetry", C.c_int32),
        ("dtfixed", C.c_double),
        ("peri_active", C.c_int32),
        ("pad5", C.c_int32),
        ("peri_xinc", C.c_double * 3),
        ("peri_yinc", C.c_double * 3),
        ("peri_zinc", C.c_double * 3),
        ("map_posmin", C.c_double * 3),
        ("map_posmax", C.c_double * 3),
    ]

    def as_dict(self) -> dict:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out


class SphRunStats(C.Structure):
    _fields_ = [
        ("time", C.c_double),
        ("last_dt", C.c_double),
        ("sym_dtpre", C.c_double),
        ("nstep", C.c_uint64),
        ("np", C.c_uint32),
        ("npb", C.c_uint32),
        ("npbok", C.c_uint32),
        ("nout", C.c_uint32),
        ("dtmodif", C.c_uint32),
        ("error_flags", C.c_uint32),
        ("velmax", C.c_float),
        ("acemax", C.c_float),
        ("viscdtmax", C.c_float),
        ("viscetadtmax", C.c_float),
        ("fused_updates", C.c_uint64),
        ("npbper", C.c_uint32),
        ("npfper", C.c_uint32),
        ("dem_dtforce", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class SphParticlesHost(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("idp", C.POINTER(C.c_uint32)),
        ("pos", C.POINTER(C.c_double)),
        ("vel", C.POINTER(C.c_float)),
        ("rhop", C.POINTER(C.c_float)),
        ("code", C.POINTER(C.c_uint16)),
        ("boundnormal", C.POINTER(C.c_float)),
    ]


class SphInterOut(C.Structure):
    _fields_ = [
        ("ar", C.POINTER(C.c_float)),
        ("ace", C.POINTER(C.c_float)),
        ("viscdtmax", C.c_float),
        ("velmax", C.c_float),
        ("acemax", C.c_float),
    ]


class SphExtOut(C.Structure):
    _fields_ = [
        ("shiftposfs", C.POINTER(C.c_float)),
        ("tau", C.POINTER(C.c_float)),
    ]


class SphSlabDef(C.Structure):
    _fields_ = [
        ("rank", C.c_int32),
        ("nranks", C.c_int32),
        ("cx_begin", C.c_int32),
        ("cx_end", C.c_int32),
        ("axis", C.c_int32),
        ("pad", C.c_int32),
        ("comm_id", C.c_ubyte * 128),
    ]


class SphSlabInfo(C.Structure):
    _fields_ = [
        ("rank", C.c_int32),
        ("nranks", C.c_int32),
        ("cx_begin", C.c_int32),
        ("cx_end", C.c_int32),
        ("repartitions", C.c_uint32),
        ("axis", C.c_int32),
        ("last_imbalance", C.c_double),
    ]


class SphPartHeader(C.Structure):
    _fields_ = [
        ("app_name", C.c_char * 64),
        ("case_name", C.c_char * 64),
        ("cpart", C.c_uint32),
        ("npok", C.c_uint32),
        ("nout", C.c_uint32),
        ("step", C.c_uint32),
        ("timestep", C.c_double),
        ("runtime", C.c_double),
        ("domain_min", C.c_double * 3),
        ("domain_max", C.c_double * 3),
        ("symplectic_dtpre", C.c_double),
        ("np_total", C.c_uint64),
        ("case_np", C.c_uint64),
        ("case_nfixed", C.c_uint64),
        ("case_nmoving", C.c_uint64),
        ("case_nfloat", C.c_uint64),
        ("case_nfluid", C.c_uint64),
        ("dp", C.c_double),
        ("h", C.c_double),
        ("b", C.c_double),
        ("rhop0", C.c_double),
        ("gamma", C.c_double),
        ("massbound", C.c_double),
        ("massfluid", C.c_double),
        ("map_posmin", C.c_double * 3),
        ("map_posmax", C.c_double * 3),
        ("case_posmin", C.c_double * 3),
        ("case_posmax", C.c_double * 3),
        ("peri_xinc", C.c_double * 3),
        ("peri_yinc", C.c_double * 3),
        ("peri_zinc", C.c_double * 3),
        ("data2d_posy", C.c_double),
        ("data2d", C.c_int32),
        ("peri_mode", C.c_int32),
        ("axis_div", C.c_int32),
        ("np_dynamic", C.c_int32),
        ("reuse_ids", C.c_int32),
        ("symmetry", C.c_int32),
        ("splitting", C.c_int32),
        ("pos_double", C.c_int32),
        ("visco_type", C.c_int32),
        ("visco", C.c_float),
        ("viscoboundfactor", C.c_float),
        ("gravity", C.c_float * 3),
        ("mkbound", C.c_uint32),
        ("mkfluid", C.c_uint32),
        ("dem_dtforce", C.c_double),
    ]

    def as_dict(self) -> dict:
        d = {}
        for name, t in self._fields_:
            v = getattr(self, name)
            if isinstance(v, bytes):
                v = v.decode()
            elif hasattr(v, "__len__"):
                v = list(v)
            d[name] = v
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "SphPartHeader":
        h = cls()
        for name, t in cls._fields_:
            if name not in d:
                continue
            v = d[name]
            if isinstance(v, str):
                v = v.encode()
            if hasattr(getattr(h, name), "__len__") and not isinstance(v, bytes):
                arr = getattr(h, name)
                for i, x in enumerate(v):
                    arr[i] = x
            else:
                setattr(h, name, v)
        return h


def _ptr(arr: np.ndarray | None, ctype):
    if arr is None:
        return C.POINTER(ctype)()
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(C.POINTER(ctype))


class SphMotionMov(C.Structure):
    _fields_ = [
        ("obj", C.c_int32), ("id", C.c_int32), ("next", C.c_int32), ("type", C.c_int32), ("prev", C.c_int32),
        ("fields", C.c_int32), ("data_first", C.c_uint32), ("data_n", C.c_uint32), ("duration", C.c_double),
        ("vec", C.c_double * 3), ("vec2", C.c_double * 3), ("phase", C.c_double * 3), ("axisp1", C.c_double * 3),
        ("axisp2", C.c_double * 3), ("ref", C.c_double * 3), ("ang", C.c_double), ("ang2", C.c_double),
        ("ang3", C.c_double),
    ]


class SphMotionObj(C.Structure):
    _fields_ = [("parent", C.c_int32), ("ref", C.c_int32)]


class SphMotionEvent(C.Structure):
    _fields_ = [("obj", C.c_int32), ("mov", C.c_int32), ("start", C.c_double), ("finish", C.c_double)]


class SphFloatingDef(C.Structure):
    _fields_ = [
        ("idbegin", C.c_uint32), ("count", C.c_uint32), ("massbody", C.c_double), ("masspart", C.c_double),
        ("center", C.c_double * 3), ("inertia", C.c_double * 9), ("linvelini", C.c_double * 3),
        ("angvelini", C.c_double * 3), ("translationfree", C.c_int32 * 3), ("rotationfree", C.c_int32 * 3),
    ]


class SphFloatingState(C.Structure):
    _fields_ = [
        ("center", C.c_double * 3), ("fvel", C.c_float * 3), ("fomega", C.c_float * 3), ("angles", C.c_float * 3),
        ("facelin", C.c_float * 3), ("faceang", C.c_float * 3), ("pad", C.c_float),
    ]

    def as_dict(self) -> dict:
        return {k: np.array(getattr(self, k)) for k in ("center", "fvel", "fomega", "angles", "facelin", "faceang")}


SPH_GAUGE_VEL, SPH_GAUGE_SWL, SPH_GAUGE_MAXZ, SPH_GAUGE_FORCE = 0, 1, 2, 3
GAUGE_TYPES = {"velocity": SPH_GAUGE_VEL, "swl": SPH_GAUGE_SWL, "maxz": SPH_GAUGE_MAXZ, "force": SPH_GAUGE_FORCE}
SPH_FLAG_GAUGE_FULL = 64
SPH_FLAG_PERIODIC_FULL = 128


class SphGaugeDef(C.Structure):
    _fields_ = [
        ("type", C.c_int32), ("output", C.c_int32),
        ("computestart", C.c_double), ("computeend", C.c_double), ("computedt", C.c_double),
        ("outputstart", C.c_double), ("outputend", C.c_double), ("outputdt", C.c_double),
        ("point0", C.c_double * 3), ("point2", C.c_double * 3), ("pointdir", C.c_double * 3),
        ("height", C.c_double), ("pointnp", C.c_uint32), ("masslimit", C.c_float), ("distlimit", C.c_float),
        ("code", C.c_uint32),
    ]


class SphGaugeRecord(C.Structure):
    _fields_ = [("time", C.c_double), ("gauge", C.c_uint32), ("v", C.c_float * 3)]


# numpy view of SphGaugeRecord[]
GAUGE_RECORD_DTYPE = np.dtype([("time", np.float64), ("gauge", np.uint32), ("v", np.float32, 3)])


def gauge_array(gauges: list):
    """SphGaugeDef[] of a case's gauges (XmlCase.gauges: dicts with the struct's fields; type by name)."""
    arr = (SphGaugeDef * max(1, len(gauges)))()
    for i, g in enumerate(gauges):
        _fill(arr[i], {k: v for k, v in g.items() if k != "type"})
        arr[i].type = GAUGE_TYPES[g["type"]]
        arr[i].output = int(bool(g.get("output", False)))
    return arr


SPH_MAX_ACCINPUTS = SPH_MAX_DAMPINGS = 16
SPH_DAMP_PLANE, SPH_DAMP_BOX, SPH_DAMP_CYLINDER = 0, 1, 2
DAMP_TYPES = {"plane": SPH_DAMP_PLANE, "box": SPH_DAMP_BOX, "cylinder": SPH_DAMP_CYLINDER}
# JDsDampingOp_Box::TpDirections (JDsDamping.h:169-179)
DAMP_DIRS = {"top": 1, "bottom": 2, "left": 4, "right": 8, "front": 16, "back": 32, "all": 63}


class SphAccInputDef(C.Structure):
    _fields_ = [
        ("code1", C.c_uint32), ("code2", C.c_uint32), ("globalgravity", C.c_int32),
        ("row0", C.c_uint32), ("nrows", C.c_uint32), ("pad", C.c_uint32),
        ("timestart", C.c_double), ("timeend", C.c_double), ("centre", C.c_double * 3),
    ]


class SphDampingDef(C.Structure):
    _fields_ = [
        ("type", C.c_int32), ("usedomain", C.c_int32), ("directions", C.c_uint32),
        ("overlimit", C.c_float), ("redumax", C.c_float), ("factorxyz", C.c_float * 3),
        ("pt", (C.c_double * 3) * 4), ("dompt", (C.c_double * 2) * 4),
        ("domzmin", C.c_double), ("domzmax", C.c_double), ("radmin", C.c_double), ("radmax", C.c_double),
    ]


class SphDampingDerived(C.Structure):
    _fields_ = [
        ("plane", C.c_double * 4), ("dompla", (C.c_double * 4) * 4),
        ("limitmin1", C.c_double * 3), ("limitmin2", C.c_double * 3), ("limitmax1", C.c_double * 3),
        ("limitmax2", C.c_double * 3), ("limitover1", C.c_double * 3), ("limitover2", C.c_double * 3),
        ("boxsize1", C.c_double * 3), ("boxsize2", C.c_double * 3),
        ("axislen", C.c_double), ("dist", C.c_float), ("vertical", C.c_int32),
    ]

    def as_dict(self) -> dict:
        return {k: np.array(getattr(self, k)) if isinstance(getattr(self, k), C.Array) else getattr(self, k)
                for k, _ in self._fields_}


def accinput_arrays(accinputs: list):
    """SphAccInputDef[] and the rows (float64 [n][7]: time, linx, liny, linz, angx, angy, angz) of
    XmlCase.accinputs: dicts with code1, code2, globalgravity, timestart, timeend, centre, rows."""
    arr = (SphAccInputDef * max(1, len(accinputs)))()
    rows = []
    n = 0
    for i, a in enumerate(accinputs):
        r = np.asarray(a["rows"], np.float64).reshape(-1, 7)
        arr[i].code1, arr[i].code2 = int(a["code1"]), int(a["code2"])
        arr[i].globalgravity = int(bool(a["globalgravity"]))
        arr[i].row0, arr[i].nrows = n, len(r)
        arr[i].timestart, arr[i].timeend = float(a["timestart"]), float(a["timeend"])
        for k in range(3):
            arr[i].centre[k] = float(a["centre"][k])
        rows.append(r)
        n += len(r)
    allrows = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 7)), np.float64)
    return arr, allrows


def damping_array(damping: list):
    """SphDampingDef[] of XmlCase.damping: dicts with type ("plane", "box", "cylinder"), overlimit,
    redumax, factorxyz and, per type, plane: limitmin, limitmax (+ dompt [4][2], domzmin, domzmax);
    box: directions (DAMP_DIRS bits), limitmin_ini / _end, limitmax_ini / _end; cylinder: point1,
    point2, radmin, radmax."""
    arr = (SphDampingDef * max(1, len(damping)))()
    for i, d in enumerate(damping):
        z = arr[i]
        z.type = DAMP_TYPES[d["type"]]
        z.overlimit, z.redumax = float(d["overlimit"]), float(d.get("redumax", 10.0))
        for k, v in enumerate(d.get("factorxyz", (1.0, 1.0, 1.0))):
            z.factorxyz[k] = float(v)
        pts = {"plane": ("limitmin", "limitmax"), "box": ("limitmin_ini", "limitmin_end", "limitmax_ini", "limitmax_end"),
               "cylinder": ("point1", "point2")}[d["type"]]
        for j, key in enumerate(pts):
            for k in range(3):
                z.pt[j][k] = float(d[key][k])
        if d["type"] == "plane" and d.get("dompt") is not None:
            z.usedomain = 1
            for j in range(4):
                z.dompt[j][0], z.dompt[j][1] = float(d["dompt"][j][0]), float(d["dompt"][j][1])
            z.domzmin, z.domzmax = float(d["domzmin"]), float(d["domzmax"])
        if d["type"] == "box":
            z.directions = int(d.get("directions", 63))
        if d["type"] == "cylinder":
            z.radmin, z.radmax = float(d["radmin"]), float(d["radmax"])
    return arr


def _fill(struct, d: dict):
    for k, v in d.items():
        if k not in dict(struct._fields_):
            continue
        f = getattr(struct, k)
        if isinstance(f, C.Array):
            for i, x in enumerate(v):
                f[i] = x
        else:
            setattr(struct, k, v)
    return struct


def motion_arrays(motion: dict):
    """SphMotionMov[] / SphMotionEvent[] of a case's motion program (XmlCase.motion)."""
    movs = (SphMotionMov * max(1, len(motion["movs"])))()
    for i, m in enumerate(motion["movs"]):
        _fill(movs[i], m)
    evts = (SphMotionEvent * max(1, len(motion["evts"])))()
    for i, e in enumerate(motion["evts"]):
        _fill(evts[i], e)
    return movs, evts


def motion_tree_arrays(motion: dict):
    """The tree form (motion["objs"]: nodes depth first with parent / ref; movement and event
    `obj` are node indices; motion["rows"]: the file movements' table rows, 4 doubles each):
    SphMotionObj[], SphMotionMov[], SphMotionEvent[], the rows (float64, C order)."""
    nodes = (SphMotionObj * len(motion["objs"]))()
    for i, o in enumerate(motion["objs"]):
        nodes[i].parent, nodes[i].ref = int(o["parent"]), int(o["ref"])
    movs, evts = motion_arrays(motion)
    rows = np.ascontiguousarray(np.asarray(motion.get("rows", np.zeros((0, 4))), np.float64).reshape(-1, 4))
    return nodes, movs, evts, rows


def floating_array(floatings: list):
    arr = (SphFloatingDef * len(floatings))()
    for i, f in enumerate(floatings):
        _fill(arr[i], f)
    return arr


class SphDemDef(C.Structure):
    """StDemData of one boundary block (JSph::LoadDemData), by its particle code."""
    _fields_ = [
        ("code", C.c_uint32),
        ("mass", C.c_float),
        ("massp", C.c_float),
        ("tau", C.c_float),
        ("kfric", C.c_float),
        ("restitu", C.c_float),
    ]


def dem_array(demdata: list):
    arr = (SphDemDef * max(1, len(demdata)))()
    for i, d in enumerate(demdata):
        for name, _ in SphDemDef._fields_:
            setattr(arr[i], name, d[name])
    return arr


class HostParticles:
    """Owns numpy arrays and exposes them as an SphParticlesHost view."""

    def __init__(self, n: int, idp=None, pos=None, vel=None, rhop=None, code=None, boundnormal=None):
        self.idp = np.ascontiguousarray(idp if idp is not None else np.zeros(n, np.uint32), dtype=np.uint32)
        self.pos = np.ascontiguousarray(pos if pos is not None else np.zeros((n, 3)), dtype=np.float64)
        self.vel = np.ascontiguousarray(vel if vel is not None else np.zeros((n, 3), np.float32), dtype=np.float32)
        self.rhop = np.ascontiguousarray(rhop if rhop is not None else np.zeros(n, np.float32), dtype=np.float32)
        self.code = np.ascontiguousarray(code if code is not None else np.zeros(n, np.uint16), dtype=np.uint16)
        self.boundnormal = (None if boundnormal is None
                            else np.ascontiguousarray(boundnormal, dtype=np.float32).reshape(n, 3))
        self.view = SphParticlesHost(
            n,
            _ptr(self.idp, C.c_uint32),
            _ptr(self.pos, C.c_double),
            _ptr(self.vel, C.c_float),
            _ptr(self.rhop, C.c_float),
            _ptr(self.code, C.c_uint16),
            _ptr(self.boundnormal, C.c_float),
        )

    def trimmed(self, n: int) -> dict:
        return dict(
            idp=self.idp[:n].copy(),
            pos=self.pos[:n].copy(),
            vel=self.vel[:n].copy(),
            rhop=self.rhop[:n].copy(),
            code=self.code[:n].copy(),
        )


# ---- inlet/outlet zones (sphcore.h: sph_solver_set_inout) ----------------------------------------
SPH_MAX_INOUTZONES = 16
SPH_FLAG_INOUT_FULL = 256


class SphInOutZoneDef(C.Structure):
    _fields_ = [
        ("direction", C.c_double * 3), ("plane", C.c_float * 4), ("veldata", (C.c_float * 4) * 2),
        ("boxlimitmin", C.c_float * 3), ("boxlimitmax", C.c_float * 3), ("width", C.c_float), ("zsurf", C.c_float),
        ("cfgzone", C.c_uint32), ("cfgupdate", C.c_uint32), ("layers", C.c_uint32), ("point0", C.c_uint32),
        ("npoints", C.c_uint32), ("pad", C.c_uint32),
    ]


class SphInOutDef(C.Structure):
    _fields_ = [
        ("nzones", C.c_uint32), ("useboxlimit", C.c_int32), ("extrapolatemode", C.c_int32),
        ("codenewpart", C.c_uint32), ("determlimit", C.c_float), ("freelimitmin", C.c_float * 3),
        ("freelimitmax", C.c_float * 3), ("resize_plus0", C.c_uint32), ("capacity", C.c_uint32), ("pad", C.c_uint32),
    ]


class SphInOutStats(C.Structure):
    _fields_ = [("count", C.c_uint32), ("idmax", C.c_uint32), ("capacity", C.c_uint32), ("pad", C.c_uint32),
                ("created", C.c_uint64), ("removed", C.c_uint64)]


def inout_arrays(inout: dict, capacity: int = 0):
    """(SphInOutDef, SphInOutZoneDef[], points [n][3]) of a case's zones (XmlCase.inout); capacity:
    the explicit particle capacity (0: the particles + NpResizePlus0)."""
    zones = inout["zones"]
    d = SphInOutDef()
    d.nzones = len(zones)
    d.useboxlimit = int(bool(inout["useboxlimit"]))
    d.extrapolatemode = int(inout["extrapolatemode"])
    d.codenewpart = int(inout["codenewpart"])
    d.determlimit = float(inout["determlimit"])
    for i in range(3):
        d.freelimitmin[i] = float(inout["freelimitmin"][i])
        d.freelimitmax[i] = float(inout["freelimitmax"][i])
    d.resize_plus0 = int(inout["npresizeplus0"])
    d.capacity = int(capacity)
    arr = (SphInOutZoneDef * max(1, len(zones)))()
    pts, p0 = [], 0
    for i, z in enumerate(zones):
        a = arr[i]
        for k in range(3):
            a.direction[k] = float(z["direction"][k])
            a.boxlimitmin[k] = float(z["boxlimitmin"][k])
            a.boxlimitmax[k] = float(z["boxlimitmax"][k])
        for k in range(4):
            a.plane[k] = float(z["plane"][k])
            a.veldata[0][k] = float(z["veldata"][0][k])
            a.veldata[1][k] = float(z["veldata"][1][k])
        a.width, a.zsurf = float(z["width"]), float(z["zsurf"])
        a.cfgzone, a.cfgupdate, a.layers = int(z["cfgzone"]), int(z["cfgupdate"]), int(z["layers"])
        zp = np.asarray(z["points"], np.float64)[np.asarray(z["pointsinit"], bool)]
        a.point0, a.npoints = p0, len(zp)
        p0 += len(zp)
        pts.append(zp)
    points = np.ascontiguousarray(np.concatenate(pts).reshape(-1, 3), np.float64)
    return d, arr, points


def check_struct_sizes() -> dict:
    return {
        "SphCaseDef": C.sizeof(SphCaseDef),
        "SphConstants": C.sizeof(SphConstants),
        "SphRunStats": C.sizeof(SphRunStats),
        "SphParticlesHost": C.sizeof(SphParticlesHost),
        "SphInterOut": C.sizeof(SphInterOut),
        "SphSlabDef": C.sizeof(SphSlabDef),
        "SphPartHeader": C.sizeof(SphPartHeader),
        "SphMotionMov": C.sizeof(SphMotionMov),
        "SphMotionEvent": C.sizeof(SphMotionEvent),
        "SphFloatingDef": C.sizeof(SphFloatingDef),
        "SphFloatingState": C.sizeof(SphFloatingState),
        "SphGaugeDef": C.sizeof(SphGaugeDef),
        "SphGaugeRecord": C.sizeof(SphGaugeRecord),
        "SphAccInputDef": C.sizeof(SphAccInputDef),
        "SphDampingDef": C.sizeof(SphDampingDef),
        "SphDampingDerived": C.sizeof(SphDampingDerived),
        "SphDemDef": C.sizeof(SphDemDef),
        "SphInOutZoneDef": C.sizeof(SphInOutZoneDef),
        "SphInOutDef": C.sizeof(SphInOutDef),
        "SphInOutStats": C.sizeof(SphInOutStats),
    }
