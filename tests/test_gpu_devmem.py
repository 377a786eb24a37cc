"""Replacing a device table (csrc/sph_devmem.hpp, DevArena::release).

SetTimeTable is the one place that releases an arena allocation and puts another in its
place more than once per solver.  A solver whose DtFixedFile / ViscoTime table was replaced
must run BIT FOR BIT as one that was given the final table only, and one whose table was
removed as one that never had a table.
"""
import numpy as np
import pytest

from dualsphysics_multilayer_amd._abi import SPH_TTAB_DTFIXED, SPH_TTAB_VISCO
from dualsphysics_multilayer_amd.case import DamBreakCase

pytestmark = pytest.mark.gpu

NSTEPS = 8
# rows (time s, dt ms) / (time s, Visco): the second tables have three rows and other values.
# The fixed dt lie between the case's DtMin (0.076 ms, which a smaller one is raised to) and its
# variable dt (about 0.3 ms).
TABLES = {
    SPH_TTAB_DTFIXED: ([(0.0, 0.10), (1.0, 0.10)], [(0.0, 0.080), (2e-4, 0.090), (1.0, 0.085)]),
    SPH_TTAB_VISCO: ([(0.0, 0.05), (1.0, 0.05)], [(0.0, 0.02), (1e-4, 0.03), (1.0, 0.04)]),
}


@pytest.fixture(scope="module")
def case():
    return DamBreakCase(0.03, celldomfixed=True)  # Verlet, artificial viscosity, 5,922 particles


def _run(case, *tables):
    """The state after NSTEPS of a solver given `tables` ((kind, rows) in order)."""
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    s = SphGpuSingle(case, device=0)
    for kind, rows in tables:
        s.set_time_table(kind, rows)
    s.run(NSTEPS)
    s.sync()
    assert s.stats()["error_flags"] == 0
    p = s.particles()
    return {"idp": p["idp"], "pos": p["pos"], "vel": p["vel"], "rhop": p["rhop"], "dt": s.dt_trace()}


def _assert_same(a, b, where):
    for k in ("idp", "pos", "vel", "rhop", "dt"):  # device order
        assert np.array_equal(a[k], b[k]), (where, k)


@pytest.fixture(scope="module")
def plain(case):
    return _run(case)


@pytest.mark.parametrize("kind", [SPH_TTAB_DTFIXED, SPH_TTAB_VISCO])
def test_replaced_table_runs_as_the_final_table_alone(case, kind):
    rows1, rows2 = TABLES[kind]
    a = _run(case, (kind, rows1), (kind, rows2))
    b = _run(case, (kind, rows2))
    _assert_same(a, b, "replaced")
    if kind == SPH_TTAB_DTFIXED:
        # not vacuous: the steps took the second table's dt, which the first table's run does not
        assert len(a["dt"]) and not np.array_equal(a["dt"], _run(case, (kind, rows1))["dt"])


@pytest.mark.parametrize("kind", [SPH_TTAB_DTFIXED, SPH_TTAB_VISCO])
def test_removed_table_runs_as_no_table(case, plain, kind):
    _assert_same(_run(case, (kind, TABLES[kind][0]), (kind, None)), plain, "removed")
