"""The phase-level C ABI (sph_divide, sph_interaction_forces, sph_compute_dt, sph_step_verlet,
sph_step_symplectic_pre/cor) against sph_solver_run.

A host that steps phase by phase issues the reference's own sequence (ComputeStep_Ver /
ComputeStep_Sym, JSphCpuSingle.cpp:674-720) and the divide that ends a step; sph_solver_run
issues the same phases inside the library.  The two routes must give the same BITS after
every step: particle order, positions, velocities, densities, counts, TimeStep,
SymplecticDtPre and the dt trace.  Nothing here has a tolerance.

Also: a divide that follows no update changes nothing, the update phases refuse a solver
whose bodies only sph_solver_run moves, they count as a step, and the update kernel that
classifies the particles for the next divide (the default) is bitwise the separate
classification (SPH_CLS_SPLIT=1)."""
import copy

import numpy as np
import pytest

from dualsphysics_multilayer_amd.case import DamBreak2DCase, DamBreakCase, WaveFlumeCase, WetDambreakNNCase

pytestmark = pytest.mark.gpu

SYMPLECTIC = 2
STAT_KEYS = ("np", "npb", "npbok", "nout", "nstep", "time", "sym_dtpre", "error_flags")
PART_KEYS = ("idp", "pos", "vel", "rhop")


def gpu(case, monkeypatch=None, split=False):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    if split:  # read at construction
        monkeypatch.setenv("SPH_CLS_SPLIT", "1")
    s = SphGpuSingle(case, device=0)
    if split:
        monkeypatch.delenv("SPH_CLS_SPLIT")
    return s


def step_by_phases(s, n, between=None):
    """n steps through the phase calls only; `between()` runs between the Symplectic predictor's
    divide and the corrector's interaction."""
    for _ in range(n):
        if s.case.step_algorithm == SYMPLECTIC:
            s.Interaction_Forces(2)
            s.DtVariable(False)  # the predictor's
            s.ComputeSymplecticPre()
            s.RunCellDivide()
            if between:
                between()
            s.Interaction_Forces(3)
            s.DtVariable(True)  # the corrector's
            s.ComputeSymplecticCorr()
            s.RunCellDivide()
        else:
            s.Interaction_Forces(1)
            s.DtVariable(True)
            s.ComputeVerlet()
            s.RunCellDivide()


def state(s):
    st = s.stats()
    return {k: st[k] for k in STAT_KEYS}, s.particles(), s.dt_trace()


def same_state(a, b, where):
    for k in STAT_KEYS:
        assert a[0][k] == b[0][k], (where, k, a[0][k], b[0][k])
    for k in PART_KEYS:  # device order: the divide's order itself
        assert np.array_equal(a[1][k], b[1][k]), (where, k)
    assert np.array_equal(a[2], b[2]), (where, "dt_trace")


def same_bits(a, b, where=None):
    same_state(state(a), state(b), where)


def stirred(case, frac, speed, seed=3):
    """Fluid particles given random velocities, so that many cross cell faces in every direction
    in every step (test_divide_inc.py)."""
    c = copy.copy(case)
    c.vel = case.vel.copy()
    rng = np.random.default_rng(seed)
    fl = np.arange(case.npb, case.np)
    pick = rng.choice(fl, int(frac * len(fl)), replace=False)
    c.vel[pick] = rng.uniform(-speed, speed, size=(len(pick), 3))
    return c


def far_movers(case, nfast, seed=7):
    """The far movers of test_divide_inc.py::test_inc_divide_exclusions: OUTMOVE / OUTPOS /
    OUTRHOP exclusions (the case has rhopoutmax = 1010)."""
    rng = np.random.default_rng(seed)
    pick = rng.choice(np.arange(case.npb, case.np), nfast, replace=False)
    q = nfast // 4
    case.vel[pick[:q]] = [0, 0, 400.0]
    case.vel[pick[q:2 * q]] = [0, 0, -30.0]
    case.vel[pick[2 * q:3 * q]] = [-120.0, 0, 0]
    case.vel[pick[3 * q:]] = [0, 25.0, 0]
    return case


def with_attrs(case, **kw):
    for k, v in kw.items():
        setattr(case, k, v)
    return case


def sym_stirred():
    return stirred(DamBreakCase(0.04, step_algorithm=2, tdensity=1, celldomfixed=True), 0.3, 2.0)


def verlet_stirred():
    return stirred(DamBreakCase(0.04, celldomfixed=True), 0.5, 3.0)


# name: (case factory, steps, steps between comparisons)
CASES = {
    # verlet_steps = 40: the Euler step and the reset of the Verlet counter are step 40
    "verlet_ddt2_euler_step": (lambda: DamBreakCase(0.05), 45, 9),
    "verlet_half_cells_stirred": (lambda: stirred(DamBreakCase(0.04, cellmode=2, celldomfixed=True), 0.5, 3.0), 20, 5),
    "symplectic_ddt1_stirred": (sym_stirred, 20, 5),
    # the settings of golden symplectic_shift_full_tfs_dp0.025: the corrector takes the shifting sums
    "symplectic_shifting": (lambda: stirred(DamBreakCase(0.04, step_algorithm=2, tdensity=2, shift_mode=3,
                                                          shift_coef=-2.0, shift_tfs=2.75), 0.3, 2.0), 12, 4),
    # mDBC: the corrector's interaction skips the boundary correction
    "symplectic_mdbc": (lambda: stirred(DamBreakCase(0.03, step_algorithm=2, tdensity=1, tboundary=2), 0.3, 2.0),
                        10, 5),
    "verlet_laminar_sps": (lambda: stirred(DamBreakCase(0.04, tvisco=2, visco=1e-6), 0.3, 2.0), 12, 4),
    "verlet_exclusions": (lambda: far_movers(DamBreakCase(0.04, celldomfixed=True, rhopoutmax=1010.0), 40), 12, 3),
    "symplectic_2d": (lambda: stirred(DamBreak2DCase(0.02, step_algorithm=2), 0.3, 2.0), 20, 5),
    "symplectic_nn": (lambda: WetDambreakNNCase(0.025, width=0.2, scale=0.5), 6, 3),
    # k_dt picks the fixed dt at the step's TimeStep: the corrector sees the time already advanced.
    # The first Symplectic step runs with DtIni (1.96 ms at dp 0.04), the next seven with the
    # table's <= 0.22 ms: TimeStep stays within 1.9 - 3.5 ms, where the rows (s, ms) slope
    "symplectic_dtfixed_table": (lambda: with_attrs(sym_stirred(), dtfixed_table=np.array(
        [[0.0, 0.08], [0.0015, 0.22], [0.0026, 0.10], [0.004, 0.2], [1.0, 0.2]])), 8, 2),
    # ViscoTime: Visco of the next step is set by the corrector's DtVariable, not the predictor's
    # (rows sloping over the same times)
    "symplectic_viscotime": (lambda: with_attrs(sym_stirred(), visco_table=np.array(
        [[0.0, 0.01], [0.0022, 0.3], [0.004, 0.05], [1.0, 0.05]])), 8, 2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_phase_loop_is_run(name):
    make, nsteps, chunk = CASES[name]
    case = make()
    a, b = gpu(case), gpu(case)
    same_bits(a, b, 0)
    for done in range(chunk, nsteps + 1, chunk):
        a.run(chunk)
        step_by_phases(b, chunk)
        same_bits(a, b, done)
    assert done == nsteps and a.stats()["nstep"] == nsteps
    a.sync()  # raises on a fatal error flag
    if name == "verlet_exclusions":
        assert a.stats()["nout"] > 0
    if name == "symplectic_dtfixed_table":
        tr = a.dt_trace()
        assert a.stats()["time"] < 0.004 and len(set(tr[1:])) >= 5, tr  # the steps ran on the table's slopes


@pytest.mark.parametrize("make", [verlet_stirred, sym_stirred], ids=["verlet", "symplectic"])
def test_run_and_phases_mix(make):
    case = make()
    a, b = gpu(case), gpu(case)
    a.run(15)
    b.run(5)
    step_by_phases(b, 5)
    b.run(5)
    same_bits(a, b, 15)


@pytest.mark.parametrize("make", [verlet_stirred, sym_stirred], ids=["verlet", "symplectic"])
def test_divide_without_update_changes_nothing(make):
    case = make()
    a, b = gpu(case), gpu(case)

    def idle_divides(n, where):
        before = state(b)
        for _ in range(n):
            b.RunCellDivide()
        same_state(before, state(b), where)

    idle_divides(1, "after create")
    same_bits(a, b, "after create")
    for k in range(4):
        a.run(1)
        # Symplectic: two more divides between the predictor's divide and the corrector too
        step_by_phases(b, 1, between=lambda: idle_divides(2, ("mid step", k)))
        idle_divides(2, ("between steps", k))
        same_bits(a, b, ("phases", k))
    a.run(3)
    b.run(3)
    idle_divides(1, "after run")
    same_bits(a, b, "after run")
    a.run(4)  # ... and the later steps are the plain run's, either way of stepping
    b.run(2)
    step_by_phases(b, 2)
    same_bits(a, b, "end")


def test_update_phases_refuse_bodies_and_motion():
    from dualsphysics_multilayer_amd.core import SphError

    s = gpu(WaveFlumeCase(0.025))  # a piston, a flap and a floating box
    before = state(s)
    for call in (s.ComputeVerlet, s.ComputeSymplecticPre, s.ComputeSymplecticCorr):
        with pytest.raises(SphError, match="motion|floating") as e:
            call()
        assert e.value.status == 7  # SPH_ERR_UNSUPPORTED
    same_state(before, state(s), "refused")
    s.Interaction_Forces(1)  # stays allowed (tests/test_bodies.py compares its output)
    s.sync()


def test_phases_refused_on_group_members():
    from dualsphysics_multilayer_amd.core import SphError, SphSlabGroup, slab_partition

    case = DamBreakCase(0.05)
    grp = SphSlabGroup(case, slab_partition(case, 2))
    m = grp.members[0]
    for call in (m.RunCellDivide, lambda: m.Interaction_Forces(1), lambda: m.DtVariable(True), m.ComputeVerlet,
                 m.ComputeSymplecticPre, m.ComputeSymplecticCorr):
        with pytest.raises(SphError, match="group") as e:
            call()
        assert e.value.status == 3  # SPH_ERR_STATE
    grp.close()


def _gauges(case):
    """Three velocity gauges in the fluid and one vertical SWL line of 64 points (the dicts of
    XmlCase.gauges, as tests/test_gpu_gauges.py builds them)."""
    def gdef(type_, **kw):
        g = dict(type=type_, output=True, computestart=0.0, computeend=1e9, computedt=0.0, outputstart=0.0,
                 outputend=1e9, outputdt=0.0, point0=[0.0] * 3, point2=[0.0] * 3, pointdir=[0.0] * 3, pointnp=0,
                 masslimit=0.0, height=0.0, distlimit=0.0, code=0)
        g.update(kw)
        return g

    gs = [gdef("velocity", point0=[0.2, 0.3, 0.1 + 0.05 * i]) for i in range(3)]
    ml = float(np.float32(case.mass) * np.float32(0.5))
    return gs + [gdef("swl", point0=[0.2, 0.3, 0.06], point2=[0.2, 0.3, 0.44], pointdir=[0.0, 0.0, 0.38 / 63],
                      pointnp=63, masslimit=ml)]


@pytest.mark.parametrize("step", [1, 2], ids=["verlet", "symplectic"])
def test_a_phase_step_is_a_step(step):
    """Configuration 'before the first step' is refused after a phase step as after run(1), and
    sph_solver_measure — the phase-level form of the gauges — returns the bytes it returns
    after the equal run(1)."""
    from dualsphysics_multilayer_amd.core import SphError

    case = DamBreakCase(0.05, step_algorithm=step)
    gs = _gauges(case)
    for stepper in (lambda s: s.run(1), lambda s: step_by_phases(s, 1)):
        s = gpu(case)
        stepper(s)
        with pytest.raises(SphError, match="before the first step") as e:
            s.set_gauges(gs, 64)
        assert e.value.status == 3
    a, b = gpu(case), gpu(case)
    a.set_gauges(gs, 64)
    b.set_gauges(gs, 64)
    assert a.measure().tobytes() == b.measure().tobytes()
    a.run(1)
    step_by_phases(b, 1)
    ma, mb = a.measure(), b.measure()
    assert ma.tobytes() == mb.tobytes()
    assert np.all(ma["time"] == a.stats()["time"]) and np.any(ma["v"] != 0)
    same_bits(a, b, 1)


# ---- SPH_CLS_SPLIT: the update kernel that also classifies against the separate kernels ----
@pytest.mark.parametrize("make,nsteps", [(verlet_stirred, 40), (sym_stirred, 20)], ids=["verlet", "symplectic"])
def test_fused_update_is_the_split_kernels(monkeypatch, make, nsteps):
    case = make()
    a, b = gpu(case), gpu(case, monkeypatch, split=True)
    for done in range(5, nsteps + 1, 5):
        a.run(5)
        b.run(5)
        same_bits(a, b, done)
    # the fused solver took the fused path, at every update: on one domain nothing invalidates
    # the sorted keys that the divide of creation left
    per_step = 2 if case.step_algorithm == SYMPLECTIC else 1
    assert a.stats()["fused_updates"] == per_step * nsteps
    assert b.stats()["fused_updates"] == 0


def test_fused_update_is_the_split_kernels_on_slabs(monkeypatch):
    from dualsphysics_multilayer_amd.core import SphSlabGroup, slab_partition

    case = verlet_stirred()
    bounds = slab_partition(case, 3)
    a = SphSlabGroup(case, bounds)
    monkeypatch.setenv("SPH_CLS_SPLIT", "1")
    b = SphSlabGroup(case, bounds)
    monkeypatch.delenv("SPH_CLS_SPLIT")
    for done in range(5, 21, 5):
        a.run(5)
        b.run(5)
        for r, (ma, mb) in enumerate(zip(a.members, b.members)):
            same_bits(ma, mb, (done, r))  # each slab's own order; the pack count is fused there too
    assert all(m.stats()["fused_updates"] > 0 for m in a.members)
    assert all(m.stats()["fused_updates"] == 0 for m in b.members)
    a.close()
    b.close()
