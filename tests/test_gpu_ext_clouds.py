"""k_fluid_ext (csrc/sph_ext.hip: Laminar+SPS viscosity and / or shifting) on off-lattice clouds
against a float64 all-pairs sum (tests/ext_clouds.py), with the outputs only the diagnostic
download shows: the shifting sums and the SPS stress tensor (sph_download_ext).

Per case one SphGpuSingle, one download_ext and one or two interaction downloads; no stepping.
What the clouds reach (the segmented branch of ext_pass, later candidate rounds, the
[record, image] segments, the one-shot branch) is asserted in tests/test_ext_clouds_cpu.py.

The rules, the same for every row:
* particle order particles()["idp"]; download buffers start as NaN and every slot is written;
  a fluid particle without neighbours has zero in every output; boundary rows of tau and of
  the shifting sums are 0, of ace 0;
* against float64: ar, ace, tau, the free particles' shifting sums (the vector part and the
  fourth sum each on its own) within max |d| / max |reference array| <= MARGIN x e32, e32 being
  the float32 evaluation's distance from the float64 one for the same cloud, mode and quantity
  (computed here); MARGIN = 10 as everywhere in this project;
* viscdt within MARGIN x e32 + clouds.viscdt_rounding (one pair's value, not a sum);
* the frozen set exactly the reference's; velmax / acemax consistent with the downloaded arrays
  to 1e-5;
* a comparison may leave out only particles with a BOUNDARY neighbour inside the 2e-6 shell
  around r = 2h (the last bit of r^2 decides their DDT switch or frozen flag); no cloud here
  has one, so nothing is left out (the count is printed per case).  sym and symwall have 10
  fluid particles with a fluid pair inside the shell: its terms vanish there (the kernel
  gradient is 0 at r = 2h), so they stay in.

The Laminar+SPS rows isolate the small terms: with rhoamp = 0 the pressure is exactly 0, the
first interaction's ace is the laminar term alone and the second's is dominated by the SPS
stress divergence (tests/test_ext_clouds_cpu.py asserts both on the reference).

Measured on an MI355X: e32 as the float32 evaluation gives it, then GPU / e32 per quantity, the
largest over the row's cases (DDT, ShiftMode); CellMode full / half:

  row                         e32 ar            e32 ace           ar         ace        tau        shift xyz  shift w
  sps blob, rhoamp 0.02, 2nd  8.0e-7 / 8.0e-7   9.7e-7 / 9.7e-7   1.0 / 1.1  2.7 / 3.2  1.6 / 1.6  -          -
  sps blob, rhoamp 0, 2nd     7.9e-7 / 7.9e-7   6.4e-7 / 6.4e-7   1.1 / 1.4  2.9 / 2.9  1.1 / 1.3  -          -
  sps uniform, 0.02, 2nd      5.3e-7 / 5.3e-7   3.2e-7 / 3.2e-7   1.0 / 0.7  1.5 / 2.3  1.4 / 1.5  -          -
  sps uniform, 0, 2nd         4.9e-7 / 4.9e-7   2.6e-7 / 2.6e-7   1.0 / 0.7  1.9 / 1.9  1.0 / 0.7  -          -
  laminar alone, blob         7.9e-7 / 7.9e-7   8.9e-7 / 8.9e-7   1.1 / 1.4  1.0 / 1.0  -          -          -
  laminar alone, uniform      4.9e-7 / 4.9e-7   3.1e-7 / 3.1e-7   1.0 / 0.7  0.8 / 0.7  -          -          -
  sps Cubic blob, 2nd         6.3e-7 / 6.3e-7   8.9e-7 / 8.9e-7   1.2 / 1.3  3.6 / 3.7  1.2 / 1.5  -          -
  shift uniform, modes 1-3    5.3e-7 / 5.3e-7   3.0e-7 / 3.0e-7   1.0 / 0.7  1.2 / 1.2  -          1.5 / 1.4  1.0 / 1.0
  shift blob, modes 1-3       8.0e-7 / 8.0e-7   9.2e-7 / 9.2e-7   1.0 / 1.1  1.2 / 1.7  -          1.7 / 1.5  1.1 / 1.1
  shift sym, modes 1-3        8.1e-7 / 8.1e-7   8.7e-7 / 8.7e-7   0.9 / 0.8  1.2 / 1.1  -          1.1 / 1.2  1.1 / 1.2
  shift symwall, modes 1-3    7.6e-7 / 7.6e-7   9.6e-7 / 9.6e-7   1.1 / 1.0  1.8 / 2.3  -          1.1 / 1.0  0.9 / 0.8
  shift mixedwall, modes 1-2  7.8e-7 / 7.8e-7   9.3e-7 / 9.3e-7   1.0 / 1.0  1.1 / 1.5  -          1.7 / 1.5  0.8 / 0.8
  shift Cubic blob, mode 1    6.3e-7 / 6.3e-7   8.7e-7 / 8.7e-7   1.2 / 1.3  1.7 / 1.4  -          1.0 / 0.7  1.0 / 0.9
  sps + shift blob, 0.02      8.0e-7 / 8.0e-7   9.7e-7 / 9.7e-7   1.0 / 1.1  2.7 / 3.2  1.6 / 1.6  1.7 / 1.5  1.1 / 1.1
  sps + shift blob, 0         7.9e-7 / 7.9e-7   6.4e-7 / 6.4e-7   1.0 / 1.3  2.9 / 2.9  1.1 / 1.3  2.2 / 1.9  1.1 / 1.6
  sps + shift spray           4.2e-7 / 4.2e-7   2.5e-7 / 2.5e-7   1.4 / 0.9  1.1 / 2.0  1.4 / 0.6  1.2 / 2.3  1.8 / 1.5

GPU / e32 is 0.6 to 3.7 everywhere.  max |ace| is 0.081 (blob) and 0.0062 (uniform) in the
"laminar alone" rows and 330 / 0.053 in the second interaction at rhoamp 0, against 9.1e3 / 462
with the density noise.  viscdt: GPU 1.8e-8 to 3.4e-7 relative, e32 1.8e-8 to 5.8e-8, the
rounding bound 1.0e-5 to 6.3e-5 (it is one pair's value; see tests/test_gpu_clouds.py).
Against the oracle at ShiftMode none: ar <= 9.4e-7, ace <= 2.1e-6.  Frozen sets equal the
reference's in every case; 0 particles left out of every comparison.

A build with the laminar factor 4 changed to 4.0001 fails all "laminar alone" cases and passes
the rows with density noise; a build that drains only half of a [record, image] segment fails
symwall under NoBound / NoFixed and nothing else.
"""
import ctypes as C

import numpy as np
import pytest

import clouds
import ext_clouds as X

pytestmark = pytest.mark.gpu

MARGIN = 10.0
SPH_ERR_ARG, SPH_ERR_STATE, SPH_ERR_UNSUPPORTED = 1, 3, 7  # include/sphcore.h
FLT_MAX = np.float32(np.finfo(np.float32).max)

_REF = {}


def derived(case):
    from dualsphysics_multilayer_amd.core import case_derive

    return case_derive(case.case_def())


def reference(case, K, ddt, tau=None, tag=None):
    """brute_ext in float64 and float32 and the e32 between them; cached per (tag, tau given)."""
    key = (tag, tau is not None)
    if tag is None or key not in _REF:
        r64 = X.brute_ext(case, K, ddt, tau=tau)
        r32 = X.brute_ext(case, K, ddt, tau=tau, dtype=np.float32)
        free = (np.arange(case.np) >= case.npb) & ~r64["frozen"]
        e = X.e32(r64, r32, free=free if case.shift_mode else None)
        if case.shift_mode:
            sx = np.abs(r64["shift"][free])
            d = np.abs(r32["shift"][free].astype(np.float64) - r64["shift"][free])
            e["shift_xyz"] = float(d[:, :3].max() / sx[:, :3].max())
            e["shift_w"] = float(d[:, 3].max() / sx[:, 3].max())
        if tag is None:
            return r64, e
        _REF[key] = (r64, e)
    return _REF[key]


def interaction(g):
    """sph_download_interaction into NaN-seeded buffers."""
    from dualsphysics_multilayer_amd._abi import SphInterOut
    from dualsphysics_multilayer_amd.core import _check, load_library

    n = g.stats()["np"]
    ar = np.full(n, np.nan, np.float32)
    ace = np.full((n, 3), np.nan, np.float32)
    fp = C.POINTER(C.c_float)
    out = SphInterOut(ar.ctypes.data_as(fp), ace.ctypes.data_as(fp), 0, 0, 0)
    _check(load_library().sph_download_interaction(g._h, C.byref(out)))
    return dict(ar=ar, ace=ace, viscdtmax=out.viscdtmax, velmax=out.velmax, acemax=out.acemax)


def lonely(case, K, idp):
    P = clouds.pairs(case, K)
    has = np.zeros(case.np, bool)
    real = P["real"]
    has[P["i"][real & ((P["i"] >= case.npb) | (P["j"] >= case.npb))]] = True
    return ~has[idp]


def check_inter(label, case, K, ig, ref, e32, idp, vel, ddt):
    """ar, ace, the three maxima of one interaction download against the reference."""
    npb = case.npb
    keep = ~ref["amb_ddt"][idp]
    ar_ref, ace_ref = ref["ar"][idp], ref["ace"][idp]
    assert not np.isnan(ig["ar"]).any() and not np.isnan(ig["ace"]).any()
    e_ar = np.abs(ig["ar"] - ar_ref)[keep].max() / np.abs(ar_ref).max()
    e_ace = np.abs(ig["ace"] - ace_ref).max() / np.abs(ace_ref).max()
    e_visc = abs(float(ig["viscdtmax"]) - ref["viscdt"]) / ref["viscdt"]
    vround = clouds.viscdt_rounding(K, ref)
    print("%s: gpu ar %.2e ace %.2e viscdt %.2e | e32 ar %.2e ace %.2e viscdt %.2e | ratio ar %.1f ace %.1f | viscdt "
          "rounding bound %.2e | max|ace| %.3g | left out %d"
          % (label, e_ar, e_ace, e_visc, e32["ar"], e32["ace"], e32["viscdt"], e_ar / e32["ar"], e_ace / e32["ace"],
             vround, np.abs(ace_ref).max(), (~keep).sum()))
    assert (~keep).sum() <= 0.005 * (case.np - npb)
    lone = lonely(case, K, idp)
    assert not ig["ar"][lone].any() and not ig["ace"][lone].any()
    assert not ig["ace"][:npb].any()
    amax = float(np.sqrt((ig["ace"].astype(np.float64) ** 2).sum(axis=1).max()))
    vmax = float(np.sqrt((vel.astype(np.float64) ** 2).sum(axis=1).max()))
    assert ig["acemax"] == pytest.approx(amax, rel=1e-5)
    assert ig["velmax"] == pytest.approx(vmax, rel=1e-5)
    assert e_ar <= MARGIN * e32["ar"], ("ar", e_ar, e32["ar"])
    assert e_ace <= MARGIN * e32["ace"], ("ace", e_ace, e32["ace"], worst(ig, ref, idp))
    assert e_visc <= MARGIN * e32["viscdt"] + vround, (e_visc, e32["viscdt"], vround)


def worst(ig, ref, idp):
    d = ig["ace"].astype(np.float64) - ref["ace"][idp]
    m = int(np.abs(d).max(axis=1).argmax())
    return "worst ace: idp %d d %s, pressure %s, viscous %s, SPS %s" % (
        idp[m], d[m], ref["ace_press"][idp[m]], ref["ace_visc"][idp[m]], ref["ace_sps"][idp[m]])


def check_ext(label, case, K, ext, ref, e32, idp):
    """tau and / or the shifting sums and the frozen set of one download_ext."""
    npb = case.npb
    lone = lonely(case, K, idp)
    if case.tvisco == 2:
        tau = ext["tau"]
        assert not np.isnan(tau).any() and not tau[:npb].any() and not tau[lone].any()
        e_tau = np.abs(tau - ref["tau"][idp]).max() / np.abs(ref["tau"]).max()
        print("%s: gpu tau %.2e | e32 %.2e | ratio %.1f | max|tau| %.3g"
              % (label, e_tau, e32["tau"], e_tau / e32["tau"], np.abs(ref["tau"]).max()))
        assert e_tau <= MARGIN * e32["tau"], (e_tau, e32["tau"])
    else:
        assert ext["tau"] is None
    if case.shift_mode:
        sp = ext["shiftposfs"]
        assert not np.isnan(sp).any() and not sp[:npb].any() and not sp[lone].any()
        amb = ref["amb_frozen"][idp]
        fluid = np.arange(case.np) >= npb
        frozen = sp[:, 0] == FLT_MAX
        assert np.array_equal(frozen[~amb], ref["frozen"][idp][~amb]), "frozen set"
        free = fluid & ~ref["frozen"][idp] & ~amb
        sref = ref["shift"][idp]
        allfree = (np.arange(case.np) >= npb) & ~ref["frozen"]
        mx, mw = np.abs(ref["shift"][allfree][:, :3]).max(), np.abs(ref["shift"][allfree][:, 3]).max()
        e_xyz = np.abs(sp[free, :3] - sref[free, :3]).max() / mx
        e_w = np.abs(sp[free, 3] - sref[free, 3]).max() / mw
        print("%s: gpu shift xyz %.2e w %.2e | e32 %.2e %.2e | ratio %.1f %.1f | frozen %d free %d left out %d"
              % (label, e_xyz, e_w, e32["shift_xyz"], e32["shift_w"], e_xyz / e32["shift_xyz"], e_w / e32["shift_w"],
                 frozen.sum(), free.sum(), amb.sum()))
        assert amb.sum() <= 0.005 * (case.np - npb)
        assert free.sum() >= 0.1 * (case.np - npb)
        assert e_xyz <= MARGIN * e32["shift_xyz"], (e_xyz, e32["shift_xyz"])
        assert e_w <= MARGIN * e32["shift_w"], (e_w, e32["shift_w"])
        return frozen
    assert ext["shiftposfs"] is None
    return None


def solver(case):
    from dualsphysics_multilayer_amd.core import SphGpuSingle

    g = SphGpuSingle(case, device=0)
    s = g.stats()
    assert (s["np"], s["npb"], s["nout"]) == (case.np, case.npb, 0)
    return g


def run_case(label, case, ddt, tag, second=True):
    """One solver: download_ext(keep_tau = 1) against the reference's first interaction, then an
    interaction download against the reference's second one (tau = the reference's)."""
    K = derived(case)
    ref1, e1 = reference(case, K, ddt, tag=tag)
    g = solver(case)
    try:
        part = g.particles()
        idp = part["idp"].astype(np.int64)
        ext = g.download_ext(keep_tau=True)
        frozen = check_ext(label, case, K, ext, ref1, e1, idp)
        if second:
            tau = ref1.get("tau")
            ref2, e2 = reference(case, K, ddt, tau=tau, tag=tag) if tau is not None else (ref1, e1)
            check_inter(label + " 2nd" if tau is not None else label, case, K, interaction(g), ref2, e2, idp,
                        part["vel"], ddt)
    finally:
        g.close()
    return ref1, frozen, idp


def make(name, **kw):
    return X.make(name, small=(name == "uniform"), **kw)


# ----------------------------------------------------------------------------------------
# 1. Laminar+SPS
SPS_CASES = [("blob", d) for d in (0, 1, 2, 3)] + [("uniform", 2)]


@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("rhoamp", [0.02, 0.0])
@pytest.mark.parametrize("name,ddt", SPS_CASES)
def test_laminar_sps(name, ddt, rhoamp, cellmode):
    """tau of the first interaction, then the second interaction reading it."""
    case = make(name, tdensity=ddt, cellmode=cellmode, tvisco=2, visco=1e-6, rhoamp=rhoamp)
    run_case("sps %s ddt %d rhoamp %g cellmode %d" % (name, ddt, rhoamp, cellmode), case, ddt,
             ("sps", name, ddt, rhoamp, cellmode))


@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("name,ddt", SPS_CASES)
def test_laminar_alone(name, ddt, cellmode):
    """rhoamp = 0 on a fresh solver: no pressure, tau = 0: ace is the laminar term alone."""
    case = make(name, tdensity=ddt, cellmode=cellmode, tvisco=2, visco=1e-6, rhoamp=0.0)
    K = derived(case)
    ref, e = reference(case, K, ddt, tag=("sps", name, ddt, 0.0, cellmode))
    assert not ref["ace_press"].any() and not ref["ace_sps"].any()
    g = solver(case)
    try:
        part = g.particles()
        check_inter("laminar alone %s ddt %d cellmode %d" % (name, ddt, cellmode), case, K, interaction(g), ref, e,
                    part["idp"].astype(np.int64), part["vel"], ddt)
    finally:
        g.close()


@pytest.mark.parametrize("cellmode", [1, 2])
def test_laminar_sps_cubic(cellmode):
    case = make("blob", tdensity=2, cellmode=cellmode, tvisco=2, visco=1e-6, kernel=1)
    run_case("sps cubic blob ddt 2 cellmode %d" % cellmode, case, 2, ("spscubic", cellmode))


@pytest.mark.parametrize("cellmode", [1, 2])
def test_inspection_leaves_the_state(cellmode):
    """After download_ext(keep_tau = 0) an interaction download equals a fresh solver's bit for
    bit (the state's tensor is untouched, the accumulators are reset); after keep_tau = 1 it
    does not (the tensor is in use)."""
    case = make("blob", tdensity=2, cellmode=cellmode, tvisco=2, visco=1e-6, shift_mode=3)
    g = solver(case)
    fresh = interaction(g)
    g.close()
    g = solver(case)
    ext0 = g.download_ext(keep_tau=False)
    after = interaction(g)
    for k in ("ar", "ace"):
        assert np.array_equal(fresh[k], after[k]), k
    for k in ("viscdtmax", "velmax", "acemax"):
        assert fresh[k] == after[k], k
    ext1 = g.download_ext(keep_tau=True)
    assert np.array_equal(ext0["tau"], ext1["tau"]) and np.array_equal(ext0["shiftposfs"], ext1["shiftposfs"])
    used = interaction(g)
    g.close()
    assert np.array_equal(used["ar"], fresh["ar"]) and not np.array_equal(used["ace"], fresh["ace"])
    assert used["viscdtmax"] == fresh["viscdtmax"]


# ----------------------------------------------------------------------------------------
# 2. shifting with artificial viscosity
SHIFT_CASES = ([(n, m, 2) for n in ("uniform", "blob", "sym", "symwall") for m in (1, 2, 3)] + [("blob", 1, 1)] +
               [("mixedwall", 1, 2), ("mixedwall", 2, 2)])


@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("name,mode,ddt", SHIFT_CASES)
def test_shifting(name, mode, ddt, cellmode):
    case = make(name, tdensity=ddt, cellmode=cellmode, shift_mode=mode)
    run_case("shift %s mode %d ddt %d cellmode %d" % (name, mode, ddt, cellmode), case, ddt,
             ("shift", name, mode, ddt, cellmode))


@pytest.mark.parametrize("cellmode", [1, 2])
def test_mixedwall_modes_freeze_different_sets(cellmode):
    """NoBound freezes next to any boundary particle, NoFixed only next to a fixed one: on
    mixedwall the two frozen sets differ, in the reference and on the GPU alike."""
    got, want = {}, {}
    for mode in (1, 2):
        case = make("mixedwall", tdensity=2, cellmode=cellmode, shift_mode=mode)
        ref, frozen, idp = run_case("mixedwall mode %d cellmode %d" % (mode, cellmode), case, 2,
                                    ("shift", "mixedwall", mode, 2, cellmode), second=False)
        got[mode] = np.zeros(case.np, bool)
        got[mode][idp] = frozen
        want[mode] = ref["frozen"]
    assert (want[1] & ~want[2]).sum() >= 20 and (got[1] & ~got[2]).sum() >= 20
    assert np.array_equal(got[1] & ~got[2], want[1] & ~want[2]) and not (got[2] & ~got[1]).any()


@pytest.mark.parametrize("cellmode", [1, 2])
def test_shifting_cubic(cellmode):
    case = make("blob", tdensity=2, cellmode=cellmode, shift_mode=1, kernel=1)
    run_case("shift cubic blob mode 1 ddt 2 cellmode %d" % cellmode, case, 2, ("shiftcubic", cellmode))


@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("name,mode", [("uniform", 1), ("blob", 3), ("sym", 1), ("symwall", 1), ("symwall", 2),
                                       ("mixedwall", 2)])
def test_shifting_leaves_ar_ace_to_the_oracle(name, mode, cellmode):
    """Shifting changes neither ar nor ace nor the maxima: they equal the CPU oracle's (the real
    reference's code) on the same cloud with ShiftMode none, within the 1e-5 of
    tests/test_gpu_clouds.py."""
    oracle = pytest.importorskip("oracle.pyoracle")
    case = make(name, tdensity=2, cellmode=cellmode, shift_mode=mode)
    o = oracle.OracleSolver(X.plain(case, shift_mode=0), nthreads=8)
    io = o.interaction()
    oidp = o.particles()["idp"]
    g = solver(case)
    try:
        g.download_ext(keep_tau=False)
        ig = interaction(g)
        idp = g.particles()["idp"]
    finally:
        g.close()
    assert np.array_equal(idp, oidp)
    o_ar = np.abs(ig["ar"] - io["ar"]).max() / np.abs(io["ar"]).max()
    o_ace = np.abs(ig["ace"] - io["ace"]).max() / np.abs(io["ace"]).max()
    print("shift %s mode %d cellmode %d vs oracle: ar %.2e ace %.2e" % (name, mode, cellmode, o_ar, o_ace))
    assert o_ar <= 1e-5 and o_ace <= 1e-5
    for k in ("velmax", "acemax", "viscdtmax"):
        assert ig[k] == pytest.approx(io[k], rel=1e-5), k


# ----------------------------------------------------------------------------------------
# 3. both options
@pytest.mark.parametrize("cellmode", [1, 2])
@pytest.mark.parametrize("rhoamp", [0.02, 0.0])
@pytest.mark.parametrize("mode", [1, 3])
def test_laminar_sps_with_shifting(mode, rhoamp, cellmode):
    case = make("blob", tdensity=2, cellmode=cellmode, tvisco=2, visco=1e-6, shift_mode=mode, rhoamp=rhoamp)
    run_case("sps+shift blob mode %d rhoamp %g cellmode %d" % (mode, rhoamp, cellmode), case, 2,
             ("both", mode, rhoamp, cellmode))


@pytest.mark.parametrize("cellmode", [1, 2])
def test_isolated_particles(cellmode):
    """spray: fluid particles without any neighbour (and mostly empty rows) have zero in ar,
    ace, tau and the shifting sums; none of the other clouds has such a particle."""
    case = make("spray", tdensity=2, cellmode=cellmode, tvisco=2, visco=1e-6, shift_mode=3)
    K = derived(case)
    assert clouds.reaches(case, K)["lonely_fluid"] >= 5
    run_case("sps+shift spray mode 3 cellmode %d" % cellmode, case, 2, ("spray", cellmode))


# ----------------------------------------------------------------------------------------
# the call's error answers
def test_download_ext_errors():
    from dualsphysics_multilayer_amd._abi import SphExtOut
    from dualsphysics_multilayer_amd.case import DamBreakCase
    from dualsphysics_multilayer_amd.core import SphError, SphGpuSingle, SphSlabGroup, load_library, slab_partition

    L = load_library()
    assert L.sph_abi_version() == 18
    fp = C.POINTER(C.c_float)
    buf = np.full((8000, 6), np.nan, np.float32)
    both = SphExtOut(buf.ctypes.data_as(fp), buf.ctypes.data_as(fp))
    assert L.sph_download_ext(None, C.byref(both), 0) == SPH_ERR_ARG and b"invalid argument" in L.sph_last_error()
    plain = DamBreakCase(0.05)
    g = SphGpuSingle(plain, device=0)
    assert L.sph_download_ext(g._h, None, 0) == SPH_ERR_ARG
    with pytest.raises(SphError, match="SPH_ERR_STATE"):
        g.download_ext()  # neither option: nothing to download
    for out in (SphExtOut(buf.ctypes.data_as(fp), fp()), SphExtOut(fp(), buf.ctypes.data_as(fp))):
        assert L.sph_download_ext(g._h, C.byref(out), 0) == SPH_ERR_STATE, L.sph_last_error()
    g.close()
    assert np.isnan(buf).all()
    # tau without Laminar+SPS, shiftposfs without shifting
    g = SphGpuSingle(make("uniform", tdensity=2, shift_mode=3), device=0)
    assert L.sph_download_ext(g._h, C.byref(both), 0) == SPH_ERR_STATE and b"Laminar" in L.sph_last_error()
    assert g.download_ext()["tau"] is None
    g.close()
    g = SphGpuSingle(make("uniform", tdensity=2, tvisco=2, visco=1e-6), device=0)
    assert L.sph_download_ext(g._h, C.byref(both), 0) == SPH_ERR_STATE and b"shifting" in L.sph_last_error()
    assert g.download_ext()["shiftposfs"] is None
    g.close()
    # a slab group's member
    grp = SphSlabGroup(plain, slab_partition(plain, 2))
    assert L.sph_download_ext(grp.members[0]._h, C.byref(both), 0) == SPH_ERR_UNSUPPORTED, L.sph_last_error()
    grp.close()
