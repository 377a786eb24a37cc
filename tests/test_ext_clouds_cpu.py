"""The Laminar+SPS / shifting clouds without a GPU (tests/ext_clouds.py): they reach what makes
tests/test_gpu_ext_clouds.py mean something, from clouds.reaches and the float64 reference
alone.

k_fluid_ext (csrc/sph_ext.hip) stages ExtCap = 416 records per segment with artificial
viscosity and 312 with Laminar+SPS; a row range above that takes the segmented branch of
ext_pass, a range at or below it the one-shot branch; a window above 128 takes later candidate
rounds.  With Symmetry the ordered bound pass (ShiftMode NoBound / NoFixed) stages each record
of the first rows in y followed by its image: 2 records per particle, so more than 208
boundary particles in a range make it segmented.
"""
import numpy as np
import pytest

import clouds
import ext_clouds as X
from dualsphysics_multilayer_amd.core import case_derive

CAP_ART, CAP_SPS = X.EXTCAP[1], X.EXTCAP[2]
SHIFT_CLOUDS = (("uniform", True), ("blob", False), ("sym", False), ("symwall", False), ("mixedwall", False))


def derived(case):
    return case_derive(case.case_def())


def first_rows_bound_range(case, K):
    """The fullest 6-cell (half cells: 9) x range of one boundary row of the first S rows in y."""
    c, nc = clouds._cells(case, K)
    div = int(K["scelldiv"])
    w = 6 if div == 1 else 9
    cb = c[:case.npb]
    best = 0
    for cy in range(div):
        for cz in range(int(nc[2])):
            hist = np.bincount(cb[(cb[:, 1] == cy) & (cb[:, 2] == cz)][:, 0], minlength=int(nc[0]))
            cum = np.concatenate([[0], hist.cumsum()])
            best = max(best, int((cum[w:] - cum[:-w]).max()))
    return best


def test_download_ext_is_exported():
    """C ABI 18: sph_download_ext is there and answers NULL arguments with SPH_ERR_ARG (no GPU
    is touched before the argument check)."""
    import ctypes as C

    from dualsphysics_multilayer_amd._abi import SphExtOut
    from dualsphysics_multilayer_amd.core import load_library

    L = load_library()
    assert L.sph_abi_version() == 18
    out = SphExtOut()
    assert L.sph_download_ext(None, C.byref(out), 0) == 1 and b"invalid argument" in L.sph_last_error()
    assert C.sizeof(SphExtOut) == 2 * C.sizeof(C.c_void_p)


def test_reach_blob():
    """blob: a 6-cell fluid range and a boundary range above 416 (segments with either record
    size), windows beyond the first 128 candidates; half cells: one half-cell row range above 312."""
    case = X.make("blob", cellmode=1)
    r = clouds.reaches(case, derived(case))
    print("blob full", r)
    assert r["range_fluid"] > CAP_ART and r["range_bound"] > CAP_ART
    assert r["window_fluid"] > 128 and r["window_bound"] > 128
    case = X.make("blob", cellmode=2)
    r = clouds.reaches(case, derived(case))
    print("blob half", r)
    assert r["range_fluid"] > CAP_SPS
    assert case.np <= 5000


def test_reach_uniform_small_is_one_shot():
    """uniform (small): every range at or below 312, so the one-shot branch runs too."""
    for cm in (1, 2):
        case = X.make("uniform", small=True, cellmode=cm)
        r = clouds.reaches(case, derived(case))
        print("uniform small cellmode %d" % cm, r)
        assert 0 < r["range_fluid"] <= CAP_SPS and 0 < r["range_bound"] <= CAP_SPS


@pytest.mark.parametrize("cm", [1, 2])
def test_reach_symwall(cm):
    """symwall: more than 208 boundary particles in one range of a boundary row of the first
    rows in y (2 staged records each: more than 416), under fluid within 2h of both the patch
    and the plane."""
    case = X.make("symwall", cellmode=cm, shift_mode=1)
    K = derived(case)
    assert case.symmetry and case.np <= 5000
    n = first_rows_bound_range(case, K)
    print("symwall cellmode %d: first-rows boundary range %d" % (cm, n))
    assert n > CAP_ART // 2
    # the sym cloud itself stays below it: only the patch makes the layout segmented
    sym = X.make("sym", cellmode=cm, shift_mode=1)
    assert first_rows_bound_range(sym, derived(sym)) <= CAP_ART // 2
    ks = float(np.float32(K["kernelsize"]))
    P = clouds.pairs(case, K)
    patch = np.zeros(case.np, bool)
    patch[case.npb - X._SYMWALL_PATCH[2]:case.npb] = True
    near = np.zeros(case.np, bool)
    near[P["i"][P["real"] & patch[P["j"]] & (P["i"] >= case.npb)]] = True
    near &= case.pos[:, 1] <= ks
    print("  fluid within 2h of the patch and of the plane: %d" % near.sum())
    assert near.sum() >= 50
    # and some of them meet an image of a patch particle
    img = np.zeros(case.np, bool)
    img[P["i"][P["real"] & P["image"] & patch[P["j"]] & (P["i"] >= case.npb)]] = True
    assert img.sum() >= 50


def test_reach_mixedwall():
    """mixedwall: case order fixed, moving, fluid; at least 20 fluid particles with a moving
    but no fixed boundary neighbour and at least 20 with a fixed one; NoBound and NoFixed
    freeze different sets."""
    c1 = X.make("mixedwall", shift_mode=1)
    c2 = X.make("mixedwall", shift_mode=2)
    K = derived(c1)
    code = X.codes(c1).astype(np.int64) & 0x1800
    nmov = int((code == X.CODE_TYPE_MOVING).sum())
    nfix = c1.npb - nmov
    assert nmov >= 200 and (code[:nfix] == 0).all() and (code[nfix:c1.npb] == X.CODE_TYPE_MOVING).all()
    assert (code[c1.npb:] == 0x1800).all() and not c1.vel[:c1.npb].any()
    blob = X.make("blob")
    assert np.array_equal(np.sort(c1.pos, axis=0), np.sort(blob.pos, axis=0)) and c1.npb == blob.npb
    f1 = X.brute_ext(c1, K, 2)["frozen"]
    f2 = X.brute_ext(c2, K, 2)["frozen"]
    print("mixedwall: frozen NoBound %d, NoFixed %d" % (f1.sum(), f2.sum()))
    assert (f1 & ~f2).sum() >= 20  # a moving neighbour, no fixed one
    assert f2.sum() >= 20 and not (f2 & ~f1).any()


@pytest.mark.parametrize("name,small", SHIFT_CLOUDS)
def test_frozen_fraction_and_ambiguity(name, small):
    """Under NoBound at least 10 % of the fluid frozen and 10 % free; at most 0.5 % of the
    fluid with a pair inside the 2e-6 shell around r = 2h (for the frozen flag and the DDT
    switch: a boundary neighbour) -- the only particles a comparison may leave out."""
    for cm in (1, 2):
        case = X.make(name, small=small, cellmode=cm, shift_mode=1)
        K = derived(case)
        ref = X.brute_ext(case, K, 2)
        nf = case.np - case.npb
        fr = int(ref["frozen"][case.npb:].sum())
        print("%s cellmode %d: frozen %d of %d, in the shell: any %d, bound %d"
              % (name, cm, fr, nf, ref["amb_any"].sum(), ref["amb"].sum()))
        assert not ref["frozen"][:case.npb].any()
        assert 0.1 * nf <= fr <= 0.9 * nf
        assert ref["amb_any"].sum() <= 0.005 * nf and ref["amb"].sum() <= 0.005 * nf
        if name in X.NEW:
            # the new particles and codes add no pair inside the shell: none with a boundary
            # particle, the others those of the cloud they are built on
            src = X.make({"symwall": "sym", "mixedwall": "blob"}[name], cellmode=cm, shift_mode=1)
            assert ref["amb"].sum() == 0
            assert ref["amb_any"].sum() == X.brute_ext(src, derived(src), 2)["amb_any"].sum()


@pytest.mark.parametrize("name,small", (("uniform", True), ("blob", False)))
def test_still_density_isolates_the_viscous_terms(name, small):
    """rhoamp = 0: pressure is exactly 0, so the first interaction's ace is the laminar term
    alone, and in the second (tau of the first) the SPS term is at least half of max |ace|."""
    case = X.make(name, small=small, tdensity=2, tvisco=2, visco=1e-6, rhoamp=0.0)
    K = derived(case)
    assert (case.rhop == np.float32(case.rhop0)).all()
    assert not clouds.pressure(case, K).any()
    a = X.brute_ext(case, K, 2)
    assert not a["ace_press"].any() and not a["ace_sps"].any()
    assert np.array_equal(a["ace"], a["ace_visc"]) and np.abs(a["ace"]).max() > 0
    b = X.brute_ext(case, K, 2, tau=a["tau"])
    assert not b["ace_press"].any() and np.array_equal(b["ace_visc"], a["ace_visc"])
    sps, lam, tot = (np.abs(b[k]).max() for k in ("ace_sps", "ace_visc", "ace"))
    print("%s: max|ace| laminar %.3g, SPS %.3g, both %.3g" % (name, lam, sps, tot))
    assert sps >= 0.5 * tot
    # with the density noise the pressure term hides both (why these rows exist)
    c2 = X.make(name, small=small, tdensity=2, tvisco=2, visco=1e-6, rhoamp=0.02)
    p = np.abs(X.brute_ext(c2, derived(c2), 2)["ace_press"]).max()
    assert lam < 1e-3 * p


def test_reference_bookkeeping():
    """The reference's own consistency: with artificial viscosity and no shifting it is
    clouds.brute; the terms add up; tau is ComputeSpsTau of the gradients; a second call with
    tau changes ace only by the SPS term; the float32 evaluation is close to the float64 one."""
    case = X.make("uniform", small=True, tdensity=2)
    K = derived(case)
    b, e = clouds.brute(case, K, 2), X.brute_ext(case, K, 2)
    for q in ("ar", "ace"):
        assert np.allclose(e[q], b[q], rtol=1e-12, atol=1e-12 * np.abs(b[q]).max())
    assert e["viscdt"] == b["viscdt"]
    case = X.make("uniform", small=True, tdensity=2, tvisco=2, visco=1e-6, shift_mode=3)
    K = derived(case)
    a = X.brute_ext(case, K, 2)
    assert np.allclose(a["ace"], a["ace_press"] + a["ace_visc"] + a["ace_sps"])
    assert np.array_equal(a["tau"][case.npb:], X.sps_tau(K, a["grad"], case.rhop.astype(np.float64))[case.npb:])
    assert not a["tau"][:case.npb].any() and not a["grad"][:case.npb].any() and not a["frozen"].any()
    c = X.brute_ext(case, K, 2, tau=a["tau"])
    assert np.array_equal(c["ar"], a["ar"]) and np.array_equal(c["grad"], a["grad"])
    assert np.allclose(c["ace"] - a["ace"], c["ace_sps"], atol=1e-9 * np.abs(c["ace"]).max())
    a32 = X.brute_ext(case, K, 2, dtype=np.float32)
    assert a32["ar"].dtype == np.float32 and a32["tau"].dtype == np.float32 and a32["shift"].dtype == np.float32
    e32 = X.e32(a, a32, free=np.arange(case.np) >= case.npb)
    print("e32", e32)
    for q, v in e32.items():
        assert 0 < v <= 1e-5, (q, v)
    # the sums' signs: -sum m2/rho2 dr.fr > 0 (fac < 0), and a lone fluid particle has zero sums
    assert (a["shift"][case.npb:, 3] >= 0).all()
