"""Off-lattice clouds without a GPU (tests/clouds.py): the clouds reach what they are built
to reach, and the CPU oracle agrees with a float64 all-pairs sum on them.

* Reach preconditions: what makes tests/test_gpu_clouds.py mean something.  The tiled
  kernels (csrc/sph_tiled.hpp) hold TB = 128 particles per item, TCAP = 504 staged records
  per segment, 128 (half cells: 64) candidates per window and round.
* Oracle against brute force: the oracle (oracle/sph_oracle.cpp, float, cell search) against
  clouds.brute (float64, all pairs) for every cloud, DDT 0-3, both cell modes and both
  builds (-ffast-math and strict).  The larger error of the two builds is e_ref, the
  reference's own floor off the lattice; it is held to 1e-5, the identical-input bar of
  tests/test_gpu_parity.py::test_interaction_identical_input.
* At most 0.5 % of a cloud's fluid is left out of the ar comparison under DDT 1 and 2 (a
  bound neighbour within 2e-6 of r = 2h decides whether the DDT term is on).

Measured e_ref (max over DDT 0-3 and both cell modes; ar, ace of the array's maximum,
viscdt relative): see the table in tests/test_gpu_clouds.py.
"""
import numpy as np
import pytest

import clouds

oracle = pytest.importorskip("oracle.pyoracle")

MODES = [(name, cm) for name in clouds.NAMES for cm in (1, 2)]


def derived(case):
    return oracle.derive(case.case_def())


@pytest.mark.parametrize("name", clouds.NAMES)
def test_cloud_case_is_valid_input(name):
    """Boundary first and at rest, fluid moving, densities inside RhopOut, every particle
    strictly inside the map, cells 0 and n-1 of every axis filled; the oracle takes the case
    unchanged, excludes nothing and returns ace without gravity."""
    case = clouds.make(name, tdensity=0)
    lo, hi = case.map_limits()
    assert case.np <= 7500 and 0 < case.npb < case.np
    assert (case.pos > lo).all() and (case.pos < hi).all()
    assert not case.vel[:case.npb].any() and np.abs(case.vel[case.npb:]).max() <= 1.0
    assert case.rhop.min() > case.rhopoutmin and case.rhop.max() < case.rhopoutmax
    for cm in (1, 2):
        case = clouds.make(name, tdensity=0, cellmode=cm)
        K = derived(case)
        c, nc = clouds._cells(case, K)
        assert (c.min(axis=0) == 0).all() and (c.max(axis=0) == nc - 1).all()
    o = oracle.OracleSolver(case, nthreads=4)
    s = o.stats()
    assert (s["np"], s["npb"], s["nout"]) == (case.np, case.npb, 0)
    assert np.array_equal(np.sort(o.particles()["idp"]), case.idp)
    # a fluid particle without neighbours: ace = 0 exactly, so gravity is not part of ace
    if name == "spray":
        P = clouds.pairs(case, K)
        has = np.zeros(case.np, bool)
        has[P["i"]] = True
        io = o.interaction()
        lonely = ~has[o.particles()["idp"]]
        assert lonely[case.npb:].sum() >= 5
        assert not io["ace"][lonely].any() and not io["ar"][lonely].any()


def test_generators_are_seeded():
    a, b = clouds.make("spray", tdensity=0), clouds.make("spray", tdensity=2, cellmode=2)
    assert np.array_equal(a.pos, b.pos) and np.array_equal(a.vel, b.vel) and np.array_equal(a.rhop, b.rhop)
    c = clouds.make("spray", seed=99, tdensity=0)
    assert not np.array_equal(a.pos[:10], c.pos[:10])


# ----------------------------------------------------------------------------------------
def test_reach_blob():
    """blob: a fluid cell and a bound cell hold more than one item (items inside one cell), a
    neighbour row takes at least 3 TCAP segments, a window at least 4 rounds; with half
    cells a window takes later rounds and a single half-cell row exceeds TCAP."""
    r = clouds.reaches(clouds.make("blob", cellmode=1), derived(clouds.make("blob", cellmode=1)))
    print("blob full", r)
    assert r["cell_fluid"] > 128 and r["cell_bound"] > 128
    assert r["range_fluid"] > 2 * clouds.TCAP
    assert r["window_fluid"] > 384
    r = clouds.reaches(clouds.make("blob", cellmode=2), derived(clouds.make("blob", cellmode=2)))
    print("blob half", r)
    assert r["window_fluid"] > 128
    assert r["range_fluid"] > clouds.TCAP


def test_reach_longrow():
    """longrow with half cells: 128 consecutive fluid particles of a row span at least 30
    half-cells, so items are cut at their full 32."""
    case = clouds.make("longrow", cellmode=2)
    r = clouds.reaches(case, derived(case))
    print("longrow half", r)
    assert r["span128"] >= 30


def test_reach_spray():
    """spray: at least 5 fluid particles without any neighbour, and most rows empty."""
    case = clouds.make("spray", cellmode=1)
    r = clouds.reaches(case, derived(case))
    print("spray", r)
    assert r["lonely_fluid"] >= 5
    assert r["cell_fluid"] <= 6


def test_reach_uniform_coefh15():
    """The reduced uniform cloud at coefh = 1.5: a mirrored pair of 6-cell row ranges exceeds
    TCAP, so the units of run_pass take the row-by-row path."""
    case = clouds.make("uniform", small=True, coefh=1.5, cellmode=1)
    r = clouds.reaches(case, derived(case))
    print("uniform coefh 1.5", r)
    assert r["pair_fluid"] > clouds.TCAP
    assert case.np <= 7500


def test_reach_sym():
    """sym: at least a third of the fluid within 2h of the mirror; the first row's patch
    exceeds TCAP in one row (the mirrored units take the segmented path, the own row's image
    included), with half cells in one half-cell row."""
    for cm in (1, 2):
        case = clouds.make("sym", cellmode=cm)
        K = derived(case)
        assert case.symmetry and case.map_limits()[0][1] == 0.0 and case.pos[:, 1].min() > 0.0
        near = case.pos[case.npb:, 1] <= float(np.float32(K["kernelsize"]))
        assert near.mean() >= 1.0 / 3.0
        c, nc = clouds._cells(case, K)
        cf = c[case.npb:]
        first = cf[cf[:, 1] == 0]
        rows = np.bincount(first[:, 2], minlength=nc[2])
        print("sym cellmode %d: first-row fluid per z" % cm, rows)
        assert rows.max() > clouds.TCAP


# ----------------------------------------------------------------------------------------
E_REF = {}


@pytest.mark.parametrize("ddt", [0, 1, 2, 3])
@pytest.mark.parametrize("name,cm", MODES)
def test_oracle_matches_brute_force(name, cm, ddt):
    """e_ref(cloud, mode, quantity) <= 1e-5 for both oracle builds; real-pair counts within
    the number of pairs inside the 2e-6 shell; the particles left out of the ar comparison
    (DDT 1 and 2 only) at most 0.5 % of the fluid."""
    case = clouds.make(name, tdensity=ddt, cellmode=cm)
    K = derived(case)
    ref = clouds.brute(case, K, ddt)
    fast, strict, e_ref = clouds.oracle_floor(case, ref, ddt)
    E_REF[(name, cm, ddt)] = e_ref
    print("%s cellmode %d ddt %d: e_ref ar %.2e ace %.2e viscdt %.2e (fast-math %s, strict %s), amb %d of %d"
          % (name, cm, ddt, e_ref["ar"], e_ref["ace"], e_ref["viscdt"], fast["err"], strict["err"],
             ref["amb"][case.npb:].sum(), case.np - case.npb))
    for q in ("ar", "ace", "viscdt"):
        assert e_ref[q] <= 1e-5, (q, e_ref[q])
    for io in (fast, strict):
        assert (io["stats"]["np"], io["stats"]["nout"]) == (case.np, 0)
        assert np.all(np.abs(io["counts"][[1, 3, 5]] - ref["counts"]) <= ref["shell"]), (io["counts"], ref["counts"],
                                                                                         ref["shell"])
    assert not ref["amb"][:case.npb].any()
    assert ref["amb"].sum() <= 0.005 * (case.np - case.npb)


def test_brute_force_terms():
    """The reference's own bookkeeping: its terms add up, DDT is off exactly where a bound
    neighbour is in reach under DDT 1/2 and nowhere under DDT 3, pairs are symmetric."""
    case = clouds.make("uniform", small=True, tdensity=2)
    K = derived(case)
    P = clouds.pairs(case, K)
    fwd = set(zip(P["i"].tolist(), P["j"].tolist()))
    assert all((j, i) in fwd for i, j in list(fwd)[:2000])
    b2, b3, b0 = (clouds.brute(case, K, d) for d in (2, 3, 0))
    assert np.array_equal(b2["ace"], b0["ace"]) and np.array_equal(b2["ar_cont"], b0["ar_cont"])
    assert np.allclose(b2["ace"], b2["ace_press"] + b2["ace_visc"])
    assert b2["ddt_off"][case.npb:].any() and not b3["ddt_off"].any()
    assert np.array_equal(b3["ar"], b3["ar_cont"] + b3["delta"])
    assert np.array_equal(b2["ar"][b2["ddt_off"]], b2["ar_cont"][b2["ddt_off"]])
    assert not b2["ace"][:case.npb].any()
