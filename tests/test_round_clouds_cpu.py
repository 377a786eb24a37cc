"""What the clouds of tests/round_clouds.py hold (conditions on the inputs of
tests/test_gpu_round_clouds.py; no GPU): the window lengths at which the tiled kernel's
candidate test and drain rounds change path."""
import numpy as np
import pytest

import round_clouds

oracle = pytest.importorskip("oracle.pyoracle")


@pytest.fixture(scope="module")
def calls():
    out = {}
    for name in round_clouds.NAMES:
        case = round_clouds.make(name, tdensity=2)
        out[name] = round_clouds.windows(case, oracle.derive(case.case_def()))
    return out


def _lengths(cs):
    return np.concatenate([np.concatenate([c["la"], c["lb"]]) for c in cs])


def test_sizes(calls):
    for name in round_clouds.NAMES:
        assert round_clouds.make(name).np <= 20000


def test_every_block_count_of_the_last_group(calls):
    """Every residue mod 8 among windows in [97, 128] (the fourth group of one round) and in
    [129, 192] (a second round), in each cloud's union and in the patch cloud alone."""
    for cs in (calls["patch"], calls["even"] + calls["patch"]):
        w = _lengths(cs)
        for lo, hi in ((97, 128), (129, 192)):
            got = set(np.unique(w[(w >= lo) & (w <= hi)] % 8).tolist())
            assert got == set(range(8)), (lo, hi, got)


def test_even_cloud_sits_on_the_round_limit(calls):
    w = _lengths(calls["even"])
    w = w[w > 0]
    assert 110 <= np.median(w[w > 60]) <= 140
    assert (w <= 128).any() and (w > 128).any()


def test_long_windows(calls):
    w = _lengths(calls["patch"])
    assert ((w > 192) & (w <= 256)).any()
    assert (w > 384).any()


def test_wave_with_windows_on_both_sides_of_128(calls):
    for name in round_clouds.NAMES:
        found = 0
        for c in calls[name]:
            m = np.maximum(c["la"], c["lb"])
            for wv in (0, 1):
                mw = m[c["wave"] == wv]
                if len(mw) and (mw > 128).any() and ((mw <= 128) & (mw > 0)).any():
                    found += 1
        assert found >= 1, name


def test_window_ends_on_the_segments_last_record(calls):
    below = at = 0
    for c in calls["patch"]:
        if c["atend"].any():
            if c["segn"] == round_clouds.TCAP:
                at += 1
            elif c["segn"] < round_clouds.TCAP:
                below += 1
    assert below >= 1 and at >= 1, (below, at)


def test_short_item(calls):
    for name in round_clouds.NAMES:
        assert min(c["n"] for c in calls[name]) < 64, name
