"""The device-free size estimate (ra_legacy_bytes: plan_workspace behind pre_align_size_check) over a grid of geometries that
crosses every boundary of the search plan -- boxes 93 | 94 and 140 | 141, outer radii 36 | 37, 39 | 40 | 41 and 60 | 61, references
14 | 15, 16 | 17 and 127 | 128 -- under the default environment and under every switch the estimate reads, byte for byte against
tests/golden/plan_bytes.npz.  The fixture was recorded from the library BEFORE the planner was gathered into ralign_plan.h
(tests/golden/make_plan_bytes.py), so the test holds the planner to the answers of the code it replaced; the switches are set
one after the other inside one process, which also shows that the library reads them at every call.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from cryo_ralib_amd import api

BOXES = [48, 64, 76, 90, 93, 94, 100, 112, 128, 140, 141, 160, 200, 256]
RADII = [9, 20, 25, 30, 36, 37, 39, 40, 41, 50, 60, 61, 70, 88, 120]
NREFS = [1, 2, 10, 14, 15, 16, 17, 50, 100, 127, 128]
RANGES = [1, 3]
STEPS = [1.0, 0.5]
SBJ_NUM = 512
# (switch, value); None: the default environment.  Two of the settings move no byte count anywhere on this grid and are rows that
# must STAY equal to the default, not coverage of their switch: RALIGN_TILED=1 (the estimate never knew the forced tiled plan; the
# row fails if resident_expected comes to share the engine's tiled_class outright) and RALIGN_GCCF_SPLIT=0 (it only picks the chunk
# size when the caller gives none, and ra_legacy_bytes always gives one).
SETTINGS = [None, ("RALIGN_GENERIC", "1"), ("RALIGN_FUSED", "0"), ("RALIGN_TILED", "0"), ("RALIGN_TILED", "1"), ("RALIGN_PAIR", "0"),
            ("RALIGN_SOLO", "0"), ("RALIGN_CROP", "0"), ("RALIGN_GCCF_SPLIT", "0"), ("RALIGN_REFINE_GM", "1")]
# everything the planner reads: none of it may leak in from the environment of the run
SWITCHES = ["RALIGN_GENERIC", "RALIGN_FUSED", "RALIGN_TILED", "RALIGN_PAIR", "RALIGN_SOLO", "RALIGN_DUO", "RALIGN_TCROP", "RALIGN_CROP",
            "RALIGN_TIGHT_RINGS", "RALIGN_GCCF_SPLIT", "RALIGN_GCCF_TM", "RALIGN_REFINE_GM"]


def key_of(setting):
    return "default" if setting is None else "%s=%s" % setting


def grid():
    """[n][5] (box, outer radius, references, range, step) of every configuration whose particle stays inside the image
    (ra_create's rule: last_ring + range <= (nx - 1) / 2 in integers)"""
    rows = [(nx, ou, nref, xr, ts) for nx in BOXES for ou in RADII for nref in NREFS for xr in RANGES for ts in STEPS
            if ou + xr <= (nx - 1) // 2]
    return np.array(rows, np.float64)


def plan_bytes(lib, cfgs):
    out = np.zeros(len(cfgs), np.uint64)
    for i, (nx, ou, nref, xr, ts) in enumerate(cfgs):
        c = api.AlignConfig(SBJ_NUM, int(nref), int(nx), int(ou), 0, float(ts), float(xr), float(xr))
        out[i] = lib.ra_legacy_bytes(SBJ_NUM, ctypes.byref(c))
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return api.load_library()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "plan_bytes.npz"))


def test_the_grid_is_the_recorded_one(golden):
    cfgs = grid()
    assert len(cfgs) == 5874
    np.testing.assert_array_equal(cfgs, golden["configs"])
    assert sorted(golden.files) == sorted(["configs"] + [key_of(s) for s in SETTINGS])


@pytest.mark.parametrize("setting", SETTINGS, ids=[key_of(s) for s in SETTINGS])
def test_size_estimate_is_the_recorded_one(setting, lib, golden, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if setting:
        monkeypatch.setenv(*setting)
    got = plan_bytes(lib, grid())
    want = golden[key_of(setting)]
    assert not (got == np.uint64(2 ** 64 - 1)).any()           # (size_t)-1: bad geometry -- none in the grid
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d differ, first: config %s gives %d, recorded %d" % (
        bad.size, len(got), grid()[bad[0]], got[bad[0]], want[bad[0]])


def test_the_switches_are_read_at_every_call(lib, golden, monkeypatch):
    """one library, one process: the estimate follows a switch that is set and removed again between two calls"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    cfgs = grid()
    moved = np.flatnonzero(golden["default"] != golden["RALIGN_FUSED=0"])[:50]
    assert moved.size > 0
    monkeypatch.setenv("RALIGN_FUSED", "0")
    np.testing.assert_array_equal(plan_bytes(lib, cfgs[moved]), golden["RALIGN_FUSED=0"][moved])
    monkeypatch.delenv("RALIGN_FUSED")
    np.testing.assert_array_equal(plan_bytes(lib, cfgs[moved]), golden["default"][moved])
