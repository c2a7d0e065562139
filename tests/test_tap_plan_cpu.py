"""The containment rule behind search_fused_kernel's tap source (ra_l1_tap_rule / Engine.search_l1_tap_rings): the short rings may
read their bilinear taps from the particle's image in global memory -- which has no zero border -- only if no tap of any sample
can leave the image, for every search offset and every shift state the window rule admits.

The rule is restated here in numpy on cryo_ralib_amd.geometry's ring table and held against a brute-force enumeration of every
sample position of every ring: the four corner states +-mashi, a fractional state just inside the window, every search offset.
Every ring the rule admits keeps all four taps inside [1, nx]; the first ring it refuses really has a tap outside.  The library's
own rule (host code of the planner, no device) must give the same setting.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

from cryo_ralib_amd import api, geometry

# (nx, ou, xr): the headline; a wider window; a box tight around the rings (mashi = 1); a window so wide that not even the
# innermost ring qualifies; the smallest geometry the fused plan accepts with rings of 128 samples
GEOMETRIES = [(90, 36, 3), (90, 36, 5), (76, 36, 3), (42, 4, 16), (48, 20, 1)]
IDS = ["%d-%d-xr%d" % g for g in GEOMETRIES]


def rings_of(ou):
    numr = geometry.numrinit(1, ou, 1)
    return [(numr[3 * i], numr[3 * i + 2]) for i in range(len(numr) // 3)]        # (radius, samples)


def rule_admits(nx, ou, xr, yr, r):
    """the rule as integers: cn - mashi - ceil(xr) - r >= 1 and cn + mashi + ceil(xr) + r + 1 <= nx, and the same in y"""
    cn, mashi = nx // 2 + 1, abs(nx // 2 + 1 - ou - 2)
    ax, ay = mashi + math.ceil(xr), mashi + math.ceil(yr)
    return cn - ax - r >= 1 and cn + ax + r + 1 <= nx and cn - ay - r >= 1 and cn + ay + r + 1 <= nx


def rule_setting(nx, ou, xr, yr):
    """all or nothing per engine: the largest T of (128, 64) whose rings of at most T samples all qualify"""
    for T in (128, 64):
        if all(rule_admits(nx, ou, xr, yr, r) for r, n in rings_of(ou) if n <= T):
            return T
    return 0


def sample_offsets(r, n):
    """alrl_ms: first-quadrant (sinf, cosf) * r in float32, mirrored into the four quadrants"""
    lt = n // 4
    fi = (np.arange(lt, dtype=np.float64) * (2 * math.atan(1.0) / lt)).astype(np.float32)
    x, y = np.sin(fi).astype(np.float32) * np.float32(r), np.cos(fi).astype(np.float32) * np.float32(r)
    return np.concatenate([x, y, -x, -y]), np.concatenate([y, -x, -y, x])


def tap_extent(nx, ou, xr, r, n):
    """(lowest, highest) one-based tap index over every sample of the ring, every search offset and the states below; the taps of
    a sample at (x, y) are columns int(x), int(x) + 1 and rows int(y), int(y) + 1"""
    cn = nx // 2 + 1
    mashi = np.float32(cn - ou - 2)
    inside = np.float32(-6.9999995) if mashi >= 7 else np.nextafter(-mashi, np.float32(0))
    states = [(mashi, mashi), (mashi, -mashi), (-mashi, mashi), (-mashi, -mashi), (inside, inside), (np.float32(0), np.float32(0))]
    sh = geometry.shift_list(xr, xr, 1.0)
    dx, dy = sample_offsets(r, n)
    lo, hi = 10 ** 9, -10 ** 9
    for sx, sy in states:
        for ox, oy in sh:
            # the kernel's order: ((cnx + state) + offset) + sample, all float32
            x = ((np.float32(cn) + sx) + np.float32(ox)) + dx
            y = ((np.float32(cn) + sy) + np.float32(oy)) + dy
            ix, iy = np.floor(x).astype(int), np.floor(y).astype(int)
            lo = min(lo, ix.min(), iy.min())
            hi = max(hi, ix.max() + 1, iy.max() + 1)
    return lo, hi


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return api.load_library()


@pytest.mark.parametrize("nx,ou,xr", GEOMETRIES, ids=IDS)
def test_admitted_rings_keep_every_tap_inside_and_the_first_refused_one_does_not(nx, ou, xr):
    rings = rings_of(ou)
    refused = [(r, n) for r, n in rings if not rule_admits(nx, ou, xr, xr, r)]
    for r, n in rings:
        if rule_admits(nx, ou, xr, xr, r):
            lo, hi = tap_extent(nx, ou, xr, r, n)
            assert lo >= 1 and hi <= nx, (r, n, lo, hi)
    if refused:
        r, n = refused[0]
        lo, hi = tap_extent(nx, ou, xr, r, n)
        assert lo < 1 or hi > nx, (r, n, lo, hi)
    else:
        # every ring of the geometry qualifies: the rule is monotone in r, so the ring one pixel beyond the last admitted
        # radius is the first refused one
        r = max(r for r, _ in rings)
        while rule_admits(nx, ou, xr, xr, r):
            r += 1
        lo, hi = tap_extent(nx, ou, xr, r, 256)
        assert lo < 1 or hi > nx, (r, lo, hi)


def test_the_rule_at_the_headline_admits_radius_32():
    """cn 46, mashi 8, xr 3: r <= 32, so every ring of up to 128 samples (radius <= 20) qualifies"""
    assert rule_admits(90, 36, 3, 3, 32) and not rule_admits(90, 36, 3, 3, 33)
    assert max(r for r, n in rings_of(36) if n <= 128) == 20
    assert rule_setting(90, 36, 3, 3) == 128


@pytest.mark.parametrize("nx,ou,xr", GEOMETRIES, ids=IDS)
def test_library_rule_is_the_restated_one(lib, nx, ou, xr):
    got = lib.ra_l1_tap_rule(nx, 1, ou, 1, float(xr), float(xr))
    assert got == rule_setting(nx, ou, xr, xr)
    # 48 / 20 / 1: cn 25, mashi 3 admits r <= 18, short of the 128-sample rings (radius 11 .. 20); those of 64 end at radius 10
    assert got == {(90, 36, 3): 128, (90, 36, 5): 128, (76, 36, 3): 128, (42, 4, 16): 0, (48, 20, 1): 64}[(nx, ou, xr)]


def planner_takes_the_resident_search(lib, monkeypatch, nx, ou, xr, nref=1):
    """the planner's own answer, through its device-free size estimate (ra_legacy_bytes, tests/test_plan_cpu.py): the workspace of
    a geometry the particle-resident search takes differs from the one it is charged with that search switched off"""
    cfg = api.AlignConfig(512, nref, nx, ou, 0, 1.0, float(xr), float(xr))
    monkeypatch.delenv("RALIGN_FUSED", raising=False)
    on = lib.ra_legacy_bytes(512, ctypes.byref(cfg))
    monkeypatch.setenv("RALIGN_FUSED", "0")
    off = lib.ra_legacy_bytes(512, ctypes.byref(cfg))
    monkeypatch.delenv("RALIGN_FUSED")
    return on != off


def test_smallest_fused_geometry_with_rings_of_128_samples(lib, monkeypatch):
    """48 / 20 / 1 is taken by the fused plan (rings end at 128 samples: build_fused_plan's shortest maxrin); with rings that end at
    64 samples it is not, and the rule's answer there concerns no kernel"""
    assert rings_of(20)[-1][1] == 128
    assert planner_takes_the_resident_search(lib, monkeypatch, 48, 20, 1)
    ou = 20
    while rings_of(ou)[-1][1] == 128:
        ou -= 1
    assert rings_of(ou)[-1][1] == 64
    assert not planner_takes_the_resident_search(lib, monkeypatch, 48, ou, 1)


def test_anisotropic_window_and_the_step_from_128_to_64(lib):
    """the y range alone can refuse a setting; when the 128-sample rings fail and the shorter ones hold, the setting is 64"""
    # 90 / 36: rings of 128 samples end at radius 20, those of 64 at 10; mashi 8.  cn + mashi + yr + r + 1 <= 90 with r = 20
    # holds up to yr = 15, with r = 10 up to yr = 25
    assert rule_setting(90, 36, 3, 15) == 128 and rule_setting(90, 36, 3, 16) == 64 and rule_setting(90, 36, 3, 26) == 0
    for yr in (15, 16, 25, 26):
        assert lib.ra_l1_tap_rule(90, 1, 36, 1, 3.0, float(yr)) == rule_setting(90, 36, 3, yr)
    assert lib.ra_l1_tap_rule(90, 0, 36, 1, 3.0, 3.0) < 0          # bad ring arguments
