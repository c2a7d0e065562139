"""The size-generic polar stage without a GPU (cases and reference: tests/polar_cases.py):
  (a) build_zone_plan (csrc/ralign_zone.h) compiled for the HOST: the plan of every zone case -- zones, holes, ring lengths per quad --
      has the edge its case claims, and every tap zone_bilinear can form (every sample of every ring of a zone, every search offset,
      integer and fractional centres) resolves through rowtab to a stored float whose pixtab entry names exactly the source pixel.
      The harness refuses a tap outside a table (exit code 4, the first offending zone / ring / sample / offset) instead of reading it;
  (b) the float64 reference against closed forms (constant image, linear ramp), and the CPU oracle against the reference in the
      per-ring unit: finite, printed, kept in polar_cases.ORACLE_RATIO for tests/test_gpu_polar_edges.py;
  (c) the window rule and the live-offset lists of the edge cases restated from geometry.search_range."""
import math
import os
import subprocess

import numpy as np
import pytest

import polar_cases as pc
from cryo_ralib_amd import build, geometry

CSRC = os.path.join(build.HERE, "csrc")

HARNESS = r"""
#include <cstring>
#include "ralign_geom.h"
#include "ralign_plan.h"
#include "ralign_zone.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
using namespace ralign;
// argv: nx ir ou rs xr yr step check.  stdout: the plan; exit 0 fine, 2 bad geometry, 3 no plan, 4 a tap outside a table or at the wrong pixel
int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    const int nx = atoi(argv[1]), ir = atoi(argv[2]), ou = atoi(argv[3]), rs = atoi(argv[4]), check = atoi(argv[8]);
    const float xr = (float)atof(argv[5]), yr = (float)atof(argv[6]), step = (float)atof(argv[7]);
    Geometry g;
    if (!build_rings(g, nx, ir, ou, rs) || !build_shifts(g, xr, yr, step)) return 2;
    if (g.maxrin <= 1024) align_ring_quads(g);                                        // ra_create, size-generic class
    const int S = (int)std::ceil(std::max(g.nkx, g.nky) * g.step - 1e-6);             // setup_zones
    std::set<int> lens;
    int n_qtab = 0;                                                                    // one first-quadrant table per ring length
    for (int i = 0; i < g.nring; i++) if (lens.insert(g.numr[3 * i + 2]).second) n_qtab += g.numr[3 * i + 2] / 4;
    ZonePlanHost zp;
    const bool ok = build_zone_plan(g, S, RA_ZONE_NW, n_qtab, zp);
    printf("plan ok %d S %d n_qtab %d nring %d maxrin %d nzone %d nquad_total %d lds_bytes %zu\n", (int)ok, S, n_qtab, g.nring, g.maxrin,
           (int)zp.zones.size(), zp.nquad_total, zp.lds_bytes);
    if (!ok) return 3;
    for (size_t z = 0; z < zp.zones.size(); z++) {
        const ZoneDesc &zd = zp.zones[z];
        int holes = 0;
        for (int r = 0; r < zd.nrow; r++) { const int2 t = zp.rowtab[zd.row_off + r]; holes += t.x != t.y; }
        printf("zone %d ring0 %d nquad %d quad0 %d npix %d nrow %d H %d holes %d\n", (int)z, zd.ring0, zd.nquad, zd.quad0, zd.npix, zd.nrow, zd.H, holes);
        for (int q = 0; q < zd.nquad; q++) {
            printf("quad %d zone %d len", zd.quad0 + q, (int)z);
            for (int i = zd.ring0 + 4 * q; i < std::min(zd.ring0 + 4 * q + 4, g.nring); i++) printf(" %d", g.numr[3 * i + 2]);
            printf("\n");
        }
    }
    if (!check) return 0;
    // offsets: every integer of -S .. S and every entry of the offset list; centres: cnx + {0, 1/2, the step's fraction, just below 1}
    std::set<float> offs, fr;
    for (int o = -S; o <= S; o++) offs.insert((float)o);
    for (float v : g.shift_x) offs.insert(v);
    for (float v : g.shift_y) offs.insert(v);
    const float cn = (float)(nx / 2 + 1);
    fr.insert(cn); fr.insert(cn + 0.5f); fr.insert(cn + (step - std::floor(step))); fr.insert(std::nextafterf(cn + 1.0f, 0.0f));
    long long ntap = 0;
    for (size_t z = 0; z < zp.zones.size(); z++) {
        const ZoneDesc &zd = zp.zones[z];
        const int2 *rt = &zp.rowtab[zd.row_off];
        const int *pt = &zp.pixtab[zd.pix_off];
        for (int i = zd.ring0; i < std::min(zd.ring0 + 4 * zd.nquad, g.nring); i++) {
            const int kc = g.numr[3 * i + 1] - 1, n = g.numr[3 * i + 2];
            for (int j = 0; j < n; j++) {
                const float px = g.samp_dx[kc + j], py = g.samp_dy[kc + j];
                for (float cxf : fr) for (float cyf : fr) {
                    const int cxi = (int)cxf, cyi = (int)cyf;
                    for (float oy : offs) for (float ox : offs) {
                        // zone_bilinear's addressing, in float indices
                        const float cx = cxf + ox, cy = cyf + oy;
                        const float xo = px + cx, yo = py + cy;
                        const int ix = (int)xo, iy = (int)yo;
                        const int rx = ix - cxi, row = iy - (cyi - zd.H);
                        const bool left = rx < 0;
                        for (int t = 0; t < 4; t++) {
                            const int ddx = t & 1, ddy = t >> 1, rr = row + ddy;
                            long long idx = -1;
                            int why = 0;
                            if (rr < 0 || rr > zd.nrow) why = 1;                    // the row table has nrow + 1 entries
                            else {
                                idx = (long long)(left ? rt[rr].x : rt[rr].y) + rx + ddx;
                                if (idx < 0 || idx >= zd.npix) why = 2;
                                else {
                                    const int code = pt[idx], dy = code >> 16, dx = (int)(short)(code & 0xffff);
                                    if (dx != rx + ddx || dy != iy - cyi + ddy) why = 3;
                                }
                            }
                            if (why) {
                                printf("BAD why %d zone %d ring %d sample %d ox %g oy %g cx %.9g cy %.9g tap %d row %d idx %lld\n", why, (int)z, i, j, ox, oy,
                                       cxf, cyf, t, rr, idx);
                                return 4;
                            }
                            ntap++;
                        }
                    }
                }
            }
        }
    }
    printf("taps %lld\n", ntap);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("zonehost")
    src, exe = str(d / "zonehost.cpp"), str(d / "zonehost")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + CSRC, "-o", exe, src])
    return exe


def run_plan(harness, nx, ou, ir, rs, xr, yr, step, check=0):
    """-> (exit code, header dict, zones [dict], quads {quad index: (zone, [ring lengths])}, text)"""
    r = subprocess.run([harness] + [str(v) for v in (nx, ir, ou, rs, xr, yr, step, check)], stdout=subprocess.PIPE, universal_newlines=True)
    head, zones, quads = {}, [], {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "plan":
            head = {w[i]: int(w[i + 1]) for i in range(1, len(w), 2)}
        elif w[0] == "zone":
            zones.append({w[i]: int(w[i + 1]) for i in range(2, len(w), 2)})
        elif w[0] == "quad":
            quads[int(w[1])] = (int(w[3]), [int(v) for v in w[5:]])
    return r.returncode, head, zones, quads, r.stdout


def plan_of(harness, case, check=0):
    _, nx, ou, ir, rs, xr, yr, step = case[:8]
    return run_plan(harness, nx, ou, ir, rs, xr, yr, step, check)


ZONE_GEOMETRIES = ["two-zones", "three-zones-1024", "mixed-256-512", "ragged-last-quad", "half-pixel", "odd-box", "edge-windows"]


@pytest.mark.parametrize("name", ZONE_GEOMETRIES)
def test_every_tap_of_every_zone_names_its_source_pixel(harness, name):
    rc, head, zones, quads, text = plan_of(harness, pc.BY_NAME[name], check=1)
    summary = [l for l in text.splitlines() if not l.startswith("quad")]
    print("%s: %s" % (name, " | ".join(summary)))
    assert rc == 0, text[-400:]
    assert head["ok"] == 1 and head["nzone"] == len(zones) >= 1
    # the zones tile the quads from the outside in, and every pixel list fits the LDS the plan asks for
    assert zones[0]["ring0"] + 4 * zones[0]["nquad"] >= head["nring"] and zones[-1]["quad0"] == 0 and zones[-1]["ring0"] == 0
    for a, b in zip(zones, zones[1:]):
        assert b["quad0"] + b["nquad"] == a["quad0"] and a["ring0"] == 4 * a["quad0"]
    assert sorted(quads) == list(range(head["nquad_total"])) and head["nquad_total"] == (head["nring"] + 3) // 4
    assert head["lds_bytes"] <= 160 * 1024 - 1024
    assert int(text.splitlines()[-1].split()[1]) > 0


def test_the_cases_reach_the_edges_they_claim(harness):
    P = {n: plan_of(harness, pc.BY_NAME[n]) for n in ZONE_GEOMETRIES}
    # two-zones: two zones at ou = 88 of a 200 box and xr = 2, one at ou = 87; the outer zone (first in the plan: quad0 > 0) stores
    # rows with a hole (left and right segment) and rows without one
    rc, head, zones, quads, _ = P["two-zones"]
    assert head["nzone"] == 2 and head["maxrin"] == 1024
    assert zones[0]["quad0"] > 0 and 0 < zones[0]["holes"] < zones[0]["nrow"]
    assert run_plan(harness, 200, 87, 1, 1, 2, 2, 1.0)[1]["nzone"] == 1
    # three-zones-1024: three zones, rings of 1024 samples, and the quad of rings 80 .. 83 mixes 512 and 1024
    rc, head, zones, quads, _ = P["three-zones-1024"]
    assert head["nzone"] == 3 and head["maxrin"] == 1024
    assert quads[20][1] == [512, 1024, 1024, 1024]
    assert all(z["quad0"] > 0 for z in zones[:2])
    # mixed-256-512: rings of at most 256 samples inside a quad whose longest ring has 512
    rc, head, zones, quads, _ = P["mixed-256-512"]
    assert head["maxrin"] == 512
    assert any(max(l) == 512 and min(l) <= 256 for _, l in quads.values()), quads
    # ragged-last-quad: the last quad holds fewer than four rings
    rc, head, zones, quads, _ = P["ragged-last-quad"]
    assert head["nring"] % 4 != 0 and len(quads[head["nquad_total"] - 1][1]) == head["nring"] % 4
    # half-pixel: fractional offsets, S = ceil(2 * 0.5) = 1
    assert P["half-pixel"][1]["S"] == 1 and pc.BY_NAME["half-pixel"][7] == 0.5
    assert pc.BY_NAME["odd-box"][1] % 2 == 1
    for n in ZONE_GEOMETRIES:
        assert P[n][0] == 0 and P[n][1]["ok"] == 1, n


# ---------------------------------------------------------------------------------------------- (b) the reference

def test_reference_of_a_constant_image_is_dc_only():
    numr = geometry.numrinit(1, 30, 1)
    img = np.full((80, 80), 2.5)
    for interp in (pc.BIL, pc.QUADRI):
        got = pc.reference(img, np.float32(41.5), np.float32(40.25), numr, False, interp)
        want = np.zeros_like(got)
        for i in range(len(numr) // 3):
            want[numr[3 * i + 1] - 1] = 2.5 * numr[3 * i + 2]
        assert np.abs(got - want).max() < 1e-10
    # Normalize_ring of a constant image has sigma 0: the mean is the constant
    c = pc.sample64(img, np.float32(41.5), np.float32(40.25), numr)
    w = pc.ring_weights(numr)
    assert abs((c * w).sum() / w.sum() - 2.5) < 1e-12


def test_reference_of_a_linear_ramp_is_the_first_harmonic():
    """f(x, y) = a + b x + c y (1-based pixel coordinates) is reproduced exactly by the bilinear rule, so ring r of length L at
    centre (cx, cy) samples a + b cx + c cy + r (b sin t_j + c cos t_j) at the float32 angles: X0 = L (a + b cx + c cy) + b Sx + c Sy
    with the positions' own sums, and with exact angles X1 = L r (c - i b) / 2, every other bin 0.  The float32 angles are within
    an ulp of 2 pi j / L: the analytic first harmonic holds to 1e-6 of its size, the sums of the positions themselves to 1e-12"""
    numr = geometry.numrinit(1, 30, 1)
    nx = 80
    a, b, c = 0.75, 0.031, -0.017
    yy, xx = np.mgrid[1:nx + 1, 1:nx + 1].astype(np.float64)
    img = a + b * xx + c * yy
    cx, cy = np.float32(41.5), np.float32(39.75)
    got = pc.reference(img, cx, cy, numr, False)
    dx, dy = pc.ring_offsets(numr)
    x, y = (dx + cx).astype(np.float64), (dy + cy).astype(np.float64)
    for i in range(len(numr) // 3):
        r, o, L = numr[3 * i], numr[3 * i + 1] - 1, numr[3 * i + 2]
        assert abs(got[o] - (a * L + b * x[o:o + L].sum() + c * y[o:o + L].sum())) < 1e-10 * L
        scale = L * r * math.hypot(b, c) / 2
        if L >= 4:
            assert abs(got[o + 2] - L * r * c / 2) < 2e-6 * scale and abs(got[o + 3] + L * r * b / 2) < 2e-6 * scale, (i, got[o + 2:o + 4])
            rest = np.concatenate([got[o + 1:o + 2], got[o + 4:o + L]])
            assert np.abs(rest).max() < 2e-6 * scale, (i, np.abs(rest).max())
    # ... and Normalize_ring's statistics of the ramp: mean a + b cx + c cy up to the positions' sums
    cs = pc.sample64(img, cx, cy, numr)
    w = pc.ring_weights(numr)
    _, avg, sgm = pc.normalize64(cs, numr, w)
    assert abs(avg - (a + b * (x * w).sum() / w.sum() + c * (y * w).sum() / w.sum())) < 1e-12 and sgm > 0


def test_ring_ratio_judges_every_ring_on_its_own_scale():
    numr = geometry.numrinit(1, 12, 1)
    lcirc = numr[-2] + numr[-1] - 1
    ref = np.random.default_rng(5).standard_normal(lcirc)
    got = ref.copy()
    o, L = numr[3 * 1 + 1] - 1, numr[3 * 1 + 2]            # one slot of the second ring (8 samples) off by 1e-4 of that ring
    got[o + 3] += 1e-4 * np.linalg.norm(ref[o:o + L])
    ratio = pc.ring_ratio(got[None], ref[None], numr)
    assert ratio.shape == (1, 12)
    assert abs(ratio[0, 1] - 1e-4 / (pc.EPS * (1 + math.log2(L)))) < 1e-6 * ratio[0, 1] and np.delete(ratio[0], 1).max() == 0
    assert pc.worst(ratio, got[None], ref[None], numr)[1:] == (0, 1, 3)


@pytest.mark.parametrize("name", sorted({pc.geometry_key(c): c[0] for c in pc.CASES}.values(), key=pc.IDS.index))
def test_oracle_against_the_reference_ring_by_ring(name):
    """what float32 costs on these inputs, from the reference side only: the oracle's largest per-ring ratio of every case"""
    case = pc.BY_NAME[name]
    big, where, stats, finite = pc.oracle_figures(case)
    R = pc.case_reference(case)
    print("%s: oracle / reference, largest per-ring ratio %.3g at (particle, offset, ring, slot) = %s; %d of %d offsets in the window%s"
          % (name, big, where, R["inwin"].sum(), R["inwin"].size,
             "" if stats is None else "; mean rel. err %.3g, sigma rel. err %.3g; without Normalize_ring %.3g" % stats))
    assert finite and np.isfinite(big) and big > 0
    # the figure sets the GPU bar: held to generous pins above the recorded ones (0.34 - 0.40 without Normalize_ring, 16 - 81 with
    # it, where the innermost ring's DC slot carries the float32 mean), so that a reference and an oracle that drift apart -- in
    # the float32 positions, say -- cannot inflate every bar unseen
    assert big <= (200.0 if case[8] == pc.M else 1.0), big
    assert pc.ORACLE_RATIO[name] == big
    if case[8] == pc.M:
        assert np.isfinite(pc.ORACLE_STATS[name]).all() and 0 < pc.ORACLE_RAW_RATIO[name] <= 1.0
        assert pc.ORACLE_STATS[name][0] <= 2e-2 and pc.ORACLE_STATS[name][1] <= 1e-4          # recorded: 5e-3, 2.3e-5 at the most
    # cases that share the geometry share the figure
    for c in pc.CASES:
        if pc.geometry_key(c) == pc.geometry_key(case):
            pc.oracle_figures(c)
            assert pc.ORACLE_RATIO[c[0]] == big


# ---------------------------------------------------------------------------------------------- (c) the live lists

def test_windows_of_the_edge_cases():
    case = pc.BY_NAME["edge-windows"]
    _, st = pc.inputs(case)
    W = [pc.window(case, float(d[0]), float(d[1])) for d in st]
    counts = [(w[2] + w[3] + 1) * (w[4] + w[5] + 1) for w in W]
    assert [w[2:6] for w in W] == [(2, 1, 0, 2), (2, 0, 2, 0), (2, 2, 2, 2)]
    assert counts == [12, 9, 25] and [w[6] for w in W] == [False, False, True]
    assert W[2][:2] == (0.0, 0.0)                      # the state beyond mashi = 8 is reset
    inw = pc.in_window(case)
    assert inw.sum(1).tolist() == counts and inw.any() and (~inw).any()
    # live_index counts the in-window offsets in list order
    for p, w in enumerate(W):
        idx = [pc.live_index(case, w, s) for s in range(25)]
        assert sorted(i for i in idx if i >= 0) == list(range(counts[p]))
        assert [i for i in idx if i >= 0] == list(range(counts[p]))
    # ent_base holds unequal counts; 4 slices of the 9 offsets: 3 3 3 0, an empty last slice
    assert len(set(counts)) == 3 and -(-9 // 4) * 3 >= 9
    # zone-chunks: 25 and 9 offsets in the 4 slices of polar_zone_kernel (per = ceil(nlive / 4)): 7 7 7 4 and 3 3 3 0
    case = pc.BY_NAME["zone-chunks"]
    inw = pc.in_window(case)
    assert inw.sum(1).tolist() == [25, 9]
    slices = lambda nlive: [max(0, min(nlive, (ch + 1) * -(-nlive // 4)) - ch * -(-nlive // 4)) for ch in range(4)]
    assert slices(25) == [7, 7, 7, 4] and slices(9) == [3, 3, 3, 0] and 25 % 4 != 0
    # the cases with every offset in the window, whatever their states
    for n in pc.IDS:
        assert (n in pc.CENTRED_CASES) == bool(pc.in_window(pc.BY_NAME[n]).all()), n
    assert not {"edge-windows", "edge-windows-all", "zone-chunks"} & set(pc.CENTRED_CASES) and {"two-zones", "half-pixel"} <= set(pc.CENTRED_CASES)


def test_half_pixel_case_truncates_its_crop_centre():
    """polar_zone_kernel: cxf = cnx + sxi, cxi = (int)cxf.  The first particle's half-integer state survives the window rule, so
    both centres are truncated (one from above .5 of a positive, one of a negative state); the second particle's are whole"""
    case = pc.BY_NAME["half-pixel"]
    _, st = pc.inputs(case)
    cnx = np.float32(case[1] // 2 + 1)
    w = pc.window(case, float(st[0, 0]), float(st[0, 1]))
    assert w[:2] == (0.5, -0.5) and not w[6]
    cxf, cyf = cnx + np.float32(w[0]), cnx + np.float32(w[1])
    assert int(cxf) != cxf and int(cyf) != cyf and (int(cxf), int(cyf)) == (76, 75)
    w = pc.window(case, float(st[1, 0]), float(st[1, 1]))
    assert int(cnx + np.float32(w[0])) == cnx + np.float32(w[0])
    # the sampling centres of the case: whole, half, and the reference uses exactly them
    frac = pc.case_reference(case)["centre"] % 1
    assert set(np.unique(frac[0]).tolist()) == {0.0, 0.5} and set(np.unique(frac[1]).tolist()) == {0.0, 0.5}
