"""The arithmetic of rot_shift2D (csrc/ralign_xform.h: xf_trig, xf_pose, xf_mirror_col, xf_column, xf_source,
quadri_background_1b, xf_quadri_poly and its two padded front ends, the tile kernel's box placement) compiled for the HOST.
Every image is built the four ways the kernels build it:
  0. transform_kernel's: quadri_background_1b on the image itself;
  1. transform_sum_kernel's: a copy with a wrap-around border of one pixel (row stride (nx + 2) | 1) + quadri_background_wrap;
  2. transform_sum_db_kernel's: the same copy + quadri_background_wrap1;
  3. transform_sum_tile_kernel's: per 64 x 64 output tile a periodic 98 x 98 box of source pixels placed by xf_tile_origin +
     xf_quadri_poly, with the kernel's two side routes (own pixel for the background, the image itself for the unmirrored
     column 0 of an even box).  The harness refuses a tap outside the copy or the box (exit code 4) instead of reading it.
All four must give the bits of tests/golden/rot_shift2d_ref.npz (the reference tree's own text), and agree with each other on
the poses at the arithmetic's edges (xsum_cases.edge_poses).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build
from xsum_cases import edge_poses

CSRC = os.path.join(build.HERE, "csrc")
WAYS = ["quadri_background_1b", "quadri_background_wrap", "quadri_background_wrap1", "tile box + xf_quadri_poly"]

HARNESS = r"""
#include "ralign_xform.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace ralign;
// argv: nx n mirror; stdin: n*nx*nx image floats then n*3 pose floats (alpha, sx, sy); stdout: [4][n][nx][nx]
int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int nx = atoi(argv[1]), n = atoi(argv[2]), mirror = atoi(argv[3]), npix = nx * nx;
    std::vector<float> imgs((size_t)n * npix), pose((size_t)n * 3), out((size_t)4 * n * npix);
    if (fread(imgs.data(), 4, imgs.size(), stdin) != imgs.size() || fread(pose.data(), 4, pose.size(), stdin) != pose.size()) return 3;
    const int pst = (nx + 2) | 1, BB = RA_XT_BB, mstart = 1 - nx % 2;
    std::vector<float> pad((size_t)(nx + 2) * pst), box((size_t)BB * BB);
    for (int p = 0; p < n; p++) {
        const float *img = &imgs[(size_t)p * npix];
        float *o0 = &out[((size_t)0 * n + p) * npix], *o1 = &out[((size_t)1 * n + p) * npix], *o2 = &out[((size_t)2 * n + p) * npix],
              *o3 = &out[((size_t)3 * n + p) * npix];
        const XfPose ps = xf_pose(nx, pose[3 * p + 1], pose[3 * p + 2], xf_trig(pose[3 * p]), mirror);
        // 0: source column ix lands in column xf_mirror_col(ix)
        for (int iy = 0; iy < nx; iy++)
            for (int ix = 0; ix < nx; ix++) {
                const float2 s = xf_source(ps, xf_column(ps, ix), (float)iy, nx);
                o0[iy * nx + xf_mirror_col(nx, mirror, ix)] = quadri_background_1b(img, nx, nx, s.x, s.y, ix + 1, iy + 1);
            }
        // 1, 2: padded (row, col) <- pixel ((row - 1) mod nx, (col - 1) mod nx); destination column tx reads source column ix
        for (int pr = 0; pr < nx + 2; pr++)
            for (int pc = 0; pc < nx + 2; pc++)
                pad[(size_t)pr * pst + pc] = img[((pr + nx - 1) % nx) * nx + (pc + nx - 1) % nx];
        for (int iy = 0; iy < nx; iy++)
            for (int tx = 0; tx < nx; tx++) {
                const int ix = xf_mirror_col(nx, mirror, tx);
                const float2 s = xf_source(ps, xf_column(ps, ix), (float)iy, nx);
                o1[iy * nx + tx] = quadri_background_wrap(pad.data(), pst, nx, s.x, s.y, ix + 1, iy + 1);
                o2[iy * nx + tx] = quadri_background_wrap1(pad.data(), pst, nx, s.x, s.y, (float)ix + 1.0f, (float)iy + 1.0f);
            }
        // 3: per output tile, the box as transform_sum_tile_kernel stages it
        for (int ty0 = 0; ty0 < nx; ty0 += RA_XT_TS)
            for (int tx0 = 0; tx0 < nx; tx0 += RA_XT_TS) {
                const int2 org = xf_tile_origin(ps, nx, tx0, ty0);
                const int cb = xf_box_origin(org.x, nx), rb = xf_box_origin(org.y, nx);
                for (int row = 0; row < BB; row++)
                    for (int col = 0; col < BB; col++) box[row * BB + col] = img[xf_box_source(rb, row, nx) * nx + xf_box_source(cb, col, nx)];
                for (int iy = ty0; iy < ty0 + RA_XT_TS && iy < nx; iy++)
                    for (int tx = tx0; tx < tx0 + RA_XT_TS && tx < nx; tx++) {
                        const int ix = xf_mirror_col(nx, mirror, tx);
                        const float2 s = xf_source(ps, xf_column(ps, ix), (float)iy, nx);
                        const float X = s.x, Y = s.y;
                        float v;
                        if (!((X >= 1.0f) && (X < (float)(nx + 1)) && (Y >= 1.0f) && (Y < (float)(nx + 1)))) v = img[iy * nx + ix];
                        else if (mirror && tx < mstart) v = quadri_background_1b(img, nx, nx, X, Y, ix + 1, iy + 1);
                        else {
                            const int i = (int)X - org.x, j = (int)Y - org.y;          // the tap's element of the box; neighbours at +-1
                            if (i < 1 || i > BB - 2 || j < 1 || j > BB - 2) { fprintf(stderr, "tap (%d, %d) outside the box\n", i, j); return 4; }
                            v = xf_quadri_poly(&box[j * BB + i], BB, X - (int)X, Y - (int)Y);
                        }
                        o3[iy * nx + tx] = v;
                    }
            }
    }
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("xfhost")
    src, exe = str(d / "xfhost.cpp"), str(d / "xfhost")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + CSRC, "-o", exe, src])
    return exe


def four_ways(harness, imgs, poses, mirror):
    n, nx = imgs.shape[0], imgs.shape[-1]
    raw = subprocess.run([harness, str(nx), str(n), str(mirror)], input=imgs.astype(np.float32).tobytes() + poses.astype(np.float32).tobytes(),
                         stdout=subprocess.PIPE, check=True).stdout
    return np.frombuffer(raw, np.float32).reshape(4, n, nx, nx)


@pytest.mark.parametrize("mirror", [0, 1])
def test_every_way_gives_the_reference_trees_bits(harness, golden_dir, mirror):
    g = np.load(os.path.join(golden_dir, "rot_shift2d_ref.npz"))
    for k in range(int(g["ncase"])):
        img, ang, dx, dy, out = (g["%s%d" % (nm, k)] for nm in ("img", "ang", "dx", "dy", "out"))
        nx = img.shape[-1]
        got = four_ways(harness, img, np.stack([ang, dx, dy], axis=1), mirror)
        want = out.copy()
        if mirror:          # the rule of test_transform_kernel_matches_the_reference_tree_bit_for_bit
            start = 1 - nx % 2
            want[:, :, start:] = want[:, :, start:][:, :, ::-1]
        for w in range(4):
            np.testing.assert_array_equal(got[w], want, err_msg="case %d (box %d): %s" % (k, nx, WAYS[w]))


@pytest.mark.parametrize("nx", [32, 33, 91])
@pytest.mark.parametrize("mirror", [0, 1])
def test_the_ways_agree_at_the_edge_poses(harness, nx, mirror):
    poses = np.array(edge_poses(nx), np.float32)
    assert poses.shape == (14, 3)
    imgs = np.random.default_rng(1000 + nx).standard_normal((14, nx, nx)).astype(np.float32)
    got = four_ways(harness, imgs, poses, mirror)
    assert np.isfinite(got).all()
    for w in range(1, 4):
        np.testing.assert_array_equal(got[w], got[0], err_msg="box %d: %s" % (nx, WAYS[w]))
