"""The preprocessing passes (csrc/ralign_prep.h: pp_normalize_image with its reduction order, pp_filter_particle with the
multiplier table) compiled for the HOST and run as one sequential thread: the same index algebra and arithmetic the kernels run,
checked against the float64 statement (prep.normalize / prep.fourier_filter, backend="numpy") without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build, prep

CSRC = os.path.join(build.HERE, "csrc")

HARNESS = r"""
#include "ralign_prep.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace ralign;
// norm nx R ramp invert nt n: stdin n*nx*nx image floats; stdout the images, then n*5 statistics doubles
// filt nx pad nb n lp_kind lp_a lp_b hp_kind hp_a hp_b: stdin n*nx*nx image floats; stdout the images
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "norm") && argc == 8) {
        const int nx = atoi(argv[2]), ramp = atoi(argv[4]), invert = atoi(argv[5]), nt = atoi(argv[6]), n = atoi(argv[7]);
        PpGeom g;
        if (!pp_make_geom(nx, atof(argv[3]), g)) return 4;
        std::vector<float> img((size_t)n * nx * nx);
        std::vector<double> st((size_t)n * 5);
        if (fread(img.data(), 4, img.size(), stdin) != img.size()) return 3;
        const PpHostCtx cx{nt};
        for (int p = 0; p < n; p++) {
            float *x = &img[(size_t)p * nx * nx];
            pp_normalize_image(cx, x, x, g, ramp, invert ? -1.0 : 1.0, &st[(size_t)p * 5], true);
        }
        fwrite(img.data(), 4, img.size(), stdout);
        fwrite(st.data(), 8, st.size(), stdout);
        return 0;
    }
    if (!strcmp(argv[1], "filt") && argc == 12) {
        const int nx = atoi(argv[2]), pad = atoi(argv[3]), nb = atoi(argv[4]), n = atoi(argv[5]);
        const PpFilter f{atoi(argv[6]), atoi(argv[9]), atof(argv[7]), atof(argv[8]), atof(argv[10]), atof(argv[11])};
        PfPlan pl = pf_make_plan(nx, pad);
        if (pl.nrad == 0 && pl.P > 1) return 4;
        pl.nb = nb;
        std::vector<float> img((size_t)n * nx * nx), tab((size_t)pl.H * pl.H);
        if (fread(img.data(), 4, img.size(), stdin) != img.size()) return 3;
        for (int ay = 0; ay < pl.H; ay++)
            for (int ix = 0; ix < pl.H; ix++) tab[(size_t)ix * pl.H + ay] = pp_filter_gain(f, pl.P, ay, ix);
        std::vector<float2> tw(pl.P), work((size_t)2 * nb * pl.P), blk((size_t)nx * pl.H);
        for (int t = 0; t < pl.P; t++) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / pl.P), (float)sin(-2.0 * M_PI * t / pl.P));
        const PfCtx cx{0, 1};
        for (int p = 0; p < n; p++) pp_filter_particle(cx, &img[(size_t)p * nx * nx], tab.data(), pl, blk.data(), work.data(), tw.data());
        fwrite(img.data(), 4, img.size(), stdout);
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("pphost")
    src, exe = str(d / "pphost.cpp"), str(d / "pphost")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "-O1", "-std=c++17", "-I" + CSRC, "-o", exe, src])
    return exe


def particles(nx, n, seed):
    """100 + 7 noise + a plane: the mean and the plane are large against the noise, so cancellation is real"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:nx, 0:nx] - nx // 2
    x = 100.0 + 7.0 * rng.standard_normal((n, nx, nx))
    x += rng.uniform(-0.5, 0.5, (n, 1, 1)) * u + rng.uniform(-0.5, 0.5, (n, 1, 1)) * v
    return x.astype(np.float32)


NORM_CASES = [(nx, R, ramp, invert, nt)
              for nx, nt in ((4, 64), (5, 7), (9, 100), (33, 192), (64, 250))
              for R, ramp, invert in ((1.0, 1, 0), (nx / 2.0, 1, 1), (0.5 + nx / 4.0, 0, 0), (0.5 + nx / 4.0, 1, 0))]


@pytest.mark.parametrize("nx,R,ramp,invert,nt", NORM_CASES)
def test_host_normalise_passes_match_the_float64_statement(harness, nx, R, ramp, invert, nt):
    n = 2
    x = particles(nx, n, nx * 11 + nt)
    out = subprocess.run([harness, "norm", str(nx), repr(R), str(ramp), str(invert), str(nt), str(n)], input=x.tobytes(),
                         stdout=subprocess.PIPE, check=True).stdout
    got = np.frombuffer(out[:x.nbytes], np.float32).reshape(n, nx, nx)
    st = np.frombuffer(out[x.nbytes:], np.float64).reshape(n, 5)
    ref, rst = prep.normalize(x, R, ramp=bool(ramp), invert=bool(invert), stats=True, backend="numpy")
    scale = np.abs(x).max()
    tol = np.array([scale, scale / (nx / 2.0), scale / (nx / 2.0), scale, scale]) * 1e-12
    assert np.all(np.abs(st - rst) <= tol), (st - rst)
    r32 = ref.astype(np.float32)
    for i in range(n):
        bar = 2.0 ** -23 * np.abs(ref[i]) + 1e-10 * scale / rst[i, 4]
        assert np.all(np.abs(got[i].astype(np.float64) - r32[i]) <= bar)


def test_host_normalise_order_depends_on_nt_only_in_the_last_bits(harness):
    """two contexts sum in different orders: the statistics agree to double rounding, far below float32 accumulation (1e-6)"""
    nx, n = 33, 1
    x = particles(nx, n, 5)
    st = []
    for nt in (64, 250):
        out = subprocess.run([harness, "norm", str(nx), "10.5", "1", "0", str(nt), str(n)], input=x.tobytes(), stdout=subprocess.PIPE,
                             check=True).stdout
        st.append(np.frombuffer(out[x.nbytes:], np.float64))
    assert np.abs(st[0] - st[1]).max() <= 1e-12 * np.abs(x).max()


def test_host_normalise_sigma_zero_and_non_finite(harness):
    nx = 9
    x = particles(nx, 3, 2)
    x[0] = 3.0
    x[1, 4, 4] = np.inf                       # inside the disc: no sum over B sees it
    out = subprocess.run([harness, "norm", str(nx), "3", "0", "1", "100", "3"], input=x.tobytes(), stdout=subprocess.PIPE, check=True).stdout
    got = np.frombuffer(out[:x.nbytes], np.float32).reshape(3, nx, nx)
    st = np.frombuffer(out[x.nbytes:], np.float64).reshape(3, 5)
    assert np.all(got[0] == 0.0) and st[0, 4] == 0.0 and st[0, 3] == 3.0
    assert np.all(np.isnan(got[1])) and np.all(np.isnan(st[1]))
    ref = prep.normalize(x[2:], 3, invert=True, backend="numpy")[0]
    assert np.abs(got[2] - ref).max() <= 1e-6 * np.abs(ref).max()


FILTERS = [(("tanl", 0.2, 0.1), None), (("gauss", 0.15), None), (("tanl", 0.3, 0.2), ("gauss", 0.03)), (None, ("tanl", 0.05, 0.5))]


@pytest.mark.parametrize("nx,pad,nb,n,which", [(8, 1, 3, 2, 0), (8, 0, 5, 1, 2), (9, 0, 2, 2, 1), (9, 1, 4, 1, 3), (14, 0, 4, 2, 2),
                                               (14, 1, 3, 1, 0), (26, 1, 5, 2, 3), (26, 0, 7, 1, 1), (45, 1, 7, 1, 2), (45, 0, 4, 1, 0),
                                               (49, 0, 3, 1, 3), (49, 1, 6, 1, 1)])
def test_host_filter_passes_match_the_float64_statement(harness, nx, pad, nb, n, which):
    lowpass, highpass = FILTERS[which]
    lp, hp = prep._check_term(lowpass, "lowpass"), prep._check_term(highpass, "highpass")
    rng = np.random.default_rng(nx * 7 + pad)
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    argv = [harness, "filt", str(nx), str(pad), str(nb), str(n)] + [repr(v) for v in lp + hp]
    out = subprocess.run(argv, input=x.tobytes(), stdout=subprocess.PIPE, check=True).stdout
    got = np.frombuffer(out, np.float32).reshape(n, nx, nx)
    ref = prep.fourier_filter(x, lowpass, highpass, pad=bool(pad), backend="numpy")
    for i in range(n):
        assert np.abs(got[i] - ref[i]).max() <= 1e-5 * np.abs(ref[i]).max()
