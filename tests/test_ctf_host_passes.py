"""The phase flip's passes (csrc/ralign_ctf.h: pf_particle, pf_fft, the butterflies and the multiplier) compiled for the HOST and
run as one sequential thread: the same index algebra and arithmetic the kernel runs, checked against the float64 statement
(ctf.flip_reference) without a GPU -- odd and even boxes, both pads, radices 2 / 3 / 4 / 5 and direct stages of 7 and 13,
batches that do not divide the rows / columns."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build, ctf

CSRC = os.path.join(build.HERE, "csrc")

HARNESS = r"""
#include "ralign_ctf.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace ralign;
// argv: nx pad nb n; stdin: n*nx*nx image floats then n*9 table floats; stdout: the flipped images
int main(int argc, char **argv)
{
    const int nx = atoi(argv[1]), pad = atoi(argv[2]), nb = atoi(argv[3]), n = atoi(argv[4]);
    PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nrad == 0 && pl.P > 1) return 2;
    pl.nb = nb;
    std::vector<float> img((size_t)n * nx * nx), tab((size_t)n * 9);
    if (fread(img.data(), 4, img.size(), stdin) != img.size() || fread(tab.data(), 4, tab.size(), stdin) != tab.size()) return 3;
    std::vector<float2> tw(pl.P), work((size_t)2 * nb * pl.P), blk((size_t)nx * pl.H);
    for (int t = 0; t < pl.P; t++) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / pl.P), (float)sin(-2.0 * M_PI * t / pl.P));
    const PfCtx cx{0, 1};
    for (int p = 0; p < n; p++)
        pf_particle(cx, &img[(size_t)p * nx * nx], pf_ctf_constants(&tab[(size_t)p * 9], nx, pl.P), pl, blk.data(), work.data(), tw.data());
    fwrite(img.data(), 4, img.size(), stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("pfhost")
    src, exe = str(d / "pfhost.cpp"), str(d / "pfhost")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "-O1", "-std=c++17", "-I" + CSRC, "-o", exe, src])
    return exe


@pytest.mark.parametrize("nx,pad,nb,n", [(8, 1, 3, 2), (9, 0, 2, 2), (13, 1, 4, 1), (14, 0, 4, 2), (26, 1, 5, 2), (45, 1, 7, 1),
                                         (49, 0, 3, 1), (30, 1, 32, 1), (65, 1, 6, 1)])
def test_host_passes_match_the_float64_statement(harness, nx, pad, nb, n):
    rng = np.random.default_rng(nx * 7 + pad)
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    t = np.zeros((n, 9), np.float32)
    t[:, 0] = nx * rng.choice([1, 2], n)
    t[:, 1] = rng.uniform(1, 4, n)
    t[:, 2] = rng.uniform(5000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(0, 3000, n)
    t[:, 4] = rng.uniform(-90, 90, n)
    t[:, 5], t[:, 6], t[:, 7] = 300, 2.7, 0.1
    t[:, 8] = rng.uniform(0, 40, n)
    out = subprocess.run([harness, str(nx), str(pad), str(nb), str(n)], input=x.tobytes() + t.tobytes(), stdout=subprocess.PIPE,
                         check=True).stdout
    got = np.frombuffer(out, np.float32).reshape(n, nx, nx)
    ref = ctf.flip_reference(x, t, pad=bool(pad))
    for i in range(n):
        assert np.abs(got[i] - ref[i]).max() <= 1e-5 * np.abs(ref[i]).max()

