"""The Wiener class sums and the finalize of csrc/ralign_wiener.h on the host, element by element against the float64 contract
(wiener.class_sums_reference, numpy's irfft2): the arithmetic is __host__ __device__, so one sequential thread forms the float32
num / den in the device's association (runs of L members summed in double, rounded to float, the runs of a longer class combined
in double) and runs wn_class on given sums.  The error ratios measured here set the bounds of tests/test_gpu_wiener_sums.py,
which shares this module's cases, plan formulas and comparison:

  e_num = max_e |num - num_ref| / s_j, s_j = sqrt(mean_e |num_ref_j|^2), per class j
  e_den = max_e |den - den_ref| / max(1, count_j)
  e_fin = max |img - img_ref| / sqrt(mean img_ref^2)

Measured on the host path (x86-64, -O1, no FMA contraction; the largest ratio over the classes, flipped 0 and 1, and for e_fin
over two draws of the sums), inputs as the device holds them (float32 alpha, shifts and table):

  box (P)   8 2x (16)  9 1x (9)  13 2x (26)  45 2x (90)  64 1x (64)  75 2x (150)  114 2x (228)
  e_num     4.99e-7    5.11e-7   5.92e-7     7.44e-7     6.60e-7     8.33e-7      -
  e_den     2.72e-7    1.44e-7   3.00e-7     3.09e-7     2.69e-7     3.05e-7      -
  e_fin     2.78e-7    3.81e-7   5.81e-7     7.37e-7     6.35e-7     7.65e-7      1.24e-6

e_num and e_fin carry the FFT's rounding and grow with log2 P (e_fin by 4.4x over these boxes), e_den is the float sine's error
and does not.  The x1 figures are therefore the envelopes of the rows

  E_NUM(P) = 2.6e-7 + 0.8e-7 log2 P      (the line through the P = 9 and P = 150 columns; every other column lies below it)
  E_DEN    = 3.1e-7
  E_FIN(P) = 1.6e-7 log2 P               (the line through the origin and the P = 228 column)

A run of four particles at 1024 1x, which no test repeats, gave e_num 1.21e-6 (E_NUM(1024) = 1.06e-6, inside the 25 % below) and
e_den 3.24e-7.  The tests here hold the host path to the x1 figures plus 25 %, so the figures are re-measured on every run; the
GPU tests allow four times them (the device differs from this path in sinf / sincospi and FMA contraction only, and an indexing
error is orders of magnitude larger)."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build, wiener

from test_wiener_cpu import table

CSRC = os.path.join(build.HERE, "csrc")

# the x1 host ratios (module docstring) and what the host and the device are allowed on top
E_DEN = 3.1e-7
HOST_MARGIN, GPU_FACTOR = 1.25, 4.0


def e_num(P):
    return 2.6e-7 + 0.8e-7 * np.log2(P)


def e_fin(P):
    return 1.6e-7 * np.log2(P)


BOXES = [(8, True), (9, False), (13, True), (45, True), (64, False), (75, True)]
# the smallest box whose plan keeps its block in global scratch: pf_make_plan (ralign_ctf.h) sets gblk when
# P + 2 P PF_LDS_MIN_NB + nx H > (160 KiB - 1 KiB) / 8 = 20352 float2; at 2x (P = 2 nx, H = nx + 1) that is nx^2 + 67 nx > 20352,
# first true at nx = 114 (113: 20340); unpadded (P = nx, H = nx / 2 + 1) only from nx = 172.  test_plan_constants asks pf_make_plan
GBLK_BOX = (114, True)
K_PLANNED = 6


def run_plan(n, ph):
    """(T, L) of one chunk of n particles: the runs a class may be cut into and the members per run.  A copy of the host formulas
    of ra_wiener_accumulate (ralign_ctf.hip) with WN_THREADS = 256 elements per block, WN_BLOCKS_TARGET = 2048 workgroups and
    WN_MAX_RUNS = 64: if those change, the class sizes of `planned_case` no longer sit on the single-run boundary and this copy
    must follow"""
    eblk = -(-ph // 256)
    T = max(1, min(64, 2048 // eblk))
    return T, -(-n // T)


def chunk_size(n, ph, npix):
    """particles per chunk: wn_chunk's formula with WN_SCRATCH_BYTES = 1 GiB"""
    return max(1, min(n, (1 << 30) // (8 * ph + 4 * npix)))


def box(nx, pad):
    P = 2 * nx if pad else nx
    return P, P // 2 + 1, (P - nx) // 2


def stack(n, nx, seed):
    """images, params (alpha over 0 .. 360, non-zero shifts, mirror 0 and 1 mixed) and a table with 5000 - 8000 A of astigmatism
    at angles uniform over -180 .. 180"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nx, nx), dtype=np.float32)
    sh = rng.uniform(0.25, 3, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    prm = np.column_stack([rng.uniform(0, 360, n), sh, np.arange(n) % 2 if n > 1 else [1]])
    prm[:, 3] = rng.permutation(prm[:, 3])
    # alpha, sx, sy and the table as the device holds them (ra_result and the table are float32): a float64 alpha differs from its
    # float32 by up to 2e-5 degrees, which alone moves the CTF at Nyquist by 1e-5, fifty times the arithmetic's error
    return x, prm.astype(np.float32).astype(np.float64), table(n, nx, seed + 1).astype(np.float32)


def planned_labels(n, L, seed):
    """k = 6 classes laid on the run plan: 0 the bulk (many runs: the combine), 1 exactly L members (the single-run boundary), 2
    L + 1 (two runs, the second of one member), 3 one member, 4 none, 5 its 2 L members spread evenly through the stack (the
    stable sort gathers them)"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(n, np.int64)
    five = np.round(np.linspace(1, n - 2, 2 * L)).astype(int)
    assert len(set(five.tolist())) == 2 * L
    lab[five] = 5
    rest = rng.permutation(np.setdiff1d(np.arange(n), five))
    lab[rest[:L]] = 1
    lab[rest[L:2 * L + 1]] = 2
    lab[rest[2 * L + 1]] = 3
    return lab


def planned_case(nx, pad, n=200):
    P, H, _ = box(nx, pad)
    T, L = run_plan(n, P * H)
    assert L >= 2, "the plan formulas moved: n = %d no longer gives runs of at least two members" % n
    x, prm, tab = stack(n, nx, 100 * nx + pad)
    lab = planned_labels(n, L, nx)
    assert np.bincount(lab, minlength=K_PLANNED).tolist() == [n - 4 * L - 2, L, L + 1, 1, 0, 2 * L] and n - 4 * L - 2 > 2 * L
    return x, prm, lab, tab, L


def as_complex(num):
    num = np.asarray(num)
    return num if np.iscomplexobj(num) else num[..., 0].astype(np.float64) + 1j * num[..., 1].astype(np.float64)


def sum_ratios(num, den, counts, ref):
    """per class (e_num, e_den) of sums in the device's layout (num as float pairs or complex) against ref = (num, den, counts) of
    class_sums_reference; asserts equal counts and, for a class without members, sums that are exactly zero"""
    num, den, counts = as_complex(num), np.asarray(den, np.float64), np.asarray(counts)
    rnum, rden, rcounts = ref
    assert num.shape == rnum.shape and den.shape == rden.shape
    assert counts.tolist() == rcounts.tolist()
    e = np.zeros((len(counts), 2))
    for j, c in enumerate(rcounts):
        if c == 0:
            assert not num[j].any() and not den[j].any(), "class %d has no members and sums that are not zero" % j
            continue
        s = np.sqrt((np.abs(rnum[j]) ** 2).mean())
        e[j] = np.abs(num[j] - rnum[j]).max() / s, np.abs(den[j] - rden[j]).max() / max(1, c)
    return e


def check_sums(what, num, den, counts, ref, factor):
    """every element of every class within factor x (e_num(P) s_j, E_DEN max(1, count_j)); prints the observed ratios"""
    e = sum_ratios(num, den, counts, ref)
    bn, bd = factor * e_num(ref[0].shape[1]), factor * E_DEN
    print("%s: e_num %.3g (bound %.3g)  e_den %.3g (bound %.3g)" % (what, e[:, 0].max(), bn, e[:, 1].max(), bd))
    assert (e[:, 0] <= bn).all(), (what, "num", e[:, 0].tolist())
    assert (e[:, 1] <= bd).all(), (what, "den", e[:, 1].tolist())
    return e


def synthetic_sums(nx, pad, seed, min_count=3):
    """accumulators for the finalize alone, k = 4: num random complex float32 whose columns 0 and P/2 are not Hermitian (non-zero
    imaginary parts, at (0, 0) and (P/2, P/2) too), den random positive with a few exact zeros (the result there rests on 1/snr),
    counts on both sides of min_count"""
    P, H, _ = box(nx, pad)
    rng = np.random.default_rng(7 * nx + pad + seed)
    k = 4
    num = (rng.standard_normal((k, P, H, 2)) * rng.uniform(0.5, 20, (k, 1, 1, 1))).astype(np.float32)
    den = rng.uniform(0.05, 30, (k, P, H)).astype(np.float32)
    for j in range(k):
        den[j].flat[rng.choice(P * H, 5, replace=False)] = 0.0
        den[j, 0, 0] = 0.0
    assert (num[:, 0, 0, 1] != 0).all() and (num[:, P // 2, P // 2, 1] != 0).all()
    counts = np.array([min_count - 1, min_count, min_count + 5, 0], np.int32)
    return num, den, counts, min_count


def finalize_reference(num, den, counts, nx, pad, snr, min_count):
    P, _, o = box(nx, pad)
    out = np.zeros((len(counts), nx, nx))
    for j in range(len(counts)):
        if counts[j] >= min_count:
            out[j] = np.fft.irfft2(as_complex(num[j]) / (den[j].astype(np.float64) + 1.0 / snr), s=(P, P))[o:o + nx, o:o + nx]
    return out


def check_finalize(what, img, ref, counts, min_count, P, factor):
    """live classes within factor x e_fin(P) of their rms, the others exactly zero; prints the observed ratio"""
    worst, bound = 0.0, factor * e_fin(P)
    for j in range(len(counts)):
        if counts[j] < min_count:
            assert not img[j].any(), (what, j)
            continue
        e = np.abs(img[j] - ref[j]).max() / np.sqrt((ref[j] ** 2).mean())
        worst = max(worst, e)
        assert e <= bound, (what, j, e, bound)
    print("%s: e_fin %.3g (bound %.3g)" % (what, worst, bound))
    return worst


HARNESS = r"""
#include "ralign_wiener.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace ralign;
static bool rd(void *p, size_t sz, size_t cnt) { return fread(p, sz, cnt, stdin) == cnt; }
// plan nx pad                   -> stdout "P nb gblk lds"
// sums nx pad n k flipped L     stdin: n*nx*nx aligned images, n*9 table, n*2 (alpha, mirror) floats, n int labels
//                               -> num [k][P][H] float2, den [k][P][H]: runs of L members, as ra_wiener_accumulate cuts one chunk
// fin  nx pad k snr             stdin: num [k][P][H] float2, den [k][P][H] -> wn_class of every class, [k][nx][nx]
int main(int argc, char **argv)
{
    if (argc < 4) return 1;
    const int nx = atoi(argv[2]), pad = atoi(argv[3]);
    const PfPlan pl = pf_make_plan(nx, pad);
    if (!strcmp(argv[1], "plan")) { printf("%d %d %d %d\n", pl.P, pl.nb, pl.gblk, pl.lds); return 0; }
    if (pl.nb < 1) return 2;
    const int P = pl.P, H = pl.H, nb = pl.nb;
    const size_t ph = (size_t)P * H;
    std::vector<float2> tw(P), work((size_t)2 * nb * P), blk((size_t)nx * H);
    for (int t = 0; t < P; t++) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / P), (float)sin(-2.0 * M_PI * t / P));
    const PfCtx cx{0, 1};
    if (!strcmp(argv[1], "sums")) {
        const int n = atoi(argv[4]), k = atoi(argv[5]), flipped = atoi(argv[6]), L = atoi(argv[7]);
        std::vector<float> img((size_t)n * nx * nx), tab((size_t)n * 9), am((size_t)n * 2);
        std::vector<int> lab(n);
        if (!rd(img.data(), 4, img.size()) || !rd(tab.data(), 4, tab.size()) || !rd(am.data(), 4, am.size()) || !rd(lab.data(), 4, n)) return 3;
        std::vector<float2> spec((size_t)n * ph), num((size_t)k * ph, make_float2(0.f, 0.f));
        std::vector<float> den((size_t)k * ph, 0.f);
        std::vector<WnCtf> cst(n);
        for (int p = 0; p < n; p++) {
            wn_forward(cx, &img[(size_t)p * nx * nx], &spec[(size_t)p * ph], pl, blk.data(), work.data(), tw.data());
            cst[p] = wn_constants(&tab[(size_t)p * 9], nx, P, am[2 * p], am[2 * p + 1] != 0.f);
        }
        for (int j = 0; j < k; j++) {
            std::vector<int> mem;
            for (int p = 0; p < n; p++) if (lab[p] == j) mem.push_back(p);
            const int s = (int)mem.size();
            if (!s) continue;
            const int step = s <= L ? s : L;
            for (size_t e = 0; e < ph; e++) {                   // e = kx * P + n_, the spectrum's own order
                const int kx = (int)(e / P), n_ = (int)(e - (size_t)kx * P), iy = n_ < (P + 1) / 2 ? n_ : n_ - P;
                double cx_ = 0.0, cy_ = 0.0, cd_ = 0.0;         // the combine's sums of the runs' floats
                float fx = 0.f, fy = 0.f, fd = 0.f;
                for (int b = 0; b < s; b += step) {
                    double ax = 0.0, ay = 0.0, d = 0.0;
                    for (int m = b; m < std::min(s, b + step); m++) {
                        const int p = mem[m];
                        const float c = wn_ctf(cst[p], iy, kx), w = flipped ? fabsf(c) : c;
                        const float2 y = spec[(size_t)p * ph + e];
                        ax += (double)(w * y.x); ay += (double)(w * y.y); d += (double)(c * c);
                    }
                    fx = (float)ax; fy = (float)ay; fd = (float)d;
                    cx_ += fx; cy_ += fy; cd_ += fd;
                }
                if (s > L) { fx = (float)cx_; fy = (float)cy_; fd = (float)cd_; }
                const size_t o = (size_t)j * ph + (size_t)n_ * H + kx;
                num[o] = make_float2(num[o].x + fx, num[o].y + fy);
                den[o] += fd;
            }
        }
        fwrite(num.data(), 8, num.size(), stdout);
        fwrite(den.data(), 4, den.size(), stdout);
        return 0;
    }
    if (!strcmp(argv[1], "fin")) {
        const int k = atoi(argv[4]);
        const float snr = (float)atof(argv[5]);
        std::vector<float2> num((size_t)k * ph);
        std::vector<float> den((size_t)k * ph), out((size_t)k * nx * nx);
        if (!rd(num.data(), 8, num.size()) || !rd(den.data(), 4, den.size())) return 3;
        for (int j = 0; j < k; j++)
            wn_class(cx, &num[(size_t)j * ph], &den[(size_t)j * ph], 1.0f / snr, &out[(size_t)j * nx * nx], pl, blk.data(), work.data(), tw.data());
        fwrite(out.data(), 4, out.size(), stdout);
        return 0;
    }
    return 1;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wnsums")
    src, exe = str(d / "wnsums.cpp"), str(d / "wnsums")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(build.ROOT, "include"), "-o", exe, src])
    return exe


def host_sums(exe, y, prm, lab, k, tab, pad, flipped, L):
    """the float32 (num [k][P][H][2], den [k][P][H]) the host path forms from aligned images y"""
    n, nx = y.shape[0], y.shape[-1]
    P, H, _ = box(nx, pad)
    am = np.column_stack([prm[:, 0], prm[:, 3]]).astype(np.float32)
    r = subprocess.run([exe, "sums", str(nx), str(int(pad)), str(n), str(k), str(int(flipped)), str(L)],
                       input=np.ascontiguousarray(y, np.float32).tobytes() + np.ascontiguousarray(tab, np.float32).tobytes() + am.tobytes() +
                       np.asarray(lab).astype(np.int32).tobytes(), capture_output=True, check=True)
    a = np.frombuffer(r.stdout, np.float32)
    return a[:k * P * H * 2].reshape(k, P, H, 2), a[k * P * H * 2:].reshape(k, P, H)


def host_finalize(exe, num, den, nx, pad, snr):
    k = num.shape[0]
    r = subprocess.run([exe, "fin", str(nx), str(int(pad)), str(k), repr(float(snr))], input=num.tobytes() + den.tobytes(),
                       capture_output=True, check=True)
    return np.frombuffer(r.stdout, np.float32).reshape(k, nx, nx)


def test_plan_constants(harness):
    """the plan and chunk figures the GPU tests name: 114 at 2x is the first box whose block lives in global scratch"""
    plan = lambda nx, pad: [int(v) for v in subprocess.run([harness, "plan", str(nx), str(int(pad))], capture_output=True, check=True).stdout.split()]
    for nx in range(2, GBLK_BOX[0]):
        for pad in (0, 1):
            assert plan(nx, pad)[2] == 0, (nx, pad)
    assert plan(GBLK_BOX[0], 0)[2] == 0 and plan(*GBLK_BOX)[2] == 1
    assert plan(1024, 0)[1:3] == [8, 1]
    # the 1024 box of the chunk test: 127 particles per chunk, and one run per chunk (more element blocks than the reduce's target)
    assert chunk_size(10 ** 6, 1024 * 513, 1024 * 1024) == 127 and run_plan(127, 1024 * 513) == (1, 127)
    assert [run_plan(200, box(nx, pad)[0] * box(nx, pad)[1])[1] for nx, pad in BOXES] == [4, 4, 4, 4, 4, 5]


@pytest.mark.parametrize("nx,pad", BOXES)
def test_host_sums_within_the_measured_ratios(harness, nx, pad):
    """the host path at the GPU test's boxes and labels, its own white-noise images taken as the aligned ones (the ratios are
    relative to each class's sums): within the x1 figures plus 25 %"""
    x, prm, lab, tab, L = planned_case(nx, pad)
    for flipped in (False, True):
        ref = wiener.class_sums_reference(x, prm, lab, K_PLANNED, tab, pad, flipped, aligned=x)
        num, den = host_sums(harness, x, prm, lab, K_PLANNED, tab, pad, flipped, L)
        check_sums("host %d pad %d flipped %d" % (nx, pad, flipped), num, den, ref[2], ref, HOST_MARGIN)


@pytest.mark.parametrize("nx,pad", BOXES + [GBLK_BOX])
def test_host_finalize_within_the_measured_ratio(harness, nx, pad):
    num, den, counts, min_count = synthetic_sums(nx, pad, 0)
    snr = 0.8
    got = host_finalize(harness, num, den, nx, pad, snr).astype(np.float64)
    got[counts < min_count] = 0.0           # wn_class is the live classes' path; the kernel zeroes the others
    check_finalize("host %d pad %d" % (nx, pad), got, finalize_reference(num, den, counts, nx, pad, snr, min_count), counts, min_count,
                   box(nx, pad)[0], HOST_MARGIN)


def reference_with_row_at_opposite_frequency(x, prm, lab, k, tab, pad, aligned, row):
    """class_sums_reference (w = c) whose row `row` has the CTF of row frequency -row: what the wrong sign of iy does to that row"""
    from cryo_ralib_amd import ctf
    nx = x.shape[-1]
    P, _, o = box(nx, pad)
    num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, pad, False, aligned=aligned)
    t = wiener.aligned_table(np.asarray(tab, np.float64), prm)
    num[:, row], den[:, row] = 0, 0
    for i in range(len(x)):
        big = np.zeros((P, P))
        big[o:o + nx, o:o + nx] = aligned[i]
        c = ctf.ctf_grid(t[i], nx, P)[P - row]
        num[lab[i], row] += c * np.fft.rfft2(big)[row]
        den[lab[i], row] += c * c
    return num, den, counts


def test_comparison_sees_an_indexing_error(harness):
    """the reference perturbed, never the code: the CTF of one row taken at the opposite row frequency, and one member left out of
    the bulk class, both land orders of magnitude outside the GPU bound (e_num 2.6 .. 5.5 and 0.32, e_den 5.5e-3)"""
    nx, pad = 45, True
    x, prm, lab, tab, L = planned_case(nx, pad)
    num, den = host_sums(harness, x, prm, lab, K_PLANNED, tab, pad, False, L)
    P = box(nx, pad)[0]
    ref = wiener.class_sums_reference(x, prm, lab, K_PLANNED, tab, pad, False, aligned=x)
    e = sum_ratios(num, den, ref[2], reference_with_row_at_opposite_frequency(x, prm, lab, K_PLANNED, tab, pad, x, 7))
    print("row 7 at the opposite frequency: e_num %s" % e[:, 0])
    live = ref[2] > 0
    assert (e[live, 0] > 1000 * GPU_FACTOR * e_num(P)).all()
    keep = np.ones(len(x), bool)
    keep[np.nonzero(lab == 0)[0][-1]] = False
    drop = wiener.class_sums_reference(x[keep], prm[keep], lab[keep], K_PLANNED, tab[keep], pad, False, aligned=x[keep])
    e = sum_ratios(num, den, drop[2], drop)          # the counts would tell first: taken as agreed to see the sums' ratios
    print("one of %d members dropped: e_num %.3g e_den %.3g" % (ref[2][0], e[0, 0], e[0, 1]))
    assert e[0, 0] > 1000 * GPU_FACTOR * e_num(P) and e[0, 1] > 100 * GPU_FACTOR * E_DEN
