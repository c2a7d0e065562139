"""Half-set FRC and SSNR-weighted Wiener class averages without a GPU: the float64 contract (wiener.ssnr_reference,
frc_from_sums, resolution) on cases whose answer is known, the tool's refusals before any device work, and the FRC and finalize
passes of csrc/ralign_wiener.h compiled for the host and run as one sequential thread against the contract."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build, wiener

from test_wiener_cpu import masked_corr, physical_case, table

CSRC = os.path.join(build.HERE, "csrc")


def _full_plane_shells(P):
    k = np.fft.fftfreq(P) * P
    return np.floor(np.sqrt(k[None, :] ** 2 + k[:, None] ** 2) + 0.5).astype(np.int64)


@pytest.mark.parametrize("P", [63, 64])
def test_hermitian_weights_give_the_full_plane_shell_sums(P):
    rng = np.random.default_rng(P)
    a, b = rng.standard_normal((2, P, P))
    s, g = wiener.shells(P)
    sf = _full_plane_shells(P)
    ra, rb, fa, fb = np.fft.rfft2(a), np.fft.rfft2(b), np.fft.fft2(a), np.fft.fft2(b)
    for shell in range(P // 2 + 1):
        h, f = s == shell, sf == shell
        for half, full in (((g * np.abs(ra) ** 2)[h].sum(), (np.abs(fa) ** 2)[f].sum()),
                           ((g * (ra * np.conj(rb)).real)[h].sum(), (fa * np.conj(fb)).real[f].sum()),
                           (g[h].sum(), f.sum())):
            assert abs(half - full) <= 1e-9 * max(1.0, abs(full)), (shell, half, full)
    assert s.max() > P // 2          # the corners lie beyond the last shell


def _noise_case(n, nx, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nx, nx))
    prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.integers(0, 2, n)])
    return x, prm, rng.integers(0, k, n), table(n, nx, seed + 1)


def test_identical_halves_correlate_fully():
    m, nx, k = 12, 20, 2
    x, prm, lab, tab = _noise_case(m, nx, k, 3)
    rep = np.repeat(np.arange(m), 2)           # particle m at indices 2m and 2m + 1: one copy in each half
    out, counts, frc, reg = wiener.ssnr_reference(x[rep], prm[rep], lab[rep], k, tab[rep], snr=1.0, ssnr_floor=1e-3)
    num, den, cnt = wiener.class_sums_reference(x[rep], prm[rep], wiener.half_labels(lab[rep]), 2 * k, tab[rep])
    P = 2 * nx
    s, g = wiener.shells(P)
    for j in range(k):
        assert cnt[2 * j] == cnt[2 * j + 1] == counts[j] // 2
        power = np.bincount(s[s <= P // 2], (g * np.abs(num[2 * j]) ** 2)[s <= P // 2], P // 2 + 1) > 0
        assert power.all()
        assert np.abs(frc[j] - 1).max() <= 1e-12
        dbar = np.bincount(s[s <= P // 2], (g * (den[2 * j] + den[2 * j + 1]))[s <= P // 2], P // 2 + 1) / \
            np.bincount(s[s <= P // 2], g[s <= P // 2], P // 2 + 1)
        assert np.allclose(dbar / reg[j], 1998.0, rtol=1e-9)
    assert np.isfinite(out).all() and np.abs(out).max() > 0


@pytest.mark.parametrize("pad", [False, True])
def test_pure_noise_halves_do_not_correlate(pad):
    n, nx, k = 80, 24, 1
    x, prm, lab, tab = _noise_case(n, nx, k, 11 + pad)
    _, _, frc, reg = wiener.ssnr_reference(x, prm, lab, k, tab, snr=1.0, ssnr_floor=1e-3, pad=pad)
    num, den, _ = wiener.class_sums_reference(x, prm, wiener.half_labels(lab), 2, tab, pad)
    P = 2 * nx if pad else nx
    s, g = wiener.shells(P)
    inside = s <= P // 2
    gsum = np.bincount(s[inside], g[inside], P // 2 + 1)
    f = frc[0, 2:]
    # with 2x padding neighbouring elements are correlated: about 4x fewer independent samples per shell
    bound = 6 / np.sqrt(gsum[2:] / (4 if pad else 1))
    assert (np.abs(f) < bound).all(), np.abs(f) / bound
    assert abs(f.mean()) < 0.05
    dbar = np.bincount(s[inside], (g * (den[0] + den[1]))[inside], P // 2 + 1) / gsum
    low = frc[0] <= 0
    assert low.any()
    assert np.allclose(reg[0][low], dbar[low] / 1e-3, rtol=1e-12)


def test_half_sums_add_to_the_constant_path_sums():
    n, nx, k = 15, 16, 3
    x, prm, lab, tab = _noise_case(n, nx, k, 5)
    for index0 in (0, 7):
        for flipped in (False, True):
            num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, flipped=flipped)
            num2, den2, cnt2 = wiener.class_sums_reference(x, prm, wiener.half_labels(lab, index0), 2 * k, tab, flipped=flipped)
            assert np.abs(num2[0::2] + num2[1::2] - num).max() <= 1e-12 * np.abs(num).max()
            assert np.abs(den2[0::2] + den2[1::2] - den).max() <= 1e-12 * np.abs(den).max()
            assert (cnt2[0::2] + cnt2[1::2] == counts).all()
            assert cnt2[0::2].tolist() == [int(((index0 + np.arange(n)) % 2 == 0)[lab == j].sum()) for j in range(k)]


def test_ssnr_average_recovers_the_truth_better_than_a_constant_snr():
    fl, prm, tab, truth, mask = physical_case(120, seed=6, sigma=2.0)
    lab = np.zeros(len(fl), np.int64)
    const, _ = wiener.wiener_reference(fl, prm, lab, 1, tab, snr=1.0, flipped=True)
    ssnr, counts, frc, _ = wiener.ssnr_reference(fl, prm, lab, 1, tab, snr=1.0, flipped=True)
    c_c, c_s = masked_corr(const[0], truth, mask), masked_corr(ssnr[0], truth, mask)
    print("1 - corr with truth: constant snr 1 %.3g, SSNR-weighted %.3g" % (1 - c_c, 1 - c_s))
    assert counts.tolist() == [120]
    assert c_s > c_c
    assert frc[0, 1] > 0.9 and frc[0, -8:].mean() < 0.2      # the band-limited truth: signal at low, noise at high frequency


def test_resolution_of_hand_built_curves():
    nx = 32                                     # P = 64, shells 0 .. 32
    S = 33
    f = np.ones((4, S))
    f[0, 1] = 0.1                               # crossing at shell 1: s* = 0
    f[2, 10:] = 0.3                             # 0.5 crossed at 10, 0.143 never
    f[3, 5:] = 0.0
    f[3, 7] = 0.9                               # the first crossing counts, not a later recovery
    r05 = wiener.resolution(f, nx, True, threshold=0.5)
    r0143 = wiener.resolution(f, nx, True, threshold=0.143)
    assert r05[0] == np.inf and r0143[0] == np.inf
    assert r05[1] == r0143[1] == 64 / 32         # no crossing: Nyquist of the nx sampling, 2 pixels
    assert r05[2] == 64 / 9 and r0143[2] == 2.0
    assert r05[3] == r0143[3] == 64 / 4
    assert wiener.resolution(f, nx, True, apix=1.5, threshold=0.5)[2] == 64 * 1.5 / 9
    assert wiener.resolution(f[2], nx, True, apix=1.5, threshold=0.5) == 64 * 1.5 / 9
    nan = wiener.resolution(f, nx, True, threshold=0.5, counts=[5, 5, 1, 5], min_count=2)
    assert np.isnan(nan[2]) and nan[3] == 16.0
    assert wiener.resolution(np.ones(nx // 2 + 1), nx, False, apix=2.0) == 4.0
    with pytest.raises(wiener.WienerError):
        wiener.resolution(f, nx, False)
    res = wiener.resolutions(f, [5] * 4, nx, True, None)
    assert res["units"] == "px" and wiener.resolutions(f, [5] * 4, nx, True, 1.5)["units"] == "A"


def test_table_pixel_size():
    t = table(6, 40, 2)
    assert wiener.table_apix(t, 40) is None
    t[:, 1] = 1.25
    t[:, 0] = 80
    assert wiener.table_apix(t, 40) == 2.5
    t[3, 1] *= 1 + 5e-5
    assert wiener.table_apix(t, 40) == 2.5
    t[3, 1] *= 1 + 5e-4
    assert wiener.table_apix(t, 40) is None


def test_ssnr_argument_errors():
    n, nx = 4, 16
    x, prm, lab, tab = np.zeros((n, nx, nx)), np.zeros((n, 4)), np.zeros(n, np.int64), table(n, nx, 1)
    for kw in ({"k": 513}, {"ssnr_floor": 0.0}, {"ssnr_floor": -1.0}, {"ssnr_floor": np.nan}, {"ssnr_floor": np.inf}, {"snr": 0.0}):
        args = dict(k=1, ssnr_floor=1e-3, snr=1.0)
        args.update(kw)
        with pytest.raises(wiener.WienerError):
            wiener.ssnr_reference(x, prm, lab, args["k"], tab, snr=args["snr"], ssnr_floor=args["ssnr_floor"])


def test_tool_refuses_bad_ssnr_options_before_the_device(tmp_path):
    n, nx = 5, 16
    stack, prm, tab = tmp_path / "s.npy", tmp_path / "p.txt", tmp_path / "t.npy"
    np.save(stack, np.zeros((n, nx, nx), np.float32))
    np.savetxt(prm, np.column_stack([np.arange(n), np.zeros((n, 4)), np.arange(n) % 2]))
    np.save(tab, table(n, nx, 2))
    base = [str(stack), str(prm), str(tab), str(tmp_path / "o.npy")]
    with pytest.raises(SystemExit, match="k <= 512"):
        wiener.main(base + ["--ssnr", "--k", "513"])
    for floor in ("0", "-1", "nan"):
        with pytest.raises(SystemExit, match="ssnr_floor"):
            wiener.main(base + ["--ssnr", "--ssnr_floor", floor])
    with pytest.raises(SystemExit, match="--frc needs --ssnr"):
        wiener.main(base + ["--frc", str(tmp_path / "f.npz")])
    assert not os.path.exists(str(tmp_path / "o.npy"))


HARNESS = r"""
#include "ralign_wiener.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace ralign;
// argv: nx pad nb k rows snr floor min_count; stdin: num2 [k][2][P][H] float2, den2 [k][2][P][H], counts2 [k][2] int;
// stdout: frc [k][S] double, reg [k][S] float, the averages [k][nx][nx] float
int main(int argc, char **argv)
{
    const int nx = atoi(argv[1]), pad = atoi(argv[2]), nb = atoi(argv[3]), k = atoi(argv[4]), rows = atoi(argv[5]);
    const float snr = (float)atof(argv[6]), floor_ = (float)atof(argv[7]);
    const int min_count = atoi(argv[8]);
    PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nrad == 0 && pl.P > 1) return 2;
    pl.nb = nb;
    const int P = pl.P, H = pl.H, S = P / 2 + 1;
    const size_t ph = (size_t)P * H;
    std::vector<float2> num2((size_t)k * 2 * ph);
    std::vector<float> den2((size_t)k * 2 * ph);
    std::vector<int> counts2((size_t)k * 2);
    if (fread(num2.data(), 8, num2.size(), stdin) != num2.size() || fread(den2.data(), 4, den2.size(), stdin) != den2.size() ||
        fread(counts2.data(), 4, counts2.size(), stdin) != counts2.size()) return 3;
    const int blocks = (P + rows - 1) / rows;
    std::vector<double> part((size_t)k * blocks * 5 * S), frc((size_t)k * S);
    std::vector<float> reg((size_t)k * S);
    for (int j = 0; j < k; j++)
        for (int b = 0; b < blocks; b++)
            for (int s = 0; s < S; s++) {
                double a[5];
                const float2 *n0 = &num2[(size_t)2 * j * ph];
                const float *d0 = &den2[(size_t)2 * j * ph];
                wn_frc_shell_rows(n0, n0 + ph, d0, d0 + ph, P, b * rows, std::min(P, (b + 1) * rows), s, 1.0 / (double)snr, a);
                for (int q = 0; q < 5; q++) part[(((size_t)j * blocks + b) * 5 + q) * S + s] = a[q];
            }
    for (int j = 0; j < k; j++)
        for (int s = 0; s < S; s++) {
            double a[5] = {0, 0, 0, 0, 0};
            for (int b = 0; b < blocks; b++)
                for (int q = 0; q < 5; q++) a[q] += part[(((size_t)j * blocks + b) * 5 + q) * S + s];
            wn_frc_shell(a, counts2[2 * j] + counts2[2 * j + 1] >= min_count, floor_, &frc[(size_t)j * S + s], &reg[(size_t)j * S + s]);
        }
    std::vector<float2> tw(P), work((size_t)2 * nb * P), blk((size_t)nx * H);
    for (int t = 0; t < P; t++) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / P), (float)sin(-2.0 * M_PI * t / P));
    std::vector<float> out((size_t)k * nx * nx, 0.f);
    const PfCtx cx{0, 1};
    for (int j = 0; j < k; j++) {
        if (counts2[2 * j] + counts2[2 * j + 1] < min_count) continue;
        const size_t a = (size_t)2 * j * ph;
        const WnSsnrSrc src{&num2[a], &num2[a + ph], &den2[a], &den2[a + ph], &reg[(size_t)j * S], P};
        wn_class_src(cx, src, &out[(size_t)j * nx * nx], pl, blk.data(), work.data(), tw.data());
    }
    fwrite(frc.data(), 8, frc.size(), stdout);
    fwrite(reg.data(), 4, reg.size(), stdout);
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wnssnr")
    src, exe = str(d / "wnssnr.cpp"), str(d / "wnssnr")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(build.ROOT, "include"), "-o", exe, src])
    return exe


@pytest.mark.parametrize("nx,pad,nb,rows,n", [(8, 1, 3, 5, 16), (9, 0, 2, 1, 12), (13, 1, 4, 26, 14), (15, 1, 32, 7, 10), (20, 0, 5, 3, 30)])
def test_host_passes_match_the_contract(harness, nx, pad, nb, rows, n):
    k = 3
    rng = np.random.default_rng(nx * 5 + pad)
    y = rng.standard_normal((n, nx, nx))
    y[1::2] = y[0::2] + 0.7 * rng.standard_normal(y[1::2].shape)   # halves that share part of their signal
    prm = np.column_stack([rng.uniform(-180, 360, n), np.zeros(n), np.zeros(n), rng.integers(0, 2, n)])
    lab = rng.integers(0, k - 1, n)
    lab[:2] = k - 1                                    # the last class: two members, below min_count = 3
    tab = table(n, nx, nx)
    num, den, cnt = wiener.class_sums_reference(y, prm, wiener.half_labels(lab), 2 * k, tab, bool(pad), True, aligned=y)
    P, S = (2 * nx if pad else nx), (2 * nx if pad else nx) // 2 + 1
    num2 = num.reshape(k, 2, P, S).astype(np.complex64)
    den2 = den.reshape(k, 2, P, S).astype(np.float32)
    cnt2 = cnt.reshape(k, 2).astype(np.int32)
    snr, floor = 1.5, np.float32(1e-3)
    r = subprocess.run([harness, str(nx), str(pad), str(nb), str(k), str(rows), repr(snr), repr(float(floor)), "3"],
                       input=num2.tobytes() + den2.tobytes() + cnt2.tobytes(), capture_output=True, check=True)
    buf = r.stdout
    got_f = np.frombuffer(buf[:k * S * 8], np.float64).reshape(k, S)
    got_r = np.frombuffer(buf[k * S * 8:k * S * 12], np.float32).reshape(k, S)
    got_a = np.frombuffer(buf[k * S * 12:], np.float32).reshape(k, nx, nx)
    want_f, want_r = wiener.frc_from_sums(num2, den2, cnt2, nx, bool(pad), snr, 3, float(floor))
    assert np.abs(got_f - want_f).max() <= 1e-12
    assert np.all(np.abs(got_r - want_r) <= 1e-6 * np.abs(want_r))
    assert not got_f[k - 1].any() and not got_a[k - 1].any()
    assert np.abs(got_f[:k - 1]).max() > 0.1
    # step 5 on the same (float32) sums and regulariser
    s, _ = wiener.shells(P)
    s = np.minimum(s, P // 2)
    o = (P - nx) // 2
    for j in range(k - 1):
        d = den2[j, 0].astype(np.float64) + den2[j, 1] + got_r[j][s]
        want = np.fft.irfft2((num2[j, 0].astype(np.complex128) + num2[j, 1]) / d, s=(P, P))[o:o + nx, o:o + nx]
        assert np.abs(got_a[j] - want).max() <= 1e-5 * np.abs(want).max()
