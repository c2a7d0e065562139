"""CTF-corrected (Wiener) class averages without a GPU: the angle rule of the CTF in the aligned frame against explicitly rotated
and reflected frequencies, the convention on rotated CTF-modulated images, the limits of the float64 contract
(wiener.wiener_reference), its argument checks, and the device passes of csrc/ralign_wiener.h compiled for the host and run as
one sequential thread against the contract."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build, ctf, geometry, synth, wiener

CSRC = os.path.join(build.HERE, "csrc")


def table(n, nx, seed, astig=5000.0):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 9))
    t[:, 0] = nx
    t[:, 1] = rng.uniform(1.2, 2.5, n)
    t[:, 2] = rng.uniform(15000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(astig, astig + 3000, n)
    t[:, 4] = rng.uniform(-180, 180, n)
    t[:, 5] = rng.choice([200.0, 300.0], n)
    t[:, 6] = rng.uniform(0.01, 2.7, n)
    t[:, 7] = rng.uniform(0.0, 0.2, n)
    t[:, 8] = rng.choice([0.0, 25.0], n)
    return t


def _rotated_frequencies(P, alpha, mirror):
    """G k on the rfft2 grid: rot_shift2D reads its input at G r + b, G = R(alpha) M^mirror (M: x -> -x)"""
    ix = np.arange(P // 2 + 1)[None, :] * np.ones((P, 1))
    iy = (np.fft.fftfreq(P) * P)[:, None] * np.ones((1, P // 2 + 1))
    if mirror:
        ix = -ix
    a = np.radians(alpha)
    return np.cos(a) * ix - np.sin(a) * iy, np.sin(a) * ix + np.cos(a) * iy


@pytest.mark.parametrize("P", [64, 75])
@pytest.mark.parametrize("mirror", [0, 1])
def test_angle_rule_is_the_ctf_at_rotated_frequencies(P, mirror):
    rng = np.random.default_rng(P + 10 * mirror)
    nx = P // 2 if P % 2 == 0 else P
    tab = table(6, nx, P + mirror)
    for i in range(6):
        alpha = rng.uniform(-180, 360)
        kx, ky = _rotated_frequencies(P, alpha, mirror)
        want = wiener.ctf_at(tab[i], nx, P, kx, ky)
        row = wiener.aligned_table(tab[i:i + 1], [[alpha, 0, 0, mirror]])[0]
        assert np.abs(ctf.ctf_grid(row, nx, P) - want).max() < 1e-12
        # the other sign choices do not match
        for ang in (tab[i, 4] + alpha, -alpha - tab[i, 4]) if not mirror else (tab[i, 4] - alpha, alpha + tab[i, 4]):
            wrong = tab[i].copy()
            wrong[4] = ang
            assert np.abs(ctf.ctf_grid(wrong, nx, P) - want).max() > 0.1
    # ctf_at on the integer grid is ctf_grid
    kx, ky = _rotated_frequencies(P, 0.0, 0)
    assert np.abs(wiener.ctf_at(tab[0], nx, P, kx, ky) - ctf.ctf_grid(tab[0], nx, P)).max() < 1e-12


def _apply_ctf(img, row, nx):
    """the particle as the microscope records it, in EMAN2's orientation (-ctf_np), in a 2x padded image"""
    P, o = 2 * nx, nx // 2
    big = np.zeros((P, P))
    big[o:o + nx, o:o + nx] = img
    return np.fft.irfft2(np.fft.rfft2(big) * -ctf.ctf_grid(row, nx, P), s=(P, P))[o:o + nx, o:o + nx]


def physical_case(n, nx=64, ou=26, seed=5, sigma=0.5):
    """truth T; particle i = CTF_i(rot_shift2D(T, inverse of params_i)) + noise, so rot_shift2D(particle_i, params_i) ~ CTF_i T;
    returns the phase-flipped particles, params, table, truth and the mask"""
    truth = synth.make_references(1, nx, ou, seed=seed)[0].astype(np.float64)
    rng = np.random.default_rng(seed)
    tab = table(n, nx, seed + 1)
    prm = np.zeros((n, 4))
    parts = np.zeros((n, nx, nx))
    for i in range(n):
        a, sx, sy, m = rng.uniform(0, 360), rng.integers(-2, 3), rng.integers(-2, 3), int(rng.integers(0, 2))
        prm[i] = (a, sx, sy, m)
        ia, isx, isy, im = geometry.inverse_transform2(a, sx, sy, m)
        parts[i] = _apply_ctf(synth.rot_shift2d_np(truth, ia, isx, isy, im), tab[i], nx)
    parts += rng.normal(0, sigma * truth.std(), parts.shape)
    flipped = ctf.flip_reference(parts, tab)
    return flipped, prm, tab, truth, geometry.model_circle(ou, nx, nx) > 0.5


def masked_corr(a, b, mask):
    a = a[mask] - a[mask].mean()
    b = b[mask] - b[mask].mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_contract_recovers_the_truth_better_than_the_flipped_mean(monkeypatch):
    """on this seed 1 - corr: Wiener 6.3e-4, plain mean of the flipped particles 2.3e-2, the opposite angle rule 1.0e-3 (the truth
    is smooth, so the gains are small in correlation and large in the residual)"""
    fl, prm, tab, truth, mask = physical_case(150)
    lab = np.zeros(len(fl), np.int64)
    avg, counts = wiener.wiener_reference(fl, prm, lab, 1, tab, snr=2.0, flipped=True)
    plain = np.mean([synth.rot_shift2d_np(fl[i], *prm[i, :3], int(prm[i, 3])) for i in range(len(fl))], axis=0)
    orig = wiener.aligned_table

    def opposite(t, p):
        t2 = orig(t, p)
        t2[:, 4] = 2 * np.asarray(t, np.float64)[:, 4] - t2[:, 4]        # DefocusAngle + alpha, -alpha - DefocusAngle
        return t2
    monkeypatch.setattr(wiener, "aligned_table", opposite)
    wrong, _ = wiener.wiener_reference(fl, prm, lab, 1, tab, snr=2.0, flipped=True)
    c_w, c_p, c_x = masked_corr(avg[0], truth, mask), masked_corr(plain, truth, mask), masked_corr(wrong[0], truth, mask)
    print("1 - corr with truth: wiener %.3g, flipped mean %.3g, opposite angle rule %.3g" % (1 - c_w, 1 - c_p, 1 - c_x))
    assert counts.tolist() == [150]
    assert 1 - c_w < 0.1 * (1 - c_p)
    assert 1 - c_w < 0.8 * (1 - c_x)


def test_unit_ctf_and_large_snr_give_the_plain_mean(monkeypatch):
    rng = np.random.default_rng(3)
    n, nx, k = 9, 20, 3
    x = rng.standard_normal((n, nx, nx))
    prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.integers(0, 2, n)])
    lab = np.array([0, 0, 0, 0, 2, 2, 0, 2, 0])
    monkeypatch.setattr(ctf, "ctf_grid", lambda row, nx, P: np.ones((P, P // 2 + 1)))
    for pad in (True, False):
        avg, counts = wiener.wiener_reference(x, prm, lab, k, table(n, nx, 4), snr=1e12, pad=pad)
        al = np.array([synth.rot_shift2d_np(x[i], *prm[i, :3], int(prm[i, 3])) for i in range(n)], np.float64)
        assert counts.tolist() == [6, 0, 3]
        for j in range(k):
            want = al[lab == j].mean(0) if counts[j] else np.zeros((nx, nx))
            assert np.abs(avg[j] - want).max() < 1e-10
    avg, _ = wiener.wiener_reference(x, prm, lab, k, table(n, nx, 4), snr=1e12, min_count=4)
    assert not avg[2].any() and not avg[1].any() and avg[0].any()


def test_argument_errors():
    n, nx = 4, 16
    x = np.zeros((n, nx, nx))
    prm, lab, tab = np.zeros((n, 4)), np.zeros(n, np.int64), table(n, nx, 1)
    bad_row = tab.copy()
    bad_row[2, 1] = -1.0
    nan_prm = prm.copy()
    nan_prm[1, 0] = np.nan
    for args, kw in [((x[:, :, :8], prm, lab, 1, tab), {}), ((x, prm[:, :3], lab, 1, tab), {}), ((x, nan_prm, lab, 1, tab), {}),
                     ((x, prm, lab + 1, 1, tab), {}), ((x, prm, lab - 1, 1, tab), {}), ((x, prm, lab.astype(float), 1, tab), {}),
                     ((x, prm, lab, 0, tab), {}), ((x, prm, lab, 1, tab[:3]), {}), ((x, prm, lab, 1, bad_row), {}),
                     ((x, prm, lab, 1, tab), {"snr": 0.0}), ((x, prm, lab, 1, tab), {"snr": -1.0})]:
        with pytest.raises(wiener.WienerError):
            wiener.wiener_reference(*args, **kw)


def test_tool_refuses_bad_inputs_before_the_device(tmp_path):
    n, nx = 5, 16
    stack, prm, tab = tmp_path / "s.npy", tmp_path / "p.txt", tmp_path / "t.npy"
    np.save(stack, np.zeros((n, nx, nx), np.float32))
    np.savetxt(prm, np.column_stack([np.arange(n), np.zeros((n, 4)), np.arange(n) % 2]))
    t = table(n, nx, 2)
    t[3, 5] = 0.0
    np.save(tab, t)
    with pytest.raises(SystemExit, match="row 3"):
        wiener.main([str(stack), str(prm), str(tab), str(tmp_path / "o.npy")])
    np.save(tab, table(n, nx, 2))
    with pytest.raises(SystemExit, match="labels"):
        wiener.main([str(stack), str(prm), str(tab), str(tmp_path / "o.npy"), "--k", "1"])


HARNESS = r"""
#include "ralign_wiener.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace ralign;
// argv: nx pad nb n flipped snr; stdin: n*nx*nx aligned images, n*9 table, n*2 (alpha, mirror); stdout: the one-class average
int main(int argc, char **argv)
{
    const int nx = atoi(argv[1]), pad = atoi(argv[2]), nb = atoi(argv[3]), n = atoi(argv[4]), flipped = atoi(argv[5]);
    const float snr = (float)atof(argv[6]);
    PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nrad == 0 && pl.P > 1) return 2;
    pl.nb = nb;
    const int P = pl.P, H = pl.H;
    std::vector<float> img((size_t)n * nx * nx), tab((size_t)n * 9), am((size_t)n * 2);
    if (fread(img.data(), 4, img.size(), stdin) != img.size() || fread(tab.data(), 4, tab.size(), stdin) != tab.size() ||
        fread(am.data(), 4, am.size(), stdin) != am.size()) return 3;
    std::vector<float2> tw(P), work((size_t)2 * nb * P), blk((size_t)nx * H), spec((size_t)H * P), num((size_t)P * H);
    std::vector<double> nx_(num.size()), ny_(num.size()), dd(num.size());
    std::vector<float> den((size_t)P * H);
    for (int t = 0; t < P; t++) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / P), (float)sin(-2.0 * M_PI * t / P));
    const PfCtx cx{0, 1};
    for (int p = 0; p < n; p++) {
        wn_forward(cx, &img[(size_t)p * nx * nx], spec.data(), pl, blk.data(), work.data(), tw.data());
        const WnCtf c = wn_constants(&tab[(size_t)p * 9], nx, P, am[2 * p], am[2 * p + 1] != 0.f);
        for (int kx = 0; kx < H; kx++)
            for (int n_ = 0; n_ < P; n_++) {
                const float cc = wn_ctf(c, n_ < (P + 1) / 2 ? n_ : n_ - P, kx), w = flipped ? fabsf(cc) : cc;
                const float2 y = spec[(size_t)kx * P + n_];
                const size_t o = (size_t)n_ * H + kx;
                nx_[o] += w * y.x; ny_[o] += w * y.y; dd[o] += cc * cc;
            }
    }
    for (size_t e = 0; e < num.size(); e++) { num[e] = make_float2((float)nx_[e], (float)ny_[e]); den[e] = (float)dd[e]; }
    std::vector<float> out((size_t)nx * nx);
    wn_class(cx, num.data(), den.data(), 1.0f / snr, out.data(), pl, blk.data(), work.data(), tw.data());
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wnhost")
    src, exe = str(d / "wnhost.cpp"), str(d / "wnhost")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(build.ROOT, "include"), "-o", exe, src])
    return exe


@pytest.mark.parametrize("nx,pad,nb,n,flipped", [(8, 1, 3, 3, 0), (9, 0, 2, 2, 1), (13, 1, 4, 2, 1), (26, 1, 5, 2, 0), (15, 1, 32, 2, 1)])
def test_host_passes_match_the_contract(harness, nx, pad, nb, n, flipped):
    rng = np.random.default_rng(nx * 3 + pad)
    y = rng.standard_normal((n, nx, nx)).astype(np.float32)
    tab = table(n, nx, nx).astype(np.float32)
    am = np.column_stack([rng.uniform(-180, 360, n), rng.integers(0, 2, n)]).astype(np.float32)
    prm = np.column_stack([am[:, 0], np.zeros(n), np.zeros(n), am[:, 1]]).astype(np.float64)
    snr = 0.7
    r = subprocess.run([harness, str(nx), str(pad), str(nb), str(n), str(flipped), repr(snr)],
                       input=y.tobytes() + tab.tobytes() + am.tobytes(), capture_output=True, check=True)
    got = np.frombuffer(r.stdout, np.float32).reshape(nx, nx)
    want, _ = wiener.wiener_reference(y, prm, np.zeros(n, np.int64), 1, tab.astype(np.float64), snr, bool(pad), bool(flipped),
                                      aligned=y)
    assert np.abs(got - want[0]).max() <= 1e-5 * np.abs(want[0]).max()
