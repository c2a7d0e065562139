"""Per-particle agreement scores and class pruning without a GPU: the float64 contract (wiener.score_reference, select) on cases
whose answer is known -- the leave-one-out identity, pure-noise classes, a seeded class with replaced particles, invariances --
the argument checks of the contract, the tool and the drivers before any device work, and the score pass of
csrc/ralign_wiener.h compiled for the host and run as one sequential thread against the contract."""
import os
import subprocess

import numpy as np
import pytest

from cryo_ralib_amd import build, cli, ctf, synth, wiener

from test_wiener_cpu import physical_case, table

CSRC = os.path.join(build.HERE, "csrc")


def _noise_case(n, nx, k, seed, lab=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nx, nx))
    prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.integers(0, 2, n)])
    return x, prm, (rng.integers(0, k, n) if lab is None else np.asarray(lab)), table(n, nx, seed + 1)


def _aligned(x, prm):
    return np.array([synth.rot_shift2d_np(x[i], *prm[i, :3], int(prm[i, 3])) for i in range(len(x))], np.float64)


def _reg(k, P, seed):
    return np.random.default_rng(seed).uniform(0.2, 3.0, (k, P // 2 + 1))


@pytest.mark.parametrize("nx,pad", [(12, True), (13, False)])
@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("shell_term", [False, True])
def test_leave_one_out_is_the_score_against_sums_without_the_particle(nx, pad, flipped, shell_term):
    """float64 against float64: the bar is 1e-12 of sqrt(E F); this test prints about 1e-16"""
    n, k = 14, 2
    x, prm, lab, tab = _noise_case(n, nx, k, nx + flipped)
    al = _aligned(x, prm)
    P = 2 * nx if pad else nx
    reg = _reg(k, P, 5) if shell_term else None
    num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, pad, flipped, aligned=al)
    got = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, 1.7, reg, True, None, pad, flipped, aligned=al)
    worst = 0.0
    for i in range(n):
        rest = np.arange(n) != i
        n1, d1, c1 = wiener.class_sums_reference(x[rest], prm[rest], lab[rest], k, tab[rest], pad, flipped, aligned=al[rest])
        one = wiener.score_reference(x[i:i + 1], prm[i:i + 1], lab[i:i + 1], k, tab[i:i + 1], n1, d1, c1, 1.7, reg, False, None, pad,
                                     flipped, aligned=al[i:i + 1])
        X, E, F = one["sums"][0]
        worst = max(worst, np.abs(got["sums"][i] - one["sums"][0]).max() / np.sqrt(E * F))
        assert abs(got["cc"][i] - one["cc"][0]) <= 1e-12
    print("leave-one-out identity: max |difference| / sqrt(E F) = %.3g" % worst)
    assert worst <= 1e-12


def test_pure_noise_classes_score_zero_only_with_leave_one_out():
    """white noise: the particle's own term dominates the plain score, so its mean is 1/sqrt(n_j) (within 25 %), and leave-one-out
    brings it at least five times closer to 0.  This test prints 0.492 and 0.249 against -0.003 and -0.0002"""
    nx, k = 24, 6
    for m in (4, 16):
        lab = np.repeat(np.arange(k), m)
        x, prm, lab, tab = _noise_case(k * m, nx, k, 40 + m, lab)
        al = _aligned(x, prm)
        num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, True, False, aligned=al)
        plain = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, leave_one_out=False, aligned=al)["cc"].mean()
        loo = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, leave_one_out=True, aligned=al)["cc"].mean()
        print("classes of %d: mean cc %.3f without leave-one-out (1/sqrt(n) = %.3f), %.4f with it" % (m, plain, m ** -0.5, loo))
        assert abs(plain - m ** -0.5) <= 0.25 * m ** -0.5
        assert abs(loo) <= abs(plain) / 5


def junk_case():
    """two classes of 60 CTF-modulated particles (seeds 5 and 9, nx = 32, ou = 13, sigma = 2), 6 of each replaced by phase-flipped
    white noise of the stack's std; returns (particles, params, labels, table, replaced mask)"""
    parts, prms, tabs = [], [], []
    for seed in (5, 9):
        fl, prm, tab, _, _ = physical_case(60, nx=32, ou=13, seed=seed, sigma=2.0)
        parts.append(fl); prms.append(prm); tabs.append(tab)
    x, prm, tab = np.concatenate(parts), np.concatenate(prms), np.concatenate(tabs)
    lab = np.repeat([0, 1], 60)
    rng = np.random.default_rng(1)
    bad = np.concatenate([rng.choice(60, 6, replace=False), 60 + rng.choice(60, 6, replace=False)])
    x[bad] = ctf.flip_reference(rng.normal(0, x.std(), (12, 32, 32)), tab[bad])
    mask = np.zeros(120, bool)
    mask[bad] = True
    return x, prm, lab, tab, mask


def test_replaced_particles_score_below_every_member_and_are_pruned():
    """every replaced particle scores below every member (this test prints max 0.170 against min 0.272), so keeping the best 90 %
    of each class drops exactly the replaced ones"""
    x, prm, lab, tab, bad = junk_case()
    al = _aligned(x, prm)
    num, den, counts = wiener.class_sums_reference(x, prm, lab, 2, tab, True, True, aligned=al)
    cc = wiener.score_reference(x, prm, lab, 2, tab, num, den, counts, snr=2.0, flipped=True, aligned=al)["cc"]
    print("replaced: max cc %.3f; members: min cc %.3f" % (cc[bad].max(), cc[~bad].min()))
    assert cc[bad].max() < cc[~bad].min()
    keep = wiener.select(cc, lab, 2, keep=0.9)
    assert np.array_equal(~keep, bad)


def test_scaling_a_particle_keeps_its_cc_and_scales_its_amplitude():
    n, nx, k = 12, 16, 2
    x, prm, lab, tab = _noise_case(n, nx, k, 8)
    x[lab == 0] += 2 * x[np.nonzero(lab == 0)[0][0]]
    al = _aligned(x, prm)
    num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, aligned=al)
    a = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, aligned=al)
    i, f = int(np.nonzero(lab == 0)[0][2]), 2.5
    x2, al2 = x.copy(), al.copy()
    x2[i] *= f
    al2[i] *= f
    num2, den2, _ = wiener.class_sums_reference(x2, prm, lab, k, tab, aligned=al2)
    b = wiener.score_reference(x2, prm, lab, k, tab, num2, den2, counts, aligned=al2)
    assert abs(b["cc"][i] - a["cc"][i]) <= 1e-6
    assert abs(b["scale"][i] - f * a["scale"][i]) <= 1e-6 * abs(f * a["scale"][i])


def test_one_shell_band_is_the_sum_over_that_shell():
    n, nx, k, pad = 9, 14, 2, True
    x, prm, lab, tab = _noise_case(n, nx, k, 12)
    al = _aligned(x, prm)
    P, o = 2 * nx, nx // 2
    num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, pad, True, aligned=al)
    s, g = wiener.shells(P)
    tabal = wiener.aligned_table(tab, prm)
    for shell in (0, 5, P // 2):
        got = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, 0.8, None, True, (shell, shell), pad, True, aligned=al)
        for i in (0, 4):
            big = np.zeros((P, P))
            big[o:o + nx, o:o + nx] = al[i]
            Y, c = np.fft.rfft2(big), ctf.ctf_grid(tabal[i], nx, P)
            X = E = F = 0.0
            for iy, ix in zip(*np.nonzero(s == shell)):
                w = abs(c[iy, ix])
                M = w * (num[lab[i]][iy, ix] - w * Y[iy, ix]) / (max(den[lab[i]][iy, ix] - c[iy, ix] ** 2, 0.0) + 1 / 0.8)
                X += g[iy, ix] * (Y[iy, ix] * np.conj(M)).real
                E += g[iy, ix] * abs(Y[iy, ix]) ** 2
                F += g[iy, ix] * abs(M) ** 2
            assert np.allclose(got["sums"][i], [X, E, F], rtol=1e-12, atol=1e-12 * np.sqrt(E * F))


def test_unit_ctf_and_large_snr_give_the_correlation_with_the_class_mean(monkeypatch):
    n, nx = 7, 18
    x, prm, _, tab = _noise_case(n, nx, 1, 21)
    x += 0.5 * np.random.default_rng(2).standard_normal((nx, nx))
    lab = np.zeros(n, np.int64)
    al = _aligned(x, prm)
    monkeypatch.setattr(ctf, "ctf_grid", lambda row, nx, P: np.ones((P, P // 2 + 1)))
    for pad in (True, False):
        P = 2 * nx if pad else nx
        num, den, counts = wiener.class_sums_reference(x, prm, lab, 1, tab, pad, aligned=al)
        got = wiener.score_reference(x, prm, lab, 1, tab, num, den, counts, 1e12, None, False, (0, P // 2), pad, aligned=al)
        # shells 0 .. P/2 of the padded image: the full plane without the corners beyond P/2
        s, g = wiener.shells(P)
        o = (P - nx) // 2
        mean = np.zeros((P, P))
        mean[o:o + nx, o:o + nx] = al.mean(0)
        Fm = np.where(s <= P // 2, np.fft.rfft2(mean), 0)
        for i in range(n):
            big = np.zeros((P, P))
            big[o:o + nx, o:o + nx] = al[i]
            Fy = np.where(s <= P // 2, np.fft.rfft2(big), 0)
            a, b = np.fft.irfft2(Fy, s=(P, P)), np.fft.irfft2(Fm, s=(P, P))      # the band-limited images
            want = (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())
            assert abs(got["cc"][i] - want) <= 1e-9
            assert abs(got["scale"][i] - (a * b).sum() / (b * b).sum()) <= 1e-9


def test_select():
    nan = np.nan
    cc = np.array([0.5, 0.5, 0.5, 0.1, nan, 0.9, 0.2, 0.7])
    lab = np.array([0, 0, 0, 0, 0, 1, 1, 3])
    # ties by the lower index: ceil(0.5 * 4) = 2 of class 0's scored members, the first two of the three 0.5s
    assert wiener.select(cc, lab, 4, keep=0.5).tolist() == [True, True, False, False, True, True, False, True]
    assert wiener.select(cc, lab, 4, min_cc=0.5).tolist() == [True, True, True, False, True, True, False, True]
    assert wiener.select(cc, lab, 4, keep=0.75, min_cc=0.6).tolist() == [False, False, False, False, True, True, False, True]
    assert wiener.select(cc, lab, 4).all()                                   # nothing asked: everything stays
    assert wiener.select(cc, lab, 4, keep=1.0).all()
    assert wiener.select(cc[7:], lab[7:], 4, keep=0.01).tolist() == [True]      # a class of one: ceil keeps it; class 2 is empty
    assert wiener.select(np.zeros(0), np.zeros(0, np.int64), 2, keep=0.5).shape == (0,)
    for kw in ({"keep": 0.0}, {"keep": 1.5}, {"keep": nan}, {"min_cc": nan}):
        with pytest.raises(wiener.WienerError):
            wiener.select(cc, lab, 4, **kw)
    with pytest.raises(wiener.WienerError):
        wiener.select(cc, lab, 3, keep=0.5)
    with pytest.raises(wiener.WienerError):
        wiener.select(cc, lab[:3], 4, keep=0.5)


def test_small_classes_are_unscored():
    n, nx, k = 9, 12, 4
    lab = np.array([0, 0, 0, 0, 0, 1, 1, 2, 0])                # sizes 6, 2, 1, 0
    x, prm, lab, tab = _noise_case(n, nx, k, 3, lab)
    al = _aligned(x, prm)
    num, den, counts = wiener.class_sums_reference(x, prm, lab, k, tab, aligned=al)
    r = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, aligned=al)
    assert np.isnan(r["cc"][7]) and np.isnan(r["scale"][7]) and np.isfinite(r["cc"][lab != 2]).all()
    assert r["sums"][7, 0] == 0 and r["sums"][7, 2] == 0 and r["sums"][7, 1] > 0          # nobody left to compare with
    r = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, min_count=3, aligned=al)
    assert np.isnan(r["cc"][lab != 0]).all() and np.isfinite(r["cc"][lab == 0]).all()
    r = wiener.score_reference(x, prm, lab, k, tab, num, den, counts, leave_one_out=False, aligned=al)
    assert np.isfinite(r["cc"]).all() and r["cc"][7] > 0.5          # a class of one against itself


def test_argument_errors():
    n, nx, k = 4, 16, 2
    x, prm, lab, tab = np.zeros((n, nx, nx)), np.zeros((n, 4)), np.zeros(n, np.int64), table(n, nx, 1)
    num, den, counts = np.zeros((k, 32, 17), complex), np.zeros((k, 32, 17)), np.array([4, 0])
    ok = dict(snr=1.0, reg=None, band=None)
    for kw in ({"band": (-1, 3)}, {"band": (3, 2)}, {"band": (0, 17)}, {"band": (1.0, 3)}, {"band": 3}, {"snr": 0.0}, {"snr": np.nan},
               {"reg": np.zeros((k, 16))}, {"reg": -np.ones((k, 17))}, {"reg": np.full((k, 17), np.inf)}):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(wiener.WienerError):
            wiener.score_reference(x, prm, lab, k, tab, num, den, counts, a["snr"], a["reg"], True, a["band"])
    with pytest.raises(wiener.WienerError):
        wiener.score_reference(x, prm, lab, k, tab, num[:, :16], den, counts)
    with pytest.raises(wiener.WienerError):
        wiener.score_reference(x, prm, lab, k, tab, num, den, counts[:1])
    with pytest.raises(wiener.WienerError):
        wiener.score_reference(x, prm, lab + 2, k, tab, num, den, counts)
    with pytest.raises(wiener.WienerError):                  # the per-shell term is the SSNR path's: k <= 512
        wiener.check_score(nx, True, 513, 1.0, np.zeros((513, 17)), None)
    assert wiener.check_score(nx, True, k, 1.0, None, None)[:2] == (1, 16)
    assert wiener.check_score(nx, False, k, 1.0, None, (0, 8))[:2] == (0, 8)


def test_tool_and_drivers_refuse_bad_score_options_before_the_device(tmp_path, capsys):
    n, nx = 5, 16
    stack, prm, tab = tmp_path / "s.npy", tmp_path / "p.txt", tmp_path / "t.npy"
    np.save(stack, np.zeros((n, nx, nx), np.float32))
    np.savetxt(prm, np.column_stack([np.arange(n), np.zeros((n, 4)), np.arange(n) % 2]))
    np.save(tab, table(n, nx, 2))
    base = [str(stack), str(prm), str(tab), str(tmp_path / "o.npy")]
    sc = ["--scores", str(tmp_path / "sc.npz")]
    for extra in (["--keep", "0.9"], ["--min_cc", "0.1"], ["--band", "1", "4"], ["--no_leave_one_out"], sc + ["--keep", "0"],
                  sc + ["--keep", "1.5"], sc + ["--band", "0", "17"], sc + ["--band", "5", "4"], sc + ["--band", "-1", "4"],
                  sc + ["--nopad", "--band", "1", "9"]):
        with pytest.raises(SystemExit) as e:
            wiener.main(base + extra)
        assert e.value.code == 2, extra
    assert not os.path.exists(str(tmp_path / "o.npy")) and not os.path.exists(str(tmp_path / "sc.npz"))
    np.save(tmp_path / "refs.npy", np.zeros((2, nx, nx), np.float32))
    for main, pos in ((cli.main_mref, [str(stack), str(tmp_path / "refs.npy"), str(tmp_path / "out")]),
                      (cli.main_reffree, [str(stack), str(tmp_path / "out")])):
        with pytest.raises(SystemExit) as e:
            main(pos + ["--phase_flip", str(tab), "--wiener_scores"])
        assert e.value.code == 2
    assert not os.path.exists(str(tmp_path / "out"))
    capsys.readouterr()


HARNESS = r"""
#include "ralign_wiener.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace ralign;
// argv: nx pad nb n flipped loo shell_term snr s_lo s_hi count; stdin: n*nx*nx aligned images, n*9 table, n*2 (alpha, mirror),
// num [P][H] float2, den [P][H], reg [P/2 + 1]; stdout: sums [n][3] double against that one class
int main(int argc, char **argv)
{
    const int nx = atoi(argv[1]), pad = atoi(argv[2]), nb = atoi(argv[3]), n = atoi(argv[4]), flipped = atoi(argv[5]);
    const int loo = atoi(argv[6]), shell_term = atoi(argv[7]);
    const double tau = 1.0 / (double)(float)atof(argv[8]);
    const int s_lo = atoi(argv[9]), s_hi = atoi(argv[10]), count = atoi(argv[11]);
    PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nrad == 0 && pl.P > 1) return 2;
    pl.nb = nb;
    const int P = pl.P, H = pl.H;
    std::vector<float> img((size_t)n * nx * nx), tab((size_t)n * 9), am((size_t)n * 2), den((size_t)P * H), reg(P / 2 + 1);
    std::vector<float2> num((size_t)P * H);
    if (fread(img.data(), 4, img.size(), stdin) != img.size() || fread(tab.data(), 4, tab.size(), stdin) != tab.size() ||
        fread(am.data(), 4, am.size(), stdin) != am.size() || fread(num.data(), 8, num.size(), stdin) != num.size() ||
        fread(den.data(), 4, den.size(), stdin) != den.size() || fread(reg.data(), 4, reg.size(), stdin) != reg.size()) return 3;
    std::vector<float2> tw(P), work((size_t)2 * nb * P), blk((size_t)nx * H), spec((size_t)H * P);
    for (int t = 0; t < P; t++) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / P), (float)sin(-2.0 * M_PI * t / P));
    const PfCtx cx{0, 1};
    std::vector<double> out((size_t)n * 3, 0.0);
    for (int p = 0; p < n; p++) {
        wn_forward(cx, &img[(size_t)p * nx * nx], spec.data(), pl, blk.data(), work.data(), tw.data());
        const WnCtf c = wn_constants(&tab[(size_t)p * 9], nx, P, am[2 * p], am[2 * p + 1] != 0.f);
        for (int kx = 0; kx < H; kx++)
            for (int n_ = 0; n_ < P; n_++)
                wn_score_at(spec.data(), P, H, n_, kx, c, flipped, num.data(), den.data(), loo != 0, !loo || count >= 2, tau,
                            shell_term ? reg.data() : nullptr, s_lo, s_hi, &out[(size_t)p * 3]);
    }
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wnscore")
    src, exe = str(d / "wnscore.cpp"), str(d / "wnscore")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call([build.hipcc_path(), "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(build.ROOT, "include"), "-o", exe, src])
    return exe


@pytest.mark.parametrize("nx,pad,nb,n,flipped,loo,shell_term,band",
                         [(8, 1, 3, 5, 0, 1, 0, None), (9, 0, 2, 4, 1, 1, 1, (0, 4)), (13, 1, 4, 3, 1, 0, 0, (2, 7)),
                          (26, 1, 5, 4, 0, 1, 1, None), (15, 1, 32, 1, 1, 1, 0, None)])
def test_host_score_pass_matches_the_contract(harness, nx, pad, nb, n, flipped, loo, shell_term, band):
    """the device's arithmetic (float32 spectra and CTF sine, double sums) against the float64 contract on the same float32 class
    sums: 1e-5 of sqrt(E F), the bar of the other Wiener host passes"""
    rng = np.random.default_rng(nx * 7 + pad)
    y = rng.standard_normal((n, nx, nx)).astype(np.float32)
    y += rng.standard_normal((nx, nx)).astype(np.float32)
    tab = table(n, nx, nx).astype(np.float32)
    am = np.column_stack([rng.uniform(-180, 360, n), rng.integers(0, 2, n)]).astype(np.float32)
    prm = np.column_stack([am[:, 0], np.zeros(n), np.zeros(n), am[:, 1]]).astype(np.float64)
    lab = np.zeros(n, np.int64)
    P = 2 * nx if pad else nx
    num, den, counts = wiener.class_sums_reference(y, prm, lab, 1, tab.astype(np.float64), bool(pad), bool(flipped), aligned=y)
    num32, den32 = num.astype(np.complex64), den.astype(np.float32)
    reg = _reg(1, P, nx).astype(np.float32)
    snr = float(np.float32(0.7))
    lo, hi = band if band else (1, P // 2)
    r = subprocess.run([harness] + [str(v) for v in (nx, pad, nb, n, flipped, loo, shell_term, repr(snr), lo, hi, n)],
                       input=y.tobytes() + tab.tobytes() + am.tobytes() + num32.tobytes() + den32.tobytes() + reg.tobytes(),
                       capture_output=True, check=True)
    got = np.frombuffer(r.stdout, np.float64).reshape(n, 3)
    want = wiener.score_reference(y, prm, lab, 1, tab.astype(np.float64), num32, den32, counts, snr,
                                  reg.astype(np.float64) if shell_term else None, bool(loo), band, bool(pad), bool(flipped), aligned=y)
    norm = np.sqrt(want["sums"][:, 1] * want["sums"][:, 2])
    if n == 1 and loo:
        assert got[0, 0] == 0 and got[0, 2] == 0 and abs(got[0, 1] - want["sums"][0, 1]) <= 1e-5 * want["sums"][0, 1]
        return
    assert (norm > 0).all()
    err = np.abs(got - want["sums"]).max(1) / norm
    print("host score pass: max |difference| / sqrt(E F) = %.3g" % err.max())
    assert err.max() <= 1e-5
