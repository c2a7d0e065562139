"""The preprocessing contract (cryo_ralib_amd/prep.py) on its float64 checker: properties of N and F, the multiplier against
literal restatements, the domains, the tool on the numpy backend and every usage error of the tool and of both drivers."""
import math

import numpy as np
import pytest

from cryo_ralib_amd import api, cli, prep, stackio


def stack(nx, n, seed, plane=True):
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:nx, 0:nx] - nx // 2
    x = 100.0 + 7.0 * rng.standard_normal((n, nx, nx))
    if plane:
        x += rng.uniform(-0.5, 0.5, (n, 1, 1)) * u + rng.uniform(-0.5, 0.5, (n, 1, 1)) * v
    return x


# ---- N

@pytest.mark.parametrize("nx,R", [(4, 1.0), (5, 2.5), (9, 3.3), (32, 16.0), (33, 12.0)])
@pytest.mark.parametrize("ramp", [False, True])
def test_background_has_mean_zero_and_sigma_one(nx, R, ramp):
    B = prep.background(nx, R)[0]
    assert B.sum() >= 4
    y = prep.normalize(stack(nx, 3, nx), R, ramp=ramp, backend="numpy")
    for i in range(3):
        assert abs(y[i][B].mean()) <= 1e-12 and abs(y[i][B].std() - 1.0) <= 1e-12


def test_the_smallest_background_is_the_four_corners():
    B = prep.background(5, 2.5)[0]
    assert B.sum() == 4 and B[0, 0] and B[0, 4] and B[4, 0] and B[4, 4]


@pytest.mark.parametrize("alpha", [3.5, -0.25])
def test_ramp_normalisation_ignores_gain_offset_and_plane(alpha):
    nx, R = 24, 9.0
    x = stack(nx, 2, 1)
    v, u = np.mgrid[0:nx, 0:nx] - nx // 2
    z = alpha * x + 17.0 + 0.3 * u - 1.1 * v
    a, b = prep.normalize(z, R, ramp=True, backend="numpy"), prep.normalize(x, R, ramp=True, backend="numpy")
    assert np.abs(a - math.copysign(1.0, alpha) * b).max() <= 1e-10
    # and invert is alpha = -1
    assert np.abs(prep.normalize(x, R, ramp=True, invert=True, backend="numpy") - prep.normalize(-x, R, ramp=True, backend="numpy")).max() <= 1e-10
    assert np.array_equal(prep.normalize(x, R, invert=True, backend="numpy"), -prep.normalize(x, R, backend="numpy"))


@pytest.mark.parametrize("ramp", [False, True])
def test_normalising_twice_is_normalising_once(ramp):
    once = prep.normalize(stack(20, 2, 4), 7.5, ramp=ramp, backend="numpy")
    assert np.abs(prep.normalize(once, 7.5, ramp=ramp, backend="numpy") - once).max() <= 1e-12


def test_a_pure_plane_is_recovered():
    nx, R, scale = 31, 10.0, 50.0
    v, u = np.mgrid[0:nx, 0:nx] - nx // 2
    x = (scale + 0.75 * u - 1.5 * v)[None]
    rng = np.random.default_rng(0)
    inside = ~prep.background(nx, R)[0]
    x[0][inside] += rng.standard_normal(inside.sum())           # what lies inside the disc does not enter the fit
    _, st = prep.normalize(x, R, ramp=True, stats=True, backend="numpy")
    assert np.abs(st[0, :3] - [scale, 0.75, -1.5]).max() <= 1e-12 * scale


def test_sigma_zero_rule():
    x = np.full((1, 8, 8), 3.0)
    x[0, 4, 4] = 9.0                                            # inside the disc
    y, st = prep.normalize(x, 2.0, invert=True, stats=True, backend="numpy")
    assert st[0, 4] == 0.0 and st[0, 3] == 3.0 and y[0, 4, 4] == -6.0 and np.all(y[0][prep.background(8, 2.0)[0]] == 0.0)


def test_a_non_finite_particle_stays_alone():
    x = stack(12, 3, 8)
    clean = prep.normalize(x, 4.0, ramp=True, stats=True, backend="numpy")
    x[1, 6, 6] = np.nan                                        # inside the disc: no sum over B sees it
    y, st = prep.normalize(x, 4.0, ramp=True, stats=True, backend="numpy")
    assert np.all(np.isnan(y[1])) and np.all(np.isnan(st[1]))
    for i in (0, 2):
        assert np.array_equal(y[i], clean[0][i]) and np.array_equal(st[i], clean[1][i])
    x[1, 6, 6] = np.inf
    assert np.all(np.isnan(prep.normalize(x, 4.0, backend="numpy")[1]))


def test_numpy_backend_copies_its_input():
    x = stack(8, 1, 3)
    keep = x.copy()
    prep.normalize(x, 3.0, backend="numpy")
    prep.fourier_filter(x, ("gauss", 0.1), backend="numpy")
    assert np.array_equal(x, keep)


# ---- F

def tanl_literal(nx, fl, aa):
    """filter_center_kernel (csrc/ralign_refine.h) term by term: fx = kx / nx, fy = kys / nx, h = 1/2 (tanh(c (d + fl)) - tanh(c (d - fl)))"""
    nxh = nx // 2 + 1
    h = np.empty((nx, nxh))
    c = math.pi / (2.0 * aa * fl)
    for ky in range(nx):
        kys = ky - nx if ky > nx // 2 else ky
        for kx in range(nxh):
            fx, fy = kx / nx, kys / nx
            d = math.sqrt(fx * fx + fy * fy)
            h[ky, kx] = 0.5 * (math.tanh(c * (d + fl)) - math.tanh(c * (d - fl)))
    return h


@pytest.mark.parametrize("nx", [8, 9])
def test_tanl_multiplier_is_the_engine_filters_formula(nx):
    g = prep.filter_multiplier(nx, nx, lowpass=("tanl", 0.2, 0.1))
    assert g.dtype == np.float64 and g.shape == (nx, nx // 2 + 1)
    assert np.abs(g - tanl_literal(nx, 0.2, 0.1)).max() <= 1e-14


def test_multiplier_at_zero_frequency():
    fl, aa, s = 0.25, 0.2, 0.1
    t0 = math.tanh(math.pi / (2.0 * aa))                        # 1/2 (tanh(k fl) - tanh(-k fl)) = tanh(pi / (2 aa))
    assert prep.filter_multiplier(16, 16, lowpass=("tanl", fl, aa))[0, 0] == pytest.approx(t0, abs=1e-15)
    assert prep.filter_multiplier(16, 32, lowpass=("gauss", s))[0, 0] == 1.0
    assert prep.filter_multiplier(16, 16, highpass=("gauss", s))[0, 0] == 0.0
    assert prep.filter_multiplier(16, 16, highpass=("tanl", fl, aa))[0, 0] == pytest.approx(1.0 - t0, abs=1e-15)
    assert prep.filter_multiplier(16, 16, lowpass=("tanl", fl, aa), highpass=("gauss", s))[0, 0] == 0.0
    g = prep.filter_multiplier(16, 32, lowpass=("gauss", s))
    assert g[3, 4] == pytest.approx(math.exp(-(25.0 / 32 ** 2) / (2 * s * s)), abs=1e-15) and g[32 - 3, 4] == g[3, 4]


@pytest.mark.parametrize("nx", [8, 9, 15, 26])
@pytest.mark.parametrize("pad", [False, True])
def test_numpy_filter_is_rfft2_times_g_irfft2(nx, pad):
    rng = np.random.default_rng(nx)
    x = rng.standard_normal((2, nx, nx))
    lp, hp = ("tanl", 0.3, 0.15), ("gauss", 0.04)
    P = 2 * nx if pad else nx
    o = (P - nx) // 2
    g = prep.filter_multiplier(nx, P, lp, hp)
    for i in range(2):
        big = np.zeros((P, P))
        big[o:o + nx, o:o + nx] = x[i]
        want = np.fft.irfft2(np.fft.rfft2(big) * g, s=(P, P))[o:o + nx, o:o + nx]
        got = prep.fourier_filter(x[i:i + 1], lp, hp, pad=pad, backend="numpy")[0]
        assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max()      # g rounded to float32 once: 6e-8 relative


def test_an_all_pass_filter_returns_the_input():
    x = np.random.default_rng(2).standard_normal((1, 12, 12))
    y = prep.fourier_filter(x, lowpass=("tanl", 0.999, 0.01), backend="numpy")
    assert np.abs(y - x).max() <= 1e-12


# ---- domains

@pytest.mark.parametrize("nx,R", [(3, 1.0), (1025, 10.0), (8, 0.999), (8, 4.001), (8, float("nan")), (8, float("inf")), (8, "2"), (8, True)])
def test_normalize_domain(nx, R):
    with pytest.raises(prep.PrepError):
        prep.normalize(np.zeros((1, nx, nx), np.float32), R, backend="numpy")


def test_normalize_domain_edges_are_inside():
    for nx, R in ((4, 1.0), (4, 2.0), (1024, 512.0)):
        prep._check_radius(nx, R)


@pytest.mark.parametrize("kw", [dict(), dict(lowpass=("tanl", 0.0, 0.1)), dict(lowpass=("tanl", 1.0, 0.1)), dict(lowpass=("tanl", 0.2, 0.0)),
                                dict(lowpass=("tanl", 0.2)), dict(lowpass=("gauss", 0.0)), dict(lowpass=("gauss", -1.0)),
                                dict(highpass=("gauss", float("nan"))), dict(highpass=("tanl", float("inf"), 0.1)),
                                dict(highpass=("tanl", 0.2, float("inf"))), dict(lowpass=("box", 0.1)), dict(lowpass="tanl"),
                                dict(lowpass=("gauss", 0.1, 0.2)), dict(lowpass=("gauss", 0.1), pad=1)])
def test_filter_domain(kw):
    with pytest.raises(prep.PrepError):
        prep.fourier_filter(np.zeros((1, 8, 8), np.float32), backend="numpy", **kw)


@pytest.mark.parametrize("nx", [1, 1025])
def test_filter_box_domain(nx):
    with pytest.raises(prep.PrepError):
        prep.fourier_filter(np.zeros((1, nx, nx), np.float32), ("gauss", 0.1), backend="numpy")
    with pytest.raises(prep.PrepError):
        prep.filter_multiplier(nx, nx, ("gauss", 0.1))


def test_filter_box_edges_and_multiplier_size():
    assert prep.fourier_filter(np.ones((1, 2, 2)), ("gauss", 0.1), backend="numpy").shape == (1, 2, 2)
    assert prep.filter_multiplier(1024, 2048, ("gauss", 0.1)).shape == (2048, 1025)
    with pytest.raises(prep.PrepError):
        prep.filter_multiplier(8, 12, ("gauss", 0.1))


@pytest.mark.parametrize("shape", [(8, 8), (2, 8, 9), (1, 2, 8, 8)])
def test_stack_shape(shape):
    with pytest.raises(prep.PrepError):
        prep.normalize(np.zeros(shape), 2.0, backend="numpy")
    with pytest.raises(prep.PrepError):
        prep.fourier_filter(np.zeros(shape), ("gauss", 0.1), backend="numpy")


def test_flags_and_backend():
    x = np.zeros((1, 8, 8))
    for kw in (dict(ramp=1), dict(invert="yes"), dict(stats=None), dict(backend="cpu")):
        with pytest.raises(prep.PrepError):
            prep.normalize(x, 2.0, **{"backend": "numpy", **kw})
    with pytest.raises(prep.PrepError):
        prep.fourier_filter(x, ("gauss", 0.1), backend="torch")


def test_api_re_exports():
    x = stack(8, 1, 0)
    assert np.array_equal(api.normalize_background(x, 3.0, backend="numpy"), prep.normalize(x, 3.0, backend="numpy"))
    assert np.array_equal(api.fourier_filter(x, lowpass=("gauss", 0.2), backend="numpy"), prep.fourier_filter(x, ("gauss", 0.2), backend="numpy"))
    assert "ra_prep_normalize" in api.EXPORTED_SYMBOLS and "ra_prep_filter" in api.EXPORTED_SYMBOLS


# ---- the tool

def test_tool_numpy_backend_writes_what_the_api_returns(tmp_path):
    x = stack(16, 7, 6).astype(np.float32)
    src, dst, sts = str(tmp_path / "in.mrcs"), str(tmp_path / "out.npy"), str(tmp_path / "st.npy")
    stackio.write_stack(src, x)
    argv = [src, dst, "--norm_bg", "6", "--ramp", "--invert", "--lowpass_tanl", "0.3", "0.1", "--highpass_gauss", "0.02", "--filter_pad",
            "--box", "12", "--stats", sts, "--batch", "3", "--backend", "numpy"]
    assert prep.main(argv) == 0
    from cryo_ralib_amd import resize
    y, st = prep.normalize(x, 6.0, ramp=True, invert=True, stats=True, backend="numpy")
    y = prep.fourier_filter(y, ("tanl", 0.3, 0.1), ("gauss", 0.02), pad=True, backend="numpy")
    y = resize.resize(y, 12, backend="numpy")
    assert np.array_equal(stackio.read_stack(dst), y.astype(np.float32))
    assert np.array_equal(np.load(sts), st)


def test_tool_res_converts_angstrom_and_invert_alone_negates(tmp_path):
    x = stack(16, 2, 7).astype(np.float32)
    src, dst = str(tmp_path / "in.npy"), str(tmp_path / "out.npy")
    stackio.write_stack(src, x)
    assert prep.main([src, dst, "--lowpass_gauss", "8", "--res", "--apix", "2", "--backend", "numpy"]) == 0
    assert np.array_equal(stackio.read_stack(dst), prep.fourier_filter(x, ("gauss", 0.25), backend="numpy").astype(np.float32))
    assert prep.main([src, dst, "--invert", "--backend", "numpy"]) == 0
    assert np.array_equal(stackio.read_stack(dst), -x)


@pytest.fixture
def small_stack(tmp_path):
    src = str(tmp_path / "in.npy")
    stackio.write_stack(src, stack(8, 2, 0).astype(np.float32))
    return src


@pytest.mark.parametrize("argv", [
    [],                                                         # no step requested
    ["--ramp"], ["--ramp", "--invert"],                         # --ramp without --norm_bg
    ["--lowpass_gauss", "10", "--res"],                         # --res without --apix
    ["--norm_bg", "0.5"], ["--norm_bg", "4.5"], ["--norm_bg", "nan"],
    ["--lowpass_tanl", "0", "0.1"], ["--lowpass_tanl", "1", "0.1"], ["--lowpass_tanl", "0.2", "0"],
    ["--highpass_tanl", "0.2", "-1"], ["--lowpass_gauss", "0"], ["--highpass_gauss", "-0.1"], ["--highpass_gauss", "inf"],
    ["--lowpass_gauss", "0", "--res", "--apix", "1.5"],
    ["--lowpass_gauss", "0.1", "--lowpass_tanl", "0.2", "0.1"],
    ["--box", "0"], ["--box", "1025"], ["--invert", "--batch", "0"],
    ["--norm_bg", "3", "--ctf", "table.npy", "--backend", "numpy"],                  # --ctf with the numpy backend
])
def test_tool_usage_errors_exit_with_status_2_before_the_device(small_stack, tmp_path, argv, monkeypatch):
    monkeypatch.setattr(api, "load_library", lambda *a, **k: pytest.fail("the device was touched"))
    with pytest.raises(SystemExit) as e:
        prep.main([small_stack, str(tmp_path / "out.npy")] + argv)
    assert e.value.code == 2


# ---- the drivers

@pytest.mark.parametrize("argv", [["--norm_ramp"], ["--norm_ramp", "--invert"], ["--norm_bg", "0.5"], ["--norm_bg", "nan"]])
def test_drivers_usage_errors_exit_with_status_2(tmp_path, argv, monkeypatch):
    monkeypatch.setattr(cli, "_setup", lambda args: pytest.fail("the device was touched"))
    with pytest.raises(SystemExit) as e:
        cli.main_mref([str(tmp_path / "nostack.hdf"), str(tmp_path / "norefs.hdf"), str(tmp_path / "out")] + argv)
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.main_reffree([str(tmp_path / "nostack.hdf"), str(tmp_path / "out")] + argv)
    assert e.value.code == 2


def test_drivers_parse_the_new_options():
    import argparse
    p = argparse.ArgumentParser()
    cli._common(p)
    args = p.parse_args(["--norm_bg", "40", "--norm_ramp", "--invert"])
    assert cli._check_prep(p, args) == dict(normalize_bg=40.0, normalize_ramp=True, invert=True)
    assert cli._check_prep(p, p.parse_args([])) == dict(normalize_bg=None, normalize_ramp=False, invert=False)
