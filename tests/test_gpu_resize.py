"""Fourier resizing on the device (ra_fourier_resize / api.fourier_resize): agreement with the float64 checker, bitwise
reproducibility and batch independence, isolation of bad images, the domain errors, the tool with --ctf, and a multi-reference
alignment of binned particles."""
import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, resize, stackio, synth
from cryo_ralib_amd.mref import MrefAligner

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RA_ERR_ARG = -1                  # include/ralign.h
PAIRS = [(64, 32), (64, 31), (63, 32), (97, 31), (32, 64), (31, 64), (32, 47), (90, 90), (360, 90), (256, 64), (512, 128),
         (1024, 256), (90, 360), (90, 1), (1, 7), (130, 129), (200, 250)]
WORST = {}


def dev_resize(x, m):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    y = api.fourier_resize(t, m)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("nx,m", PAIRS)
def test_matches_the_float64_checker(nx, m):
    n = 2 if nx * max(nx, m) >= 512 * 512 else 5
    x = np.random.default_rng(nx * 7 + m).standard_normal((n, nx, nx)).astype(np.float32)
    y = dev_resize(x, m)
    ref = resize.resize(x.astype(np.float64), m, backend="numpy")
    assert y.shape == (n, m, m)
    err = np.abs(y - ref).reshape(n, -1).max(1) / np.abs(x).reshape(n, -1).max(1)
    WORST[(nx, m)] = float(err.max())
    print("%d -> %d: max|y - y_ref| / max|x| = %.3g" % (nx, m, err.max()))
    assert (err <= 2e-5).all()


def test_report_worst_errors():
    if WORST:
        print("worst per-image error / max|x|: " + ", ".join("%d->%d %.2g" % (a, b, e) for (a, b), e in sorted(WORST.items())))


def test_identity_and_constant():
    x = np.random.default_rng(1).standard_normal((3, 90, 90)).astype(np.float32)
    assert np.abs(dev_resize(x, 90) - x).max() <= 2e-5 * np.abs(x).max()
    c = np.full((2, 128, 128), 1.5, np.float32)
    for m in (64, 45, 200):
        assert np.abs(dev_resize(c, m) - 1.5).max() < 1e-5


def test_bitwise_reproducible_and_independent_of_the_batch():
    rng = np.random.default_rng(2)
    for nx, m in ((128, 64), (360, 90), (90, 360)):
        n = 1000 if nx * max(nx, m) <= 128 * 128 else 200
        x = rng.standard_normal((n, nx, nx)).astype(np.float32)
        a, b = dev_resize(x, m), dev_resize(x, m)
        assert np.array_equal(a, b)
        k = n // 2 + 37
        alone = dev_resize(x[k:k + 1], m)
        assert np.array_equal(alone[0], a[k])
        first = dev_resize(x[:1], m)
        assert np.array_equal(first[0], a[0])
        # another stream gives the same bits
        s = torch.cuda.Stream(DEV)
        t = torch.from_numpy(x[:50]).to(DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            y = api.fourier_resize(t, m)
        s.synchronize()
        assert np.array_equal(y.cpu().numpy(), a[:50])


def test_bad_images_stay_alone():
    x = np.random.default_rng(3).standard_normal((8, 100, 100)).astype(np.float32)
    clean = dev_resize(x, 50)
    bad = x.copy()
    bad[3, 40, 41] = np.nan
    bad[5, 0, 0] = np.inf
    got = dev_resize(bad, 50)
    for i in range(8):
        if i in (3, 5):
            assert not np.isfinite(got[i]).all()
        else:
            assert np.array_equal(got[i], clean[i])


def test_out_of_domain_arguments_are_refused():
    L = api.load_library()
    x = torch.ones((4, 16, 16), device=DEV)
    y = torch.full((4, 8, 8), 7.0, device=DEV)
    big = torch.full((4, 16, 16), 7.0, device=DEV)
    vp = api.ctypes.c_void_p
    xp, yp = vp(x.data_ptr()), vp(y.data_ptr())
    for n, nx, m in ((-1, 16, 8), (4, 0, 8), (4, 16, 0), (4, 1025, 8), (4, 16, 1025)):
        assert L.ra_fourier_resize(xp, n, nx, m, yp, None) == RA_ERR_ARG, (n, nx, m)
    assert L.ra_fourier_resize(None, 4, 16, 8, yp, None) == RA_ERR_ARG
    assert L.ra_fourier_resize(xp, 4, 16, 8, None, None) == RA_ERR_ARG
    assert L.ra_fourier_resize(xp, 4, 16, 16, xp, None) == RA_ERR_ARG                             # in place
    assert L.ra_fourier_resize(xp, 4, 16, 16, vp(x.data_ptr() + 4 * 16 * 16 * 3), None) == RA_ERR_ARG  # partial overlap
    assert L.ra_fourier_resize(vp(big.data_ptr() + 4 * 8), 3, 16, 8, vp(big.data_ptr()), None) == RA_ERR_ARG
    assert L.ra_fourier_resize(None, 0, 16, 8, None, None) == 0                                    # n == 0: no-op
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((big == 7).all())
    with pytest.raises(api.EngineError):
        api.fourier_resize(x, 0)
    with pytest.raises(api.EngineError):
        api.fourier_resize(x, 2000)
    with pytest.raises(api.EngineError):
        api.fourier_resize(torch.ones((1, 1100, 1100), device=DEV), 64)


def test_numpy_input_to_the_device_backend():
    x = np.random.default_rng(4).standard_normal((3, 40, 40)).astype(np.float32)
    y = resize.resize(x, 20)
    assert isinstance(y, torch.Tensor) and y.is_cuda
    assert np.array_equal(y.cpu().numpy(), dev_resize(x, 20))
    assert np.array_equal(resize.resize(x[0], 20).cpu().numpy(), dev_resize(x[:1], 20)[0])


def test_tool_with_ctf_is_phase_flip_then_resize(tmp_path, capsys):
    rng = np.random.default_rng(5)
    n, nx, m = 9, 96, 48
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    tab = np.zeros((n, 9), np.float32)
    tab[:] = [nx, 1.2, 0, 0, 0, 300.0, 2.7, 0.1, 0.0]
    tab[:, 2] = rng.uniform(10000, 30000, n)
    tab[:, 3] = tab[:, 2] - rng.uniform(0, 1500, n)
    tab[:, 4] = rng.uniform(0, 180, n)
    src, ctfp = str(tmp_path / "in.mrcs"), str(tmp_path / "ctf.npy")
    stackio.write_stack(src, x)
    np.save(ctfp, tab)
    for extra, pad in (([], True), (["--nopad"], False)):
        out = str(tmp_path / "out.npy")
        assert resize.main([src, out, "--box", str(m), "--ctf", ctfp, "--batch", "4"] + extra) == 0
        assert "96 -> 48" in capsys.readouterr().out
        got = np.load(out)
        t = torch.from_numpy(x).to(DEV)
        api.phase_flip(t, tab, pad=pad)
        flipped = t.cpu().numpy()
        want = resize.resize(flipped.astype(np.float64), m, backend="numpy")
        assert np.abs(got - want).max() <= 2e-5 * np.abs(flipped).max()
        assert np.array_equal(got, dev_resize(flipped, m))
    # without --ctf the tool is the plain resize
    out = str(tmp_path / "plain.hdf")
    assert resize.main([src, out, "--box", str(m)]) == 0
    assert np.array_equal(stackio.read_stack(out), dev_resize(x, m))


def test_binned_particles_align_to_binned_references():
    nx, ou, n, nref, m = 128, 52, 60, 3, 64
    refs = synth.make_references(nref, nx, ou, seed=11)
    parts, truth = synth.make_particles(refs, n, 4, 4, 0.25, ou=ou)
    small = dev_resize(parts, m)
    srefs = dev_resize(refs, m)
    al = MrefAligner(small, srefs, ou // 2, 2, 2, 1.0)
    al.search()
    al.engine.sync()
    p = al.params()
    al.close()
    assert (p["ref_id"] == truth["cls"]).all(), int((p["ref_id"] != truth["cls"]).sum())
    assert (p["mirror"] == truth["mir"]).all(), int((p["mirror"] != truth["mir"]).sum())
