"""2SDR denoising on the device: ra_sdr_reconstruct entry by entry on the inputs of tests/test_sdr_denoise_cpu.py (whose
properties that file asserts without a GPU), then sdr.transform / reconstruct / denoise / eigenimages and the tool.

Integer cases are compared for equality with the float64 product; real-valued cases use that file's entry-wise bound and print
their largest error / bound ratio.  Every output is the interior of a sentinel-filled buffer (tests/test_gpu_sdr_edges.py's
Guarded): every entry must be written, no guard element touched.

Edge                                                       case
---------------------------------------------------------  ---------------------------------------------------------------
n = 1, run of 8 images - 1, + 0, + 1, three runs           test_integer_cases[n = 1 | 7 | 8 | 9 | 17]
p, q in 1, 15, 16, 17, 90, 255, 256                        test_integer_cases (INT_CASES, columns 2 and 3)
p0, q0 in 1, 16, 17, 49, 64; every register plan           test_integer_cases (columns 4 and 5; [9-130-47-40-33-65 | 2-47-192-33-5-7])
m = 2048 (64 x 32 on 64 x 64), r in 1, 64, 65, 256         test_integer_cases (column 6)
no G (rows of p0 q0 factors), no mean                      test_integer_cases[9-64-64-64-32-2048 | 7-90-90-25-25-625 | 8-17-16-..]
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, sdr  # noqa: E402
from test_gpu_sdr_edges import Guarded, P, assert_equal, on, stream  # noqa: E402
from test_sdr_denoise_cpu import (INT_CASES, OLD_KEYS, REAL_CASES, RUN, golden, int_case, real_case,  # noqa: E402
                                  reference_reconstruction)

U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def reconstruct_dev(dev, F, G, A, B, mean, p0, q0, images=None):
    """ra_sdr_reconstruct into guarded buffers: x^ [n][p][q], and resid [n] if images are given"""
    n, p, q = F.shape[0], A.shape[0], B.shape[0]
    out = Guarded(dev, (n, p, q))
    resid = Guarded(dev, (n,), torch.float64) if images is not None else None
    Fd, Gd, Ad, Bd, md, xd = (on(dev, M) for M in (F, G, A, B, mean, images))
    rc = api.load_library().ra_sdr_reconstruct(P(Fd), n, F.shape[1], P(Gd), p0, q0, P(Ad), p, P(Bd), q, P(md), P(xd), out.ptr,
                                               resid.ptr if resid else None, stream())
    assert rc == 0, api.load_library().ra_last_error()
    return (out.result(), resid.result()) if resid else out.result()


# ---- 1. integer cases

@pytest.mark.parametrize("case", INT_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_integer_cases(dev, case):
    n, p, q, p0, q0 = case[:5]
    F, G, A, B, mean, ref = int_case(*case)
    got = reconstruct_dev(dev, F, G, A, B, mean, p0, q0)
    assert_equal(got, ref.astype(np.float32))
    # with the images: the same x^, and the residual of integers is exact
    x = np.random.default_rng(n + p).integers(-3, 4, (n, p, q)).astype(np.float32)
    got2, resid = reconstruct_dev(dev, F, G, A, B, mean, p0, q0, x)
    assert_equal(got2, got)
    assert_equal(resid, ((x.astype(np.float64) - ref) ** 2).sum(axis=(1, 2)))


# ---- 2. real-valued cases

@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_real_cases_within_bound(dev, case):
    p0, q0 = case[3:5]
    F, G, A, B, mean, ref, bound = real_case(*case)
    err = np.abs(reconstruct_dev(dev, F, G, A, B, mean, p0, q0).astype(np.float64) - ref)
    print("RATIO reconstruct %s %.4f (max error %.3e)" % (case[:6], float(np.max(err / bound)), float(err.max())))
    assert np.all(err <= bound), np.argwhere(err > bound)[:10].tolist()


# ---- 3. residuals

def residual_case(n=21, seed=80):
    case = (n, 33, 47, 5, 4, 7, True, seed)
    F, G, A, B, mean, ref, _ = real_case(*case)
    x = (ref + 0.3 * np.random.default_rng(seed).standard_normal(ref.shape)).astype(np.float32)
    return F, G, A, B, mean, x


def test_residual_is_the_double_sum_over_the_written_pixels(dev):
    F, G, A, B, mean, x = residual_case()
    xh, resid = reconstruct_dev(dev, F, G, A, B, mean, 5, 4, x)
    want = ((x.astype(np.float64) - xh.astype(np.float64)) ** 2).sum(axis=(1, 2))
    print("RATIO resid %.4f" % float(np.max(np.abs(resid - want) / ((33 * 47 + 8) * U53 * want))))
    assert np.all(np.abs(resid - want) <= (33 * 47 + 8) * U53 * want)


def test_a_nan_stays_in_its_own_image(dev):
    F, G, A, B, mean, x = residual_case()
    xh, resid = reconstruct_dev(dev, F, G, A, B, mean, 5, 4, x)
    Fn, xn = F.copy(), x.copy()
    Fn[3, 2], xn[12, 5, 6] = np.nan, np.nan                  # a factor of image 3 (run 0), a pixel of image 12 (run 1)
    xh2, resid2 = reconstruct_dev(dev, Fn, G, A, B, mean, 5, 4, xn)
    others = np.setdiff1d(np.arange(F.shape[0]), [3, 12])
    assert np.all(np.isnan(xh2[3])) and np.isnan(resid2[3]) and np.isnan(resid2[12])
    assert_equal(xh2[12], xh[12])
    assert_equal(xh2[others], xh[others])
    assert_equal(resid2[others], resid[others])
    # through the Python layer: the pixel spoils its image's factors, hence its image, and nothing else
    model = sdr.SdrModel(mean, A, B, G)
    clean, rc = sdr.denoise(on(dev, x), model, residuals=True)
    dirty, rd = sdr.denoise(on(dev, xn), model, residuals=True)
    clean, dirty, rc, rd = (t.cpu().numpy() for t in (clean, dirty, rc, rd))
    keep = np.setdiff1d(np.arange(F.shape[0]), [12])
    assert np.all(np.isnan(dirty[12])) and np.isnan(rd[12])
    assert_equal(dirty[keep], clean[keep])
    assert_equal(rd[keep], rc[keep])


# ---- 4. bitwise properties

def test_same_bits_call_to_call_stream_to_stream_and_cut_to_cut(dev):
    F, G, A, B, mean, x = residual_case()
    model = sdr.SdrModel(mean, A, B, G)
    xd, Fd = on(dev, x), on(dev, F)
    a, ra = sdr.denoise(xd, model, residuals=True)
    b, rb = sdr.denoise(xd, model, residuals=True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c, rcc = sdr.denoise(xd, model, residuals=True)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(ra, rb) and torch.equal(ra, rcc)
    whole = sdr.reconstruct(Fd, model)
    for cut in (5, RUN + 1):
        parts = [sdr.reconstruct(Fd[:cut].contiguous(), model), sdr.reconstruct(Fd[cut:].contiguous(), model)]
        assert torch.equal(torch.cat(parts), whole), cut
        pieces = [sdr.denoise(xd[s].contiguous(), model, residuals=True) for s in (slice(0, cut), slice(cut, None))]
        assert torch.equal(torch.cat([p[0] for p in pieces]), a) and torch.equal(torch.cat([p[1] for p in pieces]), ra), cut
    out = torch.full_like(xd, 7.0)
    assert sdr.denoise(xd, model, out=out) is out and torch.equal(out, a)
    assert torch.equal(sdr.reconstruct(Fd, model, add_mean=False), sdr.reconstruct(Fd, sdr.SdrModel(0 * mean, A, B, G)))
    E = sdr.eigenimages(model, 3)
    assert E.shape == (3, 33, 47) and torch.equal(E, sdr.reconstruct(torch.eye(3, 7, device=dev), model, add_mean=False))


@pytest.mark.parametrize("two_stage", [True, False])
def test_transform_gives_the_fit_s_own_factors(dev, two_stage):
    c = golden(2)
    x = on(dev, c["arr"])
    res = sdr.two_sdr(x, int(c["p0"]), int(c["q0"]), int(c["r"])) if two_stage else sdr.mpca(x, int(c["p0"]), int(c["q0"]))
    f = sdr.transform(x, sdr.SdrModel.from_result(res))
    assert f.is_cuda and f.dtype == torch.float32
    assert_equal(f.cpu().numpy(), res.factors)


# ---- 5. end to end

@pytest.mark.parametrize("two_stage", [True, False])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_device_denoise_matches_the_reference_reconstruction(dev, k, two_stage):
    c = golden(k)
    x = on(dev, c["arr"])
    p0, q0, r = int(c["p0"]), int(c["q0"]), int(c["r"])
    model = sdr.SdrModel.from_result(sdr.two_sdr(x, p0, q0, r) if two_stage else sdr.mpca(x, p0, q0))
    got = sdr.denoise(x, model).cpu().numpy().astype(np.float64)
    scale = np.abs(c["arr"] - model.mean).max()
    err = np.abs(got - reference_reconstruction(c, two_stage)).max() / scale
    print("case %d %s: max |x^ - reference| / scale = %.2e" % (k, "2SDR" if two_stage else "MPCA", err))
    assert err < 1e-4


def test_tool(dev, tmp_path, capsys):
    arr = golden(0)["arr"][:30]
    T = lambda name: str(tmp_path / name)
    np.save(T("s.npy"), arr)
    fit = [T("s.npy"), T("fit.npz"), "--p0", "3", "--q0", "4", "--r", "5"]
    assert sdr.main(fit) == 0
    z = dict(np.load(T("fit.npz")))
    assert set(z) == OLD_KEYS
    assert sdr.main([T("s.npy"), T("fit2.npz"), "--p0", "3", "--q0", "4", "--r", "5", "--denoised", T("d.npy"), "--residuals",
                     "--eigenimages", T("e.mrcs"), "--n_eig", "2"]) == 0
    z2 = dict(np.load(T("fit2.npz")))
    assert set(z2) == OLD_KEYS | {"resid", "resid_rel"} and all(np.array_equal(z[k], z2[k]) for k in OLD_KEYS)
    assert z2["resid"].shape == z2["resid_rel"].shape == (30,) and z2["resid"].dtype == np.float64
    assert np.all(z2["resid_rel"] >= 0) and np.all(z2["resid_rel"] < 1)
    d = np.load(T("d.npy"))
    assert d.shape == arr.shape and d.dtype == np.float32 and np.all(np.isfinite(d))
    from cryo_ralib_amd import stackio
    assert stackio.read_stack(T("e.mrcs")).shape == (2, 20, 24)
    # a stored model, the stack read 7 images at a time: bit for bit one unbatched call
    assert sdr.main([T("s.npy"), T("app.npz"), "--model", T("fit.npz"), "--batch", "7", "--denoised", T("d7.npy"), "--residuals"]) == 0
    assert sdr.main([T("s.npy"), T("app1.npz"), "--model", T("fit.npz"), "--denoised", T("d1.npy"), "--residuals"]) == 0
    a7, a1 = dict(np.load(T("app.npz"))), dict(np.load(T("app1.npz")))
    assert set(a7) == (OLD_KEYS - {"iterations", "energies"}) | {"resid", "resid_rel"}
    assert all(np.array_equal(a7[k], a1[k]) for k in a7) and np.array_equal(np.load(T("d7.npy")), np.load(T("d1.npy")))
    assert np.array_equal(a7["factors"], z["factors"]) and np.array_equal(np.load(T("d7.npy")), d)
    assert np.array_equal(a7["resid"], z2["resid"]) and all(np.array_equal(a7[k], z[k]) for k in ("G", "A", "B", "mean", "p0", "q0", "r"))
    # MPCA: a G of zero columns comes back as a model without G
    assert sdr.main([T("s.npy"), T("mp.npz"), "--p0", "3", "--q0", "4", "--mpca"]) == 0
    assert sdr.main([T("s.npy"), T("mpa.npz"), "--model", T("mp.npz"), "--eigenimages", T("em.npy")]) == 0
    assert np.array_equal(np.load(T("mpa.npz"))["factors"], np.load(T("mp.npz"))["factors"]) and np.load(T("em.npy")).shape == (12, 20, 24)
    capsys.readouterr()


# ---- 6. domain

def test_domain(dev):
    L, s = api.load_library(), stream()
    F, G, A, B, mean, ref = int_case(17, 20, 24, 3, 4, 5, True, True)
    Fd, Gd, Ad, Bd, md = (on(dev, M) for M in (F, G, A, B, mean))
    out = Guarded(dev, (17, 20, 24))
    res = Guarded(dev, (17,), torch.float64)
    x = on(dev, ref)

    def call(n=17, r=5, G=Gd, p0=3, q0=4, p=20, q=24, F=Fd, A=Ad, B=Bd, images=None, resid=None, o=out.ptr):
        return L.ra_sdr_reconstruct(P(F), n, r, P(G), p0, q0, P(A), p, P(B), q, P(md), P(images), o, resid, s)
    bad = [call(n=-1), call(p=0), call(p=257), call(q=0), call(q=257), call(p0=0), call(p0=21), call(q0=0), call(q0=25),
           call(p=256, q=256, p0=64, q0=33), call(p=256, q=256, p0=65, q0=4), call(r=0), call(r=13), call(r=257, p=90, q=90, p0=25, q0=25),
           call(G=None), call(G=None, r=11), call(F=None), call(A=None), call(B=None), call(o=None), call(images=x), call(resid=res.ptr)]
    assert bad == [-1] * len(bad), bad
    assert b"ra_sdr_reconstruct" in L.ra_last_error()
    assert call(n=0) == 0 and call(n=0, F=None, o=None) == 0
    torch.cuda.synchronize()
    for b in (out.buf.cpu().numpy(), res.buf.cpu().numpy()):
        assert np.all(b == b[0]), "a refused or empty call wrote"
    assert call(G=None, r=12, F=on(dev, np.zeros((17, 12)))) == 0 and call(images=x, resid=res.ptr) == 0
    out.result(), res.result()
    # the Python layer refuses before a launch
    model = sdr.SdrModel(mean, A, B, G)
    for f in (lambda: sdr.reconstruct(Fd[:, :4].contiguous(), model), lambda: sdr.reconstruct(F, model), lambda: sdr.reconstruct(Fd.double(), model),
              lambda: sdr.transform(x[:, :, :23].contiguous(), model), lambda: sdr.denoise(x[:, :, :23], model),
              lambda: sdr.denoise(x, model, out=x[:5]), lambda: sdr.denoise(x, model, out=x.cpu())):
        with pytest.raises(sdr.SdrError):
            f()
    assert sdr.reconstruct(Fd[:0], model).shape == (0, 20, 24) and sdr.transform(x[:0], model).shape == (0, 5)
    e, r0 = sdr.denoise(x[:0], model, residuals=True)
    assert e.shape == (0, 20, 24) and r0.shape == (0,) and r0.dtype == torch.float64
