"""2SDR / MPCA on the device: every ra_sdr_* entry against float64 numpy, bitwise reproducibility and symmetry of the Grams,
ra_rot_shift2d against Engine.transform_accumulate, two_sdr / mpca against the reference's values (tests/golden/sdr_ref.npz)
and the numpy backend, the tool, and the domain errors."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, sdr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdr_ref.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def case(k):
    z = np.load(GOLDEN)
    return {key[:-len("_%d" % k)]: z[key] for key in z.files if key.endswith("_%d" % k)}


def stack(n, p, q, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, p, q)) + 0.3 * rng.standard_normal((1, p, q)) + 1.0).astype(np.float32)


def gram_dev(x, n, p, q, mean, form, Pm=None):
    d = p if form == 1 else q
    g = torch.empty((d, d), dtype=torch.float64, device=x.device)
    Pd = torch.from_numpy(np.ascontiguousarray(Pm, np.float32)).to(x.device) if Pm is not None else None
    rc = api.load_library().ra_sdr_gram(P(x), n, p, q, P(mean), form, P(Pd), 0 if Pm is None else Pm.shape[1], P(g), stream())
    assert rc == 0, api.load_library().ra_last_error()
    torch.cuda.synchronize()
    return g.cpu().numpy()


def gram_np(X, form, Pm=None):
    n, p, q = X.shape
    if form == 0:
        Z = X.reshape(n * p, q)
    elif form == 1:
        Z = np.einsum("irc,cj->ijr", X, Pm).reshape(-1, p)
    else:
        Z = np.einsum("rj,irc->ijc", Pm, X).reshape(-1, q)
    return Z.T @ Z


def mean_dev(x):
    n, p, q = x.shape
    m = torch.empty((p, q), dtype=torch.float32, device=x.device)
    assert api.load_library().ra_sdr_mean(P(x), n, p, q, P(m), stream()) == 0
    return m


SHAPES = [(90, 90), (33, 47), (130, 130), (256, 256)]


@pytest.mark.parametrize("p,q", SHAPES)
@pytest.mark.parametrize("n", [1, 77])
def test_mean_and_grams_match_float64(dev, p, q, n):
    if p * q > 130 * 130 and n > 1:
        n = 45                                                  # 256^2: n still not a multiple of any run length
    a = stack(n, p, q, p + q + n)
    x = torch.from_numpy(a).to(dev)
    m = mean_dev(x)
    mean = m.cpu().numpy()
    assert np.abs(mean - a.astype(np.float64).mean(0)).max() <= 1e-6 * (1 + np.abs(a).max())
    X = (a - mean).astype(np.float64)
    rng = np.random.default_rng(5)
    for form in (0, 1, 2):
        for k in ((None,) if form == 0 else (1, 25, 64)):
            side = q if form == 1 else p
            if k is not None and k > side:
                continue
            Pm = None if k is None else np.linalg.qr(rng.standard_normal((side, k)))[0].astype(np.float32)
            g = gram_dev(x, n, p, q, m, form, Pm)
            ref = gram_np(X, form, None if Pm is None else Pm.astype(np.float64))
            assert np.abs(g - ref).max() <= 1e-5 * np.linalg.norm(ref), (form, k)
            assert np.array_equal(g, g.T)


def test_second_stage_gram_and_factors(dev):
    n, m, r = 1003, 625, 50
    rng = np.random.default_rng(9)
    u = rng.standard_normal((n, m)).astype(np.float32)
    U = torch.from_numpy(u).to(dev)
    g = gram_dev(U, n, 1, m, None, 0)
    ref = u.astype(np.float64).T @ u.astype(np.float64)
    assert np.abs(g - ref).max() <= 1e-5 * np.linalg.norm(ref)
    assert np.array_equal(g, g.T)
    G = np.linalg.qr(rng.standard_normal((m, r)))[0].astype(np.float32)
    Gd = torch.from_numpy(G).to(dev)
    F = torch.empty((n, r), dtype=torch.float32, device=dev)
    assert api.load_library().ra_sdr_factors(P(U), n, m, P(Gd), r, P(F), stream()) == 0
    Fr = u.astype(np.float64) @ G.astype(np.float64)
    assert np.abs(F.cpu().numpy() - Fr).max() <= 1e-5 * np.abs(Fr).max()


@pytest.mark.parametrize("p,q,p0,q0", [(90, 90, 25, 25), (33, 47, 7, 40), (130, 130, 64, 32), (256, 256, 40, 40), (20, 24, 1, 1)])
def test_project_matches_float64(dev, p, q, p0, q0):
    n = 37
    a = stack(n, p, q, 3)
    x = torch.from_numpy(a).to(dev)
    m = mean_dev(x)
    rng = np.random.default_rng(1)
    A = np.linalg.qr(rng.standard_normal((p, p0)))[0].astype(np.float32)
    B = np.linalg.qr(rng.standard_normal((q, q0)))[0].astype(np.float32)
    U = torch.empty((n, p0 * q0), dtype=torch.float32, device=dev)
    Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    rc = api.load_library().ra_sdr_project(P(x), n, p, q, P(m), P(Ad), p0, P(Bd), q0, P(U), stream())
    assert rc == 0
    X = (a - m.cpu().numpy()).astype(np.float64)
    ref = np.einsum("ra,irc,cb->iab", A.astype(np.float64), X, B.astype(np.float64)).reshape(n, -1)
    assert np.abs(U.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_grams_bitwise_reproducible_across_calls_and_streams(dev):
    p = q = 90
    n = 300
    x = torch.from_numpy(stack(n, p, q, 21)).to(dev)
    m = mean_dev(x)
    B = np.linalg.qr(np.random.default_rng(2).standard_normal((q, 25)))[0].astype(np.float32)
    g1 = gram_dev(x, n, p, q, m, 1, B)
    g2 = gram_dev(x, n, p, q, m, 1, B)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        g3 = gram_dev(x, n, p, q, m, 1, B)
    assert np.array_equal(g1, g2) and np.array_equal(g1, g3)
    h1, h2 = gram_dev(x, n, p, q, m, 0), gram_dev(x, n, p, q, m, 0)
    assert np.array_equal(h1, h2) and np.array_equal(h1, h1.T)
    m2 = mean_dev(x)
    assert torch.equal(m, m2)


@pytest.mark.parametrize("nx", [32, 90])
def test_rot_shift2d_equals_engine_transform(dev, nx):
    n = 40
    rng = np.random.default_rng(nx)
    a = rng.standard_normal((n, nx, nx)).astype(np.float32)
    x = torch.from_numpy(a).to(dev)
    prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.integers(0, 2, n)])
    out = api.rot_shift2d(x, prm)
    eng = api.Engine(nx, min(nx // 2 - 5, 30), 2, 2, 1.0, 1, api.RA_MODE_MREF, device=0)
    rec = np.zeros(n, api.RESULT_DTYPE)
    rec["alpha"], rec["sx"], rec["sy"], rec["mirror"] = prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3]
    res = torch.from_numpy(rec.view(np.int32).reshape(n, 8)).to(dev)
    al = torch.empty_like(x)
    eng.transform_accumulate(x, res, 0, al)
    eng.sync()
    eng.close()
    torch.cuda.synchronize()
    assert torch.equal(out, al)
    from cryo_ralib_amd import synth
    for i in (0, 7):
        ref = synth.rot_shift2d_np(a[i], prm[i, 0], prm[i, 1], prm[i, 2], int(prm[i, 3]))
        assert np.abs(out[i].cpu().numpy() - ref).max() < 1e-4


@pytest.mark.parametrize("k", [0, 2])
def test_device_two_sdr_and_mpca_match_reference(dev, k):
    c = case(k)
    x = torch.from_numpy(c["arr"]).to(dev)
    p0, q0, r = int(c["p0"]), int(c["q0"]), int(c["r"])
    res = sdr.two_sdr(x, p0, q0, r)
    proj = lambda M: M @ M.T
    assert np.abs(proj(res.A) - proj(c["A"])).max() < 1e-4
    assert np.abs(proj(res.B) - proj(c["B"])).max() < 1e-4
    assert np.abs(res.mean.ravel() - c["mean"].ravel()).max() < 1e-6
    d = np.kron(np.sign((res.A * c["A"]).sum(0)), np.sign((res.B * c["B"]).sum(0)))
    assert np.abs(proj(res.G * d[:, None]) - proj(c["G"])).max() < 1e-4
    for F, Fr in ((res.factors, c["factors"]), (sdr.mpca(x, p0, q0).factors, c["mfactors"])):
        s = np.sign((F * Fr).sum(0))
        assert (np.abs(F * s - Fr).max(0) / np.linalg.norm(Fr, axis=0)).max() < 1e-3


def test_device_noise_dominated_energy(dev):
    c = case(1)
    x = torch.from_numpy(c["arr"]).to(dev)
    res = sdr.two_sdr(x, 8, 6, 10)
    X = c["arr"].astype(np.float64) - c["arr"].astype(np.float64).mean(0)
    E = lambda A, B: float((np.einsum("ra,irc,cb->iab", A, X, B) ** 2).sum())
    assert abs(E(res.A, res.B) - E(c["A"], c["B"])) / E(c["A"], c["B"]) < 1e-4


@pytest.mark.parametrize("k", [0, 1, 2])
def test_device_matches_numpy_backend(dev, k):
    c = case(k)
    p0, q0, r = int(c["p0"]), int(c["q0"]), int(c["r"])
    # the iteration count is forced on both: a stop at tol = 1e-7 compares energy steps far below the f32 rounding of E
    it, tol = 6, -np.inf
    d = sdr.two_sdr(torch.from_numpy(c["arr"]).to(dev), p0, q0, r, max_iter=it, tol=tol)
    h = sdr.two_sdr(c["arr"], p0, q0, r, max_iter=it, tol=tol, backend="numpy")
    assert d.iterations == h.iterations
    assert np.array_equal(d.mean, h.mean) or np.abs(d.mean - h.mean).max() < 1e-6
    for M, N in ((d.A, h.A), (d.B, h.B), (d.G, h.G)):
        assert np.abs(M @ M.T - N @ N.T).max() < 2e-5


def test_tool_matches_api_on_aligned_synth_stack(dev, tmp_path):
    from cryo_ralib_amd import cli, synth
    nx, ou, nref, n = 32, 12, 3, 48
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, 2, 2, 0.3, ou=ou)
    np.save(tmp_path / "stack.npy", parts)
    np.save(tmp_path / "refs.npy", refs)
    out = tmp_path / "mref"
    assert cli.main_mref([str(tmp_path / "stack.npy"), str(tmp_path / "refs.npy"), str(out), "--ou", str(ou), "--xr", "2",
                          "--yr", "2", "--maxit", "1", "--ext", "npy"]) == 0
    assert sdr.main([str(tmp_path / "stack.npy"), str(tmp_path / "o.npz"), "--p0", "5", "--q0", "5", "--r", "8",
                     "--params", str(out / "params.txt")]) == 0
    z = np.load(tmp_path / "o.npz")
    prm = sdr.read_params(str(out / "params.txt"), n)
    x = api.rot_shift2d(torch.from_numpy(parts).to(dev), prm)
    res = sdr.two_sdr(x, 5, 5, 8)
    assert np.array_equal(z["factors"], res.factors) and np.array_equal(z["G"], res.G)
    assert np.array_equal(z["A"], res.A) and np.array_equal(z["B"], res.B) and np.array_equal(z["mean"], res.mean)
    assert int(z["iterations"]) == res.iterations and (int(z["p0"]), int(z["q0"]), int(z["r"])) == (5, 5, 8)
    bad = tmp_path / "short.txt"
    bad.write_text("\n".join(open(out / "params.txt").read().splitlines()[:-1]) + "\n")
    with pytest.raises(SystemExit):
        sdr.main([str(tmp_path / "stack.npy"), str(tmp_path / "o2.npz"), "--p0", "5", "--q0", "5", "--r", "8", "--params", str(bad)])


def test_domain_errors_return_codes(dev):
    L = api.load_library()
    x = torch.zeros((4, 8, 8), device=dev)
    m = torch.zeros((8, 8), device=dev)
    g = torch.full((8, 8), 7.0, dtype=torch.float64, device=dev)
    Pm = torch.zeros((8, 2), device=dev)
    U = torch.full((4, 4), 7.0, device=dev)
    s = stream()
    bad = [L.ra_sdr_mean(P(x), 4, 257, 8, P(m), s), L.ra_sdr_mean(P(x), 0, 8, 8, P(m), s),
           L.ra_sdr_gram(P(x), 4, 8, 8, P(m), 3, None, 0, P(g), s), L.ra_sdr_gram(P(x), 4, 8, 300, P(m), 0, None, 0, P(g), s),
           L.ra_sdr_gram(P(x), 4, 8, 8, P(m), 1, P(Pm), 0, P(g), s), L.ra_sdr_gram(P(x), 4, 8, 8, P(m), 1, P(Pm), 65, P(g), s),
           L.ra_sdr_gram(P(x), 4, 8, 8, P(m), 2, P(Pm), 9, P(g), s), L.ra_sdr_gram(P(x), 4, 8, 8, P(m), 1, None, 2, P(g), s),
           L.ra_sdr_project(P(x), 4, 8, 8, P(m), P(Pm), 9, P(Pm), 2, P(U), s),
           L.ra_sdr_project(P(x), 4, 8, 8, P(m), P(Pm), 0, P(Pm), 2, P(U), s),
           L.ra_sdr_project(P(x), 4, 80, 80, P(m), P(Pm), 64, P(Pm), 64, P(U), s),
           L.ra_sdr_factors(P(U), 4, 4, P(Pm), 5, P(U), s), L.ra_sdr_factors(P(U), 4, 2049, P(Pm), 2, P(U), s),
           L.ra_sdr_factors(P(U), 0, 4, P(Pm), 2, P(U), s), L.ra_rot_shift2d(P(x), 4, 1, P(U), P(x), s)]
    assert all(rc == -1 for rc in bad), bad
    torch.cuda.synchronize()
    assert torch.all(g == 7.0) and torch.all(U == 7.0)        # nothing was launched
    with pytest.raises(sdr.SdrError):
        sdr.two_sdr(torch.zeros((4, 8, 8), device=dev), 2, 2, 4)
    with pytest.raises(sdr.SdrError):
        sdr.two_sdr(torch.zeros((4, 8, 8), device=dev, dtype=torch.float64), 2, 2, 1)
