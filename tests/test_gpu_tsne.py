"""t-SNE on the device: ra_tsne_knn against float64 brute force, the affinities against scikit-learn 1.7's
(tests/golden/tsne_ref.npz) and the numpy backend, one step and a short run against the numpy backend, full runs against
sklearn's KL, n_iter and trustworthiness, bitwise reproducibility, degenerate input, the domain errors and the tool."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, sdr, tsne  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_ref.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def csr(z, c, p):
    return (z["indptr_%s_%d" % (c, p)].astype(np.int64), z["indices_%s_%d" % (c, p)].astype(np.int64),
            z["P_%s_%d" % (c, p)].astype(np.float64))


def clusters(n, d, seed, ncl=5):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 3.0, (ncl, d))
    return (c[rng.integers(0, ncl, n)] + rng.normal(size=(n, d))).astype(np.float32)


@pytest.mark.parametrize("n,d,k", [(4096, 50, 91), (3000, 625, 31), (257, 3, 256)])
def test_knn_matches_float64_brute_force(dev, n, d, k):
    X = clusters(n, d, n + d)
    idx, d2 = tsne.knn(torch.from_numpy(X).to(dev), k)
    Xd = X.astype(np.float64)
    nrm = (Xd * Xd).sum(1)
    D = nrm[:, None] + nrm[None, :] - 2.0 * Xd @ Xd.T
    np.fill_diagonal(D, np.inf)
    cand = np.argsort(D, axis=1, kind="stable")[:, :min(n - 1, k + 8)]
    bad = 0
    for i in range(n):
        c = cand[i]
        ex = ((Xd[i] - Xd[c]) ** 2).sum(1)
        o = np.lexsort((c, ex))
        ref_idx, ref_d = c[o][:k], ex[o]
        assert np.allclose(d2[i], np.sort(((Xd[i] - Xd[idx[i]]) ** 2).sum(1)), rtol=1e-12, atol=0)
        assert np.all(np.diff(d2[i]) >= 0)
        if not np.array_equal(idx[i], ref_idx):
            # only a near-tie at the cut may swap members
            assert k < len(ref_d) and abs(ref_d[k] - ref_d[k - 1]) <= 1e-6 * ref_d[k], i
            bad += 1
    assert bad <= n // 100


def test_affinities_match_sklearn_and_numpy(dev, z):
    for c in "ab":
        for p in (30, 5):
            ip, ix, Pv = tsne.affinities(torch.from_numpy(z["X_" + c]).to(dev), float(p))
            ri, rx, rP = csr(z, c, p)
            assert np.array_equal(ip, ri) and np.array_equal(ix, rx)
            assert np.abs(Pv - rP).max() <= 2e-5 * rP.max()          # sklearn's float32 kNN distances (see test_tsne_cpu)
    X = clusters(4096, 50, 1)
    ip, ix, Pv = tsne.affinities(torch.from_numpy(X).to(dev), 30.0)
    ni, nx_, nP = tsne.affinities(X, 30.0, backend="numpy")
    assert np.array_equal(ip, ni) and np.array_equal(ix, nx_)
    assert np.abs(Pv - nP).max() <= 1e-6 * nP.max()


@pytest.mark.parametrize("n,exag", [(800, 12.0), (800, 1.0), (1500, 12.0), (1500, 1.0)])
def test_one_step_matches_numpy(dev, z, n, exag):
    if n == 800:
        X, c = z["X_a"], csr(z, "a", 30)
        Y = z["state_a_early"].astype(np.float64)
    else:
        X = clusters(n, 20, 5)
        c = tsne.affinities(X, 30.0, backend="numpy")
        Y = np.random.default_rng(2).normal(size=(n, 2)) * 5.0
    Y = Y.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(n)
    upd = (rng.normal(size=(n, 2)) * 0.1).astype(np.float32).astype(np.float64)
    gains = rng.uniform(0.5, 2.0, (n, 2)).astype(np.float32).astype(np.float64)
    e_np, g_np = tsne.gradient(Y, c, exag, backend="numpy")
    with torch.cuda.device(dev):
        e_d, g_d = tsne.gradient(Y, c, exag)
        Yd, ud, gd, err_d, gn_d = tsne.step(Y, c, upd, gains, exag, 0.5, 200.0)
    gscale = np.linalg.norm(g_np, axis=1).max()
    assert np.abs(g_d - g_np).max() <= 1e-4 * gscale
    assert abs(e_d - e_np) <= 1e-5 * abs(e_np)
    Yn, un, gnn, err_n, gn_n = tsne.step(Y, c, upd, gains, exag, 0.5, 200.0, backend="numpy")
    sign_flip = np.sign(upd * g_np) != np.sign(upd * g_d)      # a gain may branch the other way where upd g is ~0
    ok = ~sign_flip
    assert np.abs(Yd - Yn)[ok].max() <= 1e-6 + 1e-4 * gscale * 200.0 * np.abs(gains).max() * 1.3
    assert abs(err_d - err_n) <= 1e-5 * abs(err_n)
    assert abs(gn_d - gn_n) <= 1e-3 * gn_n


def test_full_run_matches_sklearn(dev, z):
    X = torch.from_numpy(z["X_a"]).to(dev)
    r = tsne.tsne(X, init=z["init_a"])
    kl = float(z["kl_a"])
    assert abs(r.kl_divergence - kl) <= 0.02 * kl, (r.kl_divergence, kl)
    assert abs(r.n_iter - int(z["n_iter_a"])) <= tsne.N_ITER_CHECK
    assert tsne.trustworthiness(z["X_a"], r.embedding) >= float(z["trust_a"]) - 0.01
    assert r.embedding.dtype == np.float32 and len(r.errors) == (r.n_iter + 1) // 50
    r2 = tsne.tsne(X)                                                   # init="pca" on the device
    assert np.isfinite(r2.kl_divergence) and abs(r2.kl_divergence - kl) <= 0.05 * kl
    assert tsne.trustworthiness(z["X_a"], r2.embedding) >= float(z["trust_a"]) - 0.01
    Yd = tsne.initial_embedding(X, "pca")
    assert np.abs(Yd - z["init_a"]).max() <= 1e-3 * np.abs(z["init_a"]).max()


def test_short_run_matches_numpy(dev, z):
    # The early phase is chaotic: in float64 alone a 1e-7 relative nudge of this init grows to 1e-4 of the spread after 10
    # iterations and to 8 % after 50, so the device's float32 trajectory is held to the numpy one over 10 iterations.
    X, c = z["X_a"], csr(z, "a", 30)
    Y0 = z["init_a"]
    lr = tsne.resolve_learning_rate("auto", X.shape[0], 12.0)
    ns = tsne._NumpyState(Y0, c)
    ns.reset()
    with torch.cuda.device(dev):
        D = tsne._Device(dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        ds = tsne._DeviceState(D, torch.from_numpy(Y0).to(dev), i32(c[0]), i32(c[1]),
                               torch.from_numpy(c[2].astype(np.float32)).to(dev))
        ds.reset()
        for i in range(10):
            ns.step(12.0, 0.5, lr, False)
            ds.step(12.0, 0.5, lr, i == 9)
        Yd = ds.embedding()
    Yn = ns.embedding()
    spread = Yn.max(0) - Yn.min(0)
    assert np.abs(Yd - Yn).max() <= 1e-3 * spread.max()


def test_bitwise_reproducible_across_calls_and_streams(dev, z):
    X = torch.from_numpy(clusters(1500, 30, 9)).to(dev)
    a = tsne.tsne(X, max_iter=300, init="random", random_state=1)
    b = tsne.tsne(X, max_iter=300, init="random", random_state=1)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        c = tsne.tsne(X, max_iter=300, init="random", random_state=1)
    s.synchronize()
    for r in (b, c):
        assert np.array_equal(a.embedding, r.embedding)
        assert a.kl_divergence == r.kl_divergence and np.array_equal(a.errors, r.errors) and a.n_iter == r.n_iter
    i1, x1, p1 = tsne.affinities(X, 30.0)
    i2, x2, p2 = tsne.affinities(X, 30.0)
    assert np.array_equal(i1, i2) and np.array_equal(x1, x2) and np.array_equal(p1, p2)


def test_degenerate_input_stays_finite(dev):
    rng = np.random.default_rng(4)
    X = rng.normal(size=(600, 8)).astype(np.float32)
    X[300:] = X[:300]                     # every point twice
    X[100:200] = X[100]                   # a hundred identical points
    r = tsne.tsne(torch.from_numpy(X).to(dev), max_iter=300, init="random", random_state=0)
    assert np.all(np.isfinite(r.embedding)) and np.isfinite(r.kl_divergence)
    idx, d2 = tsne.knn(torch.from_numpy(X).to(dev), 20)
    assert np.all((idx >= 0) & (idx < 600)) and np.all(idx != np.arange(600)[:, None]) and np.all(d2 >= 0)
    Z = np.zeros((50, 3), np.float32)     # all points identical
    r = tsne.tsne(torch.from_numpy(Z).to(dev), perplexity=10.0, max_iter=250, init="random", random_state=0)
    assert np.all(np.isfinite(r.embedding))


def test_domain_errors_return_codes(dev):
    L = api.load_library()
    x = torch.zeros((8, 4), device=dev)
    idx = torch.full((8, 4), 7, dtype=torch.int32, device=dev)
    d2 = torch.full((8, 4), 7.0, dtype=torch.float64, device=dev)
    y = torch.full((8, 2), 7.0, device=dev)
    y2 = torch.full((8, 2), 7.0, device=dev)
    ip = torch.zeros(9, dtype=torch.int32, device=dev)
    st = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    s = stream()
    bad = [L.ra_tsne_knn(P(x), 1, 4, 1, P(idx), P(d2), s), L.ra_tsne_knn(P(x), 8, 0, 4, P(idx), P(d2), s),
           L.ra_tsne_knn(P(x), 8, 2049, 4, P(idx), P(d2), s), L.ra_tsne_knn(P(x), 8, 4, 8, P(idx), P(d2), s),
           L.ra_tsne_knn(P(x), 400, 4, 302, P(idx), P(d2), s), L.ra_tsne_knn(P(x), 262145, 4, 4, P(idx), P(d2), s),
           L.ra_tsne_affinity(P(d2), 8, 4, 0.0, P(d2), s), L.ra_tsne_affinity(P(d2), 8, 4, 101.0, P(d2), s),
           L.ra_tsne_affinity(P(d2), 8, 8, 3.0, P(d2), s),
           L.ra_tsne_step(P(y), P(y), P(y2), P(y2), 8, P(ip), None, None, 0, 12.0, 0.5, 50.0, P(st), s),
           L.ra_tsne_step(P(y), P(y2), P(y2), P(y2), 1, P(ip), None, None, 0, 12.0, 0.5, 50.0, P(st), s),
           L.ra_tsne_step(P(y), P(y2), P(y2), P(y2), 8, P(ip), None, None, -1, 12.0, 0.5, 50.0, P(st), s),
           L.ra_tsne_step(P(y), P(y2), P(y2), P(y2), 8, P(ip), None, None, 0, 12.0, 0.5, 0.0, P(st), s),
           L.ra_tsne_step(P(y), P(y2), P(y2), P(y2), 8, P(ip), None, None, 4, 12.0, 0.5, 50.0, P(st), s),
           L.ra_tsne_error(P(y), 8, P(ip), None, None, 0, 1.0, None, None, s),
           L.ra_tsne_error(P(y), 8, P(ip), None, None, 0, float("nan"), P(y2), P(st), s)]
    assert all(rc == -1 for rc in bad), bad
    torch.cuda.synchronize()
    assert torch.all(idx == 7) and torch.all(d2 == 7.0) and torch.all(y2 == 7.0) and torch.all(st == 7.0)
    with pytest.raises(tsne.TsneError):
        tsne.tsne(torch.zeros((40, 3), device=dev), perplexity=50.0)
    with pytest.raises(tsne.TsneError):
        tsne.tsne(torch.zeros((40, 3), device=dev, dtype=torch.float64))
    bad_x = torch.zeros((40, 3), device=dev)
    bad_x[5, 1] = float("inf")
    with pytest.raises(tsne.TsneError):
        tsne.tsne(bad_x)


def test_tool_on_sdr_output_of_aligned_synth_stack(dev, tmp_path):
    from cryo_ralib_amd import cli, synth
    nx, ou, nref, n = 32, 12, 3, 240
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, 2, 2, 0.3, ou=ou)
    np.save(tmp_path / "stack.npy", parts)
    np.save(tmp_path / "refs.npy", refs)
    out = tmp_path / "mref"
    assert cli.main_mref([str(tmp_path / "stack.npy"), str(tmp_path / "refs.npy"), str(out), "--ou", str(ou), "--xr", "2",
                          "--yr", "2", "--maxit", "1", "--ext", "npy"]) == 0
    assert sdr.main([str(tmp_path / "stack.npy"), str(tmp_path / "f.npz"), "--p0", "8", "--q0", "8", "--r", "10",
                     "--params", str(out / "params.txt")]) == 0
    assert tsne.main([str(tmp_path / "f.npz"), str(tmp_path / "e.npz"), "--seed", "0"]) == 0
    e = np.load(tmp_path / "e.npz")
    F = np.load(tmp_path / "f.npz")["factors"]
    Y = e["embedding"]
    assert Y.shape == (n, 2) and np.all(np.isfinite(Y)) and str(e["backend"]) == "device"
    assert tsne.trustworthiness(F, Y) >= 0.9
    # the classes stay apart: every point's nearest embedded neighbour is mostly of its own class
    cls = np.asarray(truth["cls"])
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    assert np.mean(cls[np.argmin(D, axis=1)] == cls) >= 0.9
