"""k-means on the device: every fixture case against scikit-learn 1.7's values (tests/golden/kmeans_ref.npz) and the numpy
backend, the assignment against float64 brute force with exact ties and near-ties the f32 screen cannot separate, one large Lloyd
step against a float64 torch restatement, bitwise reproducibility, the domain errors, the tool, and the bootstrap of a reference
stack (aligned stack -> 2SDR -> k-means -> class averages -> one multi-reference pass)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, kmeans  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_ref.npz")
CASES = ["a1", "a2", "ar", "b", "e", "u", "o"]


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


def case(z, c):
    X = z["X_" + str(z["xkey_" + c])]
    init = str(z["init_" + c])
    kw = dict(n_init=int(z["n_init_" + c]))
    if init == "array":
        kw["init"] = z["init_array_" + c]
    else:
        kw["init"], kw["random_state"] = init, int(z["seed_" + c])
    return X, int(z["k_" + c]), kw


@pytest.mark.parametrize("c", CASES)
def test_device_matches_sklearn_and_numpy(dev, z, c):
    X, k, kw = case(z, c)
    with _maybe_warns(len(np.unique(z["labels_" + c])) < k):
        r = kmeans.kmeans(torch.from_numpy(X).to(dev), k, **kw)
    rn = kmeans.kmeans(X, k, backend="numpy", **kw)
    assert r.labels.dtype == np.int32 and r.centers.dtype == np.float64
    for ref_labels, ref_iter, ref_idx in ((z["labels_" + c].astype(np.int32), int(z["n_iter_" + c]), z["init_indices_" + c]),
                                          (rn.labels, rn.n_iter, rn.init_indices)):
        assert np.array_equal(r.labels, ref_labels), c
        assert r.n_iter == ref_iter, (c, r.n_iter, ref_iter)
        if ref_idx is not None and np.size(ref_idx):
            assert np.array_equal(r.init_indices, ref_idx), (c, r.init_indices, ref_idx)
    C = z["centers_" + c]
    assert np.abs(r.centers - C).max() <= 1e-6 * np.abs(C).max()
    assert abs(r.inertia - float(z["inertia_" + c])) <= 1e-9 * float(z["inertia_" + c]) + 1e-12


class _maybe_warns:
    def __init__(self, expect):
        self.expect = expect

    def __enter__(self):
        import warnings
        self.cm = warnings.catch_warnings(record=True)
        self.w = self.cm.__enter__()
        warnings.simplefilter("always")

    def __exit__(self, *a):
        self.cm.__exit__(*a)
        got = any(issubclass(x.category, kmeans.ConvergenceWarning) for x in self.w)
        assert got == self.expect


def brute_labels(X, C):
    D = ((X.astype(np.float64)[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    return np.argmin(D, axis=1).astype(np.int32), D


@pytest.mark.parametrize("d,k", [(3, 5), (16, 20), (64, 40), (200, 256)])
def test_assignment_exact_ties_lowest_index(dev, d, k):
    rng = np.random.default_rng(d + k)
    n = 3000
    C = 2.0 * rng.integers(-10, 11, (k, d))
    X = rng.integers(-20, 21, (n, d)).astype(np.float32)
    # exact ties: with even coordinates the midpoint of two centres is an integer point equidistant from both
    for i in range(0, 600):
        a, b = rng.choice(k, 2, replace=False)
        X[i] = ((C[a] + C[b]) / 2).astype(np.float32)
    lab, D = brute_labels(X, C)
    ties = np.sum(D == D.min(1, keepdims=True), axis=1) > 1
    assert ties.sum() >= 100
    got, inertia = kmeans.labels_for(torch.from_numpy(X).to(dev), C)
    assert np.array_equal(got, lab)
    assert inertia == float(np.sum(D.min(1)))                        # integers: every distance and the sum exact
    r = kmeans.kmeans(torch.from_numpy(X).to(dev), k, init=C, max_iter=1)
    rn = kmeans.kmeans(X, k, init=C, max_iter=1, backend="numpy")
    assert np.array_equal(r.labels, rn.labels) and r.n_iter == rn.n_iter == 1


@pytest.mark.parametrize("d", [16, 128])
def test_assignment_near_ties_beyond_the_f32_screen(dev, d):
    # pairs of centres one unit apart in feature 0, at coordinates ~2e4: |x|^2 ~ 1e8 d, where float32 resolves squared distances
    # to ~10 d, and the points sit within a few units of a pair, so the two distances differ by an odd integer of a few units.
    # Only the double re-evaluation separates them (integers: exact in double).
    rng = np.random.default_rng(d)
    n, k = 4096, 32
    base = rng.integers(-20000, 20001, (k // 2, d)).astype(np.float64)
    C = np.repeat(base, 2, axis=0)
    C[1::2, 0] += 1.0
    X = (base[rng.integers(0, k // 2, n)] + rng.integers(-3, 4, (n, d))).astype(np.float32)
    lab, D = brute_labels(X, C)
    srt = np.sort(D, axis=1)
    assert np.all(srt[:, 1] - srt[:, 0] <= 7) and np.all(srt[:, 0] <= 9 * d)
    assert np.sum(lab % 2 == 1) > n // 4                          # both members of a pair win
    got, inertia = kmeans.labels_for(torch.from_numpy(X).to(dev), C)
    assert np.array_equal(got, lab)
    assert inertia == float(np.sum(D.min(1)))


def test_large_step_matches_float64_torch(dev):
    n, d, k = 262144, 64, 64
    g = torch.Generator(device="cpu").manual_seed(5)
    cent = torch.randn(k, d, generator=g, dtype=torch.float64) * 3.0
    lab0 = torch.randint(0, k, (n,), generator=g)
    X = (cent[lab0] + torch.randn(n, d, generator=g, dtype=torch.float64)).float()
    C0 = X[torch.randperm(n, generator=g)[:k]].double()
    Xd = X.to(dev)
    r = kmeans.kmeans(Xd, k, init=C0.numpy(), max_iter=1)
    # the restatement: float64 distances, argmin, member means (torch on the device)
    X64, C64 = Xd.double(), C0.to(dev)
    Dm = torch.cdist(X64, C64) ** 2
    ref = Dm.argmin(1)
    srt = Dm.topk(2, dim=1, largest=False).values
    near = (srt[:, 1] - srt[:, 0]) <= 1e-9 * srt[:, 1]
    # one iteration without strict convergence: sklearn re-assigns with the new centres; the restatement does the same
    cnt = torch.bincount(ref, minlength=k).double()
    assert bool((cnt > 0).all())
    C1 = torch.zeros(k, d, dtype=torch.float64, device=dev).index_add_(0, ref, X64) / cnt[:, None]
    D1 = torch.cdist(X64, C1) ** 2
    ref1 = D1.argmin(1).cpu().numpy()
    assert np.abs(r.centers - C1.cpu().numpy()).max() <= 1e-10 * np.abs(C1.cpu().numpy()).max()
    s1 = D1.topk(2, dim=1, largest=False).values
    near1 = ((s1[:, 1] - s1[:, 0]) <= 1e-9 * s1[:, 1]).cpu().numpy()
    bad = r.labels != ref1
    assert not np.any(bad & ~near1), int(np.sum(bad & ~near1))
    assert int(near.sum()) < n // 100
    assert abs(r.inertia - float(D1.min(1).values.sum())) <= 1e-9 * r.inertia


def test_bitwise_reproducible_across_calls_and_streams(dev, z):
    rng = np.random.default_rng(8)
    X = torch.from_numpy((rng.normal(size=(50000, 50)) + rng.integers(0, 12, 50000)[:, None] * 3.0).astype(np.float32)).to(dev)
    a = kmeans.kmeans(X, 12, random_state=4)
    b = kmeans.kmeans(X, 12, random_state=4)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        c = kmeans.kmeans(X, 12, random_state=4)
    s.synchronize()
    for r in (b, c):
        assert np.array_equal(a.labels, r.labels) and np.array_equal(a.centers, r.centers)
        assert a.inertia == r.inertia and a.n_iter == r.n_iter and np.array_equal(a.init_indices, r.init_indices)


def test_domain_errors_return_codes(dev):
    L = api.load_library()
    x = torch.zeros((8, 4), device=dev)
    nrm = torch.full((8,), 7.0, device=dev)
    c = torch.zeros((2, 4), dtype=torch.float64, device=dev)
    c2 = torch.full((2, 4), 7.0, dtype=torch.float64, device=dev)
    lab = torch.full((8,), 7, dtype=torch.int32, device=dev)
    st = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    w = torch.ones(8, dtype=torch.float64, device=dev)
    v = torch.ones(2, dtype=torch.float64, device=dev)
    idx = torch.full((20,), 7, dtype=torch.int32, device=dev)
    clo = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
    out = torch.full((20,), 7.0, dtype=torch.float64, device=dev)
    s = stream()
    bad = [L.ra_kmeans_sqnorm(P(x), 0, 4, P(nrm), s), L.ra_kmeans_sqnorm(P(x), 8, 2049, P(nrm), s),
           L.ra_kmeans_sqnorm(P(x), 4194305, 4, P(nrm), s), L.ra_kmeans_sqnorm(None, 8, 4, P(nrm), s),
           L.ra_kmeans_labels(P(x), 8, 4, None, P(c), 0, P(lab), 1, P(st), s),
           L.ra_kmeans_labels(P(x), 8, 4, None, P(c), 9, P(lab), 1, P(st), s),
           L.ra_kmeans_labels(P(x), 300, 4, None, P(c), 257, P(lab), 1, P(st), s),
           L.ra_kmeans_labels(P(x), 8, 0, None, P(c), 2, P(lab), 1, P(st), s),
           L.ra_kmeans_labels(P(x), 8, 4, None, P(c), 2, P(lab), 0, None, s),
           L.ra_kmeans_lloyd(P(x), 8, 4, None, P(c), 2, P(c), P(lab), P(st), s),
           L.ra_kmeans_lloyd(P(x), 8, 4, None, P(c), 2, P(c2), P(lab), None, s),
           L.ra_kmeans_lloyd(P(x), 8, 4, None, P(c), 0, P(c2), P(lab), P(st), s),
           L.ra_kmeans_lloyd(P(x), 8, 2049, None, P(c), 2, P(c2), P(lab), P(st), s),
           L.ra_kmeans_search(P(w), 0, P(v), 2, P(idx), s), L.ra_kmeans_search(P(w), 8, P(v), 0, P(idx), s),
           L.ra_kmeans_search(P(w), 8, P(v), 17, P(idx), s), L.ra_kmeans_search(P(w), 8, None, 2, P(idx), s),
           L.ra_kmeans_seed(P(x), 8, 4, P(idx), 0, P(clo), 0, P(out), s), L.ra_kmeans_seed(P(x), 8, 4, P(idx), 17, P(clo), 0, P(out), s),
           L.ra_kmeans_seed(P(x), 8, 4, P(idx), 2, P(clo), 1, P(out), s), L.ra_kmeans_seed(P(x), 0, 4, P(idx), 1, P(clo), 1, P(out), s),
           L.ra_kmeans_seed(P(x), 8, 4, P(idx), 1, None, 1, P(out), s)]
    assert all(rc == -1 for rc in bad), bad
    torch.cuda.synchronize()
    assert torch.all(nrm == 7.0) and torch.all(lab == 7) and torch.all(st == 7.0) and torch.all(c2 == 7.0)
    assert torch.all(idx == 7) and torch.all(clo == 7.0) and torch.all(out == 7.0)
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(torch.zeros((40, 3), device=dev, dtype=torch.float64), 2)
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(torch.zeros((3, 40), device=dev).t(), 2)
    for bad_v in (float("nan"), float("inf")):
        bx = torch.zeros((40, 3), device=dev)
        bx[5, 1] = bad_v
        with pytest.raises(kmeans.KMeansError):
            kmeans.kmeans(bx, 2)
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(torch.zeros((40, 3), device=dev), 41)


def aligned_stack(nref, n, nx, ou, sigma, xr=2):
    """a planted synth stack, its planted classes and the inverse of the planted parameters [n][4]"""
    from cryo_ralib_amd import geometry, synth
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, sigma, ou=ou)
    inv = np.array([geometry.inverse_transform2(float(a), float(sx), float(sy), int(m))
                    for a, sx, sy, m in zip(truth["ang"], truth["sx"], truth["sy"], truth["mir"])], np.float64)
    return refs, parts, np.asarray(truth["cls"]), inv


def test_tool_on_sdr_output_with_truth_and_averages(dev, tmp_path):
    from cryo_ralib_amd import cli, sdr
    nx, ou, nref, n = 32, 12, 3, 240
    refs, parts, cls, inv = aligned_stack(nref, n, nx, ou, 0.3)
    np.save(tmp_path / "stack.npy", parts)
    np.savetxt(tmp_path / "init.txt", inv)
    np.save(tmp_path / "truth.npy", cls.astype(np.int64))
    assert sdr.main([str(tmp_path / "stack.npy"), str(tmp_path / "f.npz"), "--p0", "8", "--q0", "8", "--r", "10",
                     "--params", str(tmp_path / "init.txt")]) == 0
    assert kmeans.main([str(tmp_path / "f.npz"), str(tmp_path / "o.npz"), "--k", "3", "--seed", "0", "--truth",
                        str(tmp_path / "truth.npy"), "--stack", str(tmp_path / "stack.npy"), "--params", str(tmp_path / "init.txt"),
                        "--ou", str(ou), "--averages", str(tmp_path / "avg.npy")]) == 0
    o = np.load(tmp_path / "o.npz")
    assert str(o["backend"]) == "device" and o["labels"].shape == (n,)
    assert float(o["purity"]) >= 0.95 and float(o["c_purity"]) >= 0.95 and int(o["contingency"].sum()) == n
    avg = np.load(tmp_path / "avg.npy")
    assert avg.shape == (3, nx, nx) and np.all(np.isfinite(avg))
    # the averages drop in as the multi-reference command line's refstack
    out = tmp_path / "mref"
    assert cli.main_mref([str(tmp_path / "stack.npy"), str(tmp_path / "avg.npy"), str(out), "--ou", str(ou), "--xr", "2",
                          "--yr", "2", "--maxit", "1", "--ext", "npy"]) == 0
    rows = np.loadtxt(out / "params.txt", ndmin=2)
    got = np.empty(n, np.int64)
    got[rows[:, 0].astype(np.int64)] = rows[:, 5].astype(np.int64)
    assert kmeans.purity_score(cls, got) >= 0.95


def test_bootstrap_references_from_an_aligned_stack(dev):
    from cryo_ralib_amd import mref, sdr
    # 48 pixels: at 32 (ou 12) twelve of these references are too alike at this noise for the true references themselves to
    # reach 0.95 in one pass
    nx, ou, nref, n = 48, 18, 12, 720
    refs, parts, cls, inv = aligned_stack(nref, n, nx, ou, 0.3)
    x = torch.from_numpy(parts).to(dev)
    with torch.cuda.device(dev):
        al = api.rot_shift2d(x, inv)
        F = sdr.two_sdr(al, 8, 8, 12).factors
    # ten k-means++ runs, the best kept (one run from seed 0 merges two classes, a local minimum the numpy backend finds too)
    r = kmeans.kmeans(torch.from_numpy(np.ascontiguousarray(F, np.float32)).to(dev), 12, n_init=10, random_state=0)
    assert kmeans.purity_score(cls, r.labels) >= 0.95 and kmeans.c_purity_score(cls, r.labels) >= 0.95
    avg = kmeans.class_averages(parts, inv, r.labels, 12, ou)
    assert avg.shape == (12, nx, nx) and np.all(np.isfinite(avg))
    a = mref.MrefAligner(parts, avg, ou, 2, 2)
    a.iterate()
    got = a.params()["ref_id"]
    a.close()
    assert kmeans.purity_score(cls, got) >= 0.95
