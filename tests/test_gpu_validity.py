"""Cluster validity on the device (ra_kmeans_silhouette, ra_kmeans_dispersion behind kmeans.silhouette_* / calinski_harabasz_score /
davies_bouldin_score / validity / sweep): every scikit-learn 1.7 pin of tests/golden/validity_ref.npz and the float64 numpy backend,
the shapes around the kernel's tiles, the nearest cluster, bitwise repeatability, the C entry points' rejections and the tool.

The bound on a sample's silhouette is 2 (d + 4) 2^-24: the f32 difference, square and d-term sum give a squared distance with a
relative error of at most (d + 2) 2^-24, the square root halves it and adds a rounding, the double sums add nothing at this scale,
and s is 1 - a ratio <= 1 of two such sums: (d + 4) 2^-24, doubled for the second-order terms.  The same relative bound holds for
the mean distances a and b themselves.  CH and DB are all-double: 1e-9 relative."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, kmeans  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validity_ref.npz")
CASES = "abosugdt"
TR = TC = 64        # the kernel's row and column tiles (csrc/ralign_validity.h)
FC = 32             # its feature chunk
PARENT_KEYS = {"labels", "centers", "inertia", "n_iter", "init_indices", "k", "init", "seed", "backend"}
SCORE_KEYS = {"silhouette", "class_silhouette", "silhouette_samples", "calinski_harabasz", "davies_bouldin"}


def bound(d):
    return 2.0 * (d + 4) * 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def case(z, c):
    return z["X_" + c], z["labels_" + c].astype(np.int64), int(z["k_" + c])


def check_against_numpy(X, lab, k, dev, what):
    """device s, a, b within the bound of the float64 backend; nearest where float64 separates the two smallest means"""
    d = X.shape[1]
    sv, a, b, near = kmeans.silhouette_samples(torch.from_numpy(X).to(dev), lab, k, details=True)
    rs, ra, rb, rnear = kmeans.silhouette_samples(X, lab, k, backend="numpy", details=True)
    assert sv.dtype == np.float64 and near.dtype == np.int32 and sv.shape == (len(X),)
    es = np.abs(sv - rs).max()
    ea = (np.abs(a - ra) / np.maximum(ra, 1e-300)).max()
    eb = (np.abs(b - rb) / rb).max()
    print("%s: n = %d, d = %d, k = %d: max |s - s64| = %.3g (bound %.3g), rel a %.3g, rel b %.3g" % (what, len(X), d, k, es, bound(d), ea, eb))
    assert es <= bound(d) and ea <= bound(d) and eb <= bound(d)
    # the float64 means of every other non-empty cluster, to see where the argmin is decided beyond the bound
    Xd = X.astype(np.float64)
    n = len(X)
    cnt = np.bincount(lab, minlength=k)
    H = np.zeros((n, k))
    H[np.arange(n), lab] = 1.0
    M = np.empty((n, k))
    ch = max(1, (1 << 22) // (n * d))
    for s0 in range(0, n, ch):
        M[s0:s0 + ch] = np.sqrt(((Xd[s0:s0 + ch, None, :] - Xd[None, :, :]) ** 2).sum(-1)) @ H
    with np.errstate(divide="ignore", invalid="ignore"):
        M = np.where(cnt[None, :] > 0, M / cnt[None, :], np.inf)
    M[np.arange(n), lab] = np.inf
    two = np.sort(M, axis=1)[:, :2]
    decided = ~np.isfinite(two[:, 1])
    decided[~decided] = (two[~decided, 1] - two[~decided, 0]) > bound(d) * two[~decided, 1]
    assert np.array_equal(near[decided], rnear[decided]) and decided.mean() > 0.9
    assert np.all(near != lab) and np.all(cnt[near] > 0)
    return sv, a, b, near


@pytest.mark.parametrize("c", CASES)
def test_device_matches_sklearn_and_numpy(dev, z, c):
    X, lab, k = case(z, c)
    sv, a, b, near = check_against_numpy(X, lab, k, dev, "pin " + c)
    d = X.shape[1]
    assert np.abs(sv - z["silhouette_samples_" + c]).max() <= bound(d)
    Xd = torch.from_numpy(X).to(dev)
    assert abs(kmeans.silhouette_score(Xd, lab, k) - float(z["silhouette_score_" + c])) <= bound(d)
    ch, db = kmeans.calinski_harabasz_score(Xd, lab, k), kmeans.davies_bouldin_score(Xd, lab, k)
    assert ch == pytest.approx(float(z["calinski_harabasz_score_" + c]), rel=1e-9)
    assert db == pytest.approx(float(z["davies_bouldin_score_" + c]), rel=1e-9)
    assert ch == pytest.approx(kmeans.calinski_harabasz_score(X, lab, k, backend="numpy"), rel=1e-9)
    assert db == pytest.approx(kmeans.davies_bouldin_score(X, lab, k, backend="numpy"), rel=1e-9)
    v = kmeans.validity(Xd, lab, k)
    cnt = np.bincount(lab, minlength=k)
    assert v.silhouette == sv.mean() and v.calinski_harabasz == ch and v.davies_bouldin == db and np.array_equal(v.counts, cnt)
    assert np.array_equal(np.isnan(v.class_silhouette), cnt == 0) and np.array_equal(v.samples, sv)
    for j in np.nonzero(cnt)[0]:
        assert v.class_silhouette[j] == pytest.approx(sv[lab == j].mean(), abs=1e-14)


def test_special_cases_value_for_value(dev, z):
    """what the unused-id, singleton, all-duplicates and n = 3 pins are there for, on the device"""
    X, lab, k = case(z, "u")
    sv, a, b, near = kmeans.silhouette_samples(torch.from_numpy(X).to(dev), lab, k, details=True)
    assert not np.any(near == 3) and np.isnan(kmeans.validity(torch.from_numpy(X).to(dev), lab, k).class_silhouette[3])
    X, lab, k = case(z, "g")
    sv, a, b, near = kmeans.silhouette_samples(torch.from_numpy(X).to(dev), lab, k, details=True)
    assert sv[0] == 0.0 and a[0] == 0.0 and b[0] > 0 and near[0] != 4
    X, lab, k = case(z, "d")
    sv, a, b, near = kmeans.silhouette_samples(torch.from_numpy(X).to(dev), lab, k, details=True)
    assert np.all(a[lab == 0] == 0.0) and np.all(sv[lab == 0] == 1.0)       # |x - x| = 0 exactly: no cancellation in the difference form
    X, lab, k = case(z, "t")
    sv = kmeans.silhouette_samples(torch.from_numpy(X).to(dev), lab, k)
    assert sv[2] == 0.0 and np.abs(sv - z["silhouette_samples_t"]).max() <= bound(2)
    # all points equal: every quotient is 0 / 0
    X0 = torch.ones((10, 3), device=dev)
    assert np.all(kmeans.silhouette_samples(X0, np.arange(10) % 2, 2) == 0.0)


def random_case(n, d, k, seed):
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])[rng.permutation(n)]      # every id present
    X = (rng.normal(size=(n, d)) + 2.0 * rng.normal(size=(k, d))[lab]).astype(np.float32)
    return X, lab.astype(np.int64)


@pytest.mark.parametrize("n,d,k", [(TR - 1, 5, 3), (TR, 5, 3), (TR + 1, 5, 3), (130, FC - 1, 3), (130, FC, 3), (130, FC + 1, 3),
                                   (130, 2 * FC + 1, 4), (130, 1, 3), (130, 2048, 3), (600, 4, 2), (600, 4, 256)])
def test_shapes_around_the_tiles(dev, n, d, k):
    X, lab = random_case(n, d, k, n + d + k)
    check_against_numpy(X, lab, k, dev, "shape")
    Xd = torch.from_numpy(X).to(dev)
    assert kmeans.calinski_harabasz_score(Xd, lab, k) == pytest.approx(kmeans.calinski_harabasz_score(X, lab, k, backend="numpy"), rel=1e-9)
    assert kmeans.davies_bouldin_score(Xd, lab, k) == pytest.approx(kmeans.davies_bouldin_score(X, lab, k, backend="numpy"), rel=1e-9)


def test_clusters_of_whole_column_tiles(dev):
    """clusters of exactly one and two column tiles get no padding; the third one is padded"""
    rng = np.random.default_rng(5)
    lab = np.concatenate([np.zeros(TC), np.ones(2 * TC), np.full(37, 2)]).astype(np.int64)[rng.permutation(3 * TC + 37)]
    X = (rng.normal(size=(len(lab), 7)) + 3.0 * lab[:, None]).astype(np.float32)
    check_against_numpy(X, lab, 3, dev, "whole tiles")


def test_bitwise_repeatable_and_permutation(dev):
    X, lab = random_case(1500, 50, 12, 3)
    Xd = torch.from_numpy(X).to(dev)
    r0 = kmeans.silhouette_samples(Xd, lab, 12, details=True)
    r1 = kmeans.silhouette_samples(Xd, lab, 12, details=True)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        r2 = kmeans.silhouette_samples(Xd, lab, 12, details=True)
        d2 = kmeans._dispersion(Xd, lab, 12, "device")
    s.synchronize()
    d0 = kmeans._dispersion(Xd, lab, 12, "device")
    for r in (r1, r2):
        assert all(np.array_equal(u, v) for u, v in zip(r0, r))
    assert all(np.array_equal(u, v) for u, v in zip(d0, d2))
    # rows permuted, labels alike: the permuted values, within the bound (the order of the sums follows the index order)
    perm = np.random.default_rng(4).permutation(len(X))
    rp = kmeans.silhouette_samples(torch.from_numpy(X[perm]).to(dev), lab[perm], 12, details=True)
    assert np.abs(rp[0] - r0[0][perm]).max() <= bound(50)
    for j in (1, 2):
        assert (np.abs(rp[j] - r0[j][perm]) / r0[j][perm]).max() <= bound(50)


def test_sample_size_reproduces_the_pin(dev, z):
    X, lab, k = case(z, "a")
    Xd = torch.from_numpy(X).to(dev)
    s = kmeans.silhouette_score(Xd, lab, k, sample_size=200, random_state=3)
    assert abs(s - float(z["silhouette_score_ss"])) <= bound(50)
    v = kmeans.validity(Xd, lab, k, sample_size=200, random_state=3)
    assert v.silhouette == s and np.count_nonzero(~np.isnan(v.samples)) == 200


def test_sweep_on_the_device(dev, z):
    X = z["X_a"]
    Xd = torch.from_numpy(X).to(dev)
    ks = (3, 5, 7)
    r = kmeans.sweep(Xd, ks, random_state=0)
    rn = kmeans.sweep(X, ks, random_state=0, backend="numpy")
    assert r.best_k == rn.best_k == 5 and [row.k for row in r.rows] == list(ks) and r.table().shape == (3, 5)
    for row, rown in zip(r.rows, rn.rows):
        fit = kmeans.kmeans(Xd, row.k, random_state=0)
        assert np.array_equal(row.labels, fit.labels) and np.array_equal(row.centers, fit.centers) and row.inertia == fit.inertia
        assert row.silhouette == kmeans.silhouette_score(Xd, fit.labels, row.k)
        if np.array_equal(row.labels, rown.labels):
            assert abs(row.silhouette - rown.silhouette) <= bound(50)
            assert row.calinski_harabasz == pytest.approx(rown.calinski_harabasz, rel=1e-9)
            assert row.davies_bouldin == pytest.approx(rown.davies_bouldin, rel=1e-9)
    assert api.kmeans_sweep(Xd, (5,), random_state=0).best_k == 5


def test_entry_points_reject_and_launch_nothing(dev):
    L = api.load_library()
    x = torch.zeros((8, 4), device=dev)
    lab = torch.zeros(8, dtype=torch.int32, device=dev)
    out = torch.full((8, 3), 7.0, dtype=torch.float64, device=dev)
    near = torch.full((8,), 7, dtype=torch.int32, device=dev)
    cen = torch.full((2, 4), 7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((2,), 7, dtype=torch.int32, device=dev)
    sq = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    ab = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    s = stream()
    sil, dis = L.ra_kmeans_silhouette, L.ra_kmeans_dispersion
    bad = [sil(None, 8, 4, P(lab), 2, P(out), P(near), s), sil(P(x), 8, 4, None, 2, P(out), P(near), s),
           sil(P(x), 8, 4, P(lab), 2, None, P(near), s), sil(P(x), 8, 4, P(lab), 2, P(out), None, s),
           sil(P(x), 2, 4, P(lab), 2, P(out), P(near), s), sil(P(x), 262145, 4, P(lab), 2, P(out), P(near), s),
           sil(P(x), 8, 0, P(lab), 2, P(out), P(near), s), sil(P(x), 8, 2049, P(lab), 2, P(out), P(near), s),
           sil(P(x), 8, 4, P(lab), 1, P(out), P(near), s), sil(P(x), 8, 4, P(lab), 257, P(out), P(near), s),
           dis(None, 8, 4, P(lab), 2, P(cen), P(cnt), P(sq), P(ab), s), dis(P(x), 8, 4, None, 2, P(cen), P(cnt), P(sq), P(ab), s),
           dis(P(x), 8, 4, P(lab), 2, None, P(cnt), P(sq), P(ab), s), dis(P(x), 8, 4, P(lab), 2, P(cen), None, P(sq), P(ab), s),
           dis(P(x), 8, 4, P(lab), 2, P(cen), P(cnt), None, P(ab), s), dis(P(x), 8, 4, P(lab), 2, P(cen), P(cnt), P(sq), None, s),
           dis(P(x), 0, 4, P(lab), 2, P(cen), P(cnt), P(sq), P(ab), s), dis(P(x), 4194305, 4, P(lab), 2, P(cen), P(cnt), P(sq), P(ab), s),
           dis(P(x), 8, 0, P(lab), 2, P(cen), P(cnt), P(sq), P(ab), s), dis(P(x), 8, 2049, P(lab), 2, P(cen), P(cnt), P(sq), P(ab), s),
           dis(P(x), 8, 4, P(lab), 0, P(cen), P(cnt), P(sq), P(ab), s), dis(P(x), 8, 4, P(lab), 257, P(cen), P(cnt), P(sq), P(ab), s)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ra_kmeans_dispersion" in L.ra_last_error()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(near == 7) and torch.all(cen == 7.0) and torch.all(cnt == 7)
    assert torch.all(sq == 7.0) and torch.all(ab == 7.0)
    # labels outside 0 .. k - 1 are clamped before they address anything
    wild = torch.tensor([-5, 0, 1, 9, 1, 0, 100000, -1], dtype=torch.int32, device=dev)
    xr = torch.arange(32, dtype=torch.float32, device=dev).reshape(8, 4)
    assert sil(P(xr), 8, 4, P(wild), 2, P(out), P(near), s) == 0
    torch.cuda.synchronize()
    ref = kmeans.silhouette_samples(xr.cpu().numpy(), np.clip(wild.cpu().numpy(), 0, 1), 2, backend="numpy")
    assert np.abs(out[:, 0].cpu().numpy() - ref).max() <= bound(4)
    # the python layer: errors before a launch
    with pytest.raises(ValueError, match="Number of labels is 1"):
        kmeans.silhouette_samples(x, np.zeros(8, np.int64), 2)
    with pytest.raises(kmeans.KMeansError):
        kmeans.silhouette_samples(torch.zeros((8, 4), device=dev, dtype=torch.float64), np.arange(8) % 2, 2)
    bx = torch.zeros((8, 4), device=dev)
    bx[3, 1] = float("nan")
    with pytest.raises(kmeans.KMeansError):
        kmeans.validity(bx, np.arange(8) % 2, 2)


def test_tool_end_to_end(dev, tmp_path, capsys):
    X, _ = random_case(400, 10, 4, 9)
    np.save(tmp_path / "x.npy", X)
    assert kmeans.main([str(tmp_path / "x.npy"), str(tmp_path / "w.npz"), "--sweep", "2:6", "--scores", "--sample_size", "200",
                        "--seed", "0"]) == 0
    w = np.load(tmp_path / "w.npz")
    assert set(w.files) == PARENT_KEYS | SCORE_KEYS | {"sweep", "best_k"} and str(w["backend"]) == "device"
    assert w["sweep"].shape == (5, 5) and np.array_equal(w["sweep"][:, 0], [2, 3, 4, 5, 6])
    best = int(w["best_k"])
    assert best == int(w["k"]) == int(w["sweep"][np.argmax(w["sweep"][:, 2]), 0]) == w["centers"].shape[0]
    assert np.count_nonzero(~np.isnan(w["silhouette_samples"])) == 200 and w["class_silhouette"].shape == (best,)
    assert float(w["silhouette"]) == float(w["sweep"][best - 2, 2])
    out = capsys.readouterr().out.splitlines()
    assert out[0].split() == ["k", "inertia", "silhouette", "CH", "DB"] and sum(ln.startswith("class") for ln in out) == best
    assert kmeans.main([str(tmp_path / "x.npy"), str(tmp_path / "p.npz"), "--k", "4", "--seed", "0"]) == 0
    p = np.load(tmp_path / "p.npz")
    assert set(p.files) == PARENT_KEYS and np.array_equal(p["labels"], kmeans.kmeans(torch.from_numpy(X).to(dev), 4, random_state=0).labels)
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
