"""k-means without a GPU: the numpy backend (the CPU checker) against scikit-learn 1.7's values (tests/golden/kmeans_ref.npz,
made by tests/golden/make_kmeans_pins.py), the purity scores, the domain errors and the tool."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from cryo_ralib_amd import kmeans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kmeans_ref.npz")
CASES = ["a1", "a2", "ar", "b", "e", "u", "o"]


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def case(z, c):
    """(X, k, kwargs of kmeans.kmeans) of fixture case c"""
    X = z["X_" + str(z["xkey_" + c])]
    init = str(z["init_" + c])
    kw = dict(n_init=int(z["n_init_" + c]))
    if init == "array":
        kw["init"] = z["init_array_" + c]
    else:
        kw["init"], kw["random_state"] = init, int(z["seed_" + c])
    return X, int(z["k_" + c]), kw


def check_against_fixture(z, c, r, centre_rtol, inertia_rtol):
    assert np.array_equal(r.labels, z["labels_" + c].astype(np.int32)), c
    assert r.n_iter == int(z["n_iter_" + c]), (c, r.n_iter, int(z["n_iter_" + c]))
    ref_idx = z["init_indices_" + c]
    if ref_idx.size:
        assert np.array_equal(r.init_indices, ref_idx), (c, r.init_indices, ref_idx)
    else:
        assert r.init_indices is None
    C = z["centers_" + c]
    assert r.centers.shape == C.shape and r.centers.dtype == np.float64
    assert np.abs(r.centers - C).max() <= centre_rtol * max(np.abs(C).max(), 1e-300), c
    inertia = float(z["inertia_" + c])
    assert abs(r.inertia - inertia) <= inertia_rtol * max(inertia, 1e-300) + 1e-12, (c, r.inertia, inertia)


@pytest.mark.parametrize("c", CASES)
def test_numpy_backend_matches_sklearn(z, c):
    X, k, kw = case(z, c)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = kmeans.kmeans(X, k, backend="numpy", **kw)
    check_against_fixture(z, c, r, 1e-10, 1e-10)
    distinct = len(np.unique(z["labels_" + c]))
    warned = [x for x in w if issubclass(x.category, kmeans.ConvergenceWarning)]
    assert (len(warned) == 1) == (distinct < k), c
    if warned:
        assert "Number of distinct clusters (%d) found smaller than n_clusters (%d)" % (distinct, k) in str(warned[0].message)


def test_relocation_case_has_an_empty_cluster_first(z):
    X, k, kw = case(z, "e")
    B = kmeans._Numpy(X)
    lab, _ = B.assign(np.asarray(kw["init"], np.float64))
    assert len(np.unique(lab)) == k - 1                    # the far centre wins no point in the first E-step
    C1, _, _ = B.lloyd(np.asarray(kw["init"], np.float64))
    assert np.abs(C1[k - 1]).max() < 100                   # ... and is relocated onto a point


def test_purity_matches_utils_ralib(z):
    y, lab = z["y_a"], z["labels_a1"]
    assert np.array_equal(kmeans.contingency_matrix(y, lab), z["contingency_a1"])
    assert kmeans.purity_score(y, lab) == pytest.approx(float(z["purity_a1"]), abs=1e-15)
    assert kmeans.c_purity_score(y, lab) == pytest.approx(float(z["c_purity_a1"]), abs=1e-15)
    # a hand-made case: classes 0, 0, 1, 1, 2 against clusters 5, 5, 5, 7, 7
    yt, yp = [0, 0, 1, 1, 2], [5, 5, 5, 7, 7]
    assert np.array_equal(kmeans.contingency_matrix(yt, yp), [[2, 0], [1, 1], [0, 1]])
    assert kmeans.purity_score(yt, yp) == pytest.approx(3 / 5)
    assert kmeans.c_purity_score(yt, yp) == pytest.approx(4 / 5)


def test_plusplus_trials_and_tolerance():
    assert [kmeans.n_local_trials(k) for k in (1, 2, 3, 8, 12, 256)] == [2, 2, 3, 4, 4, 7]
    X = np.random.default_rng(0).normal(size=(100, 3))
    assert kmeans.tolerance(X, 1e-4) == pytest.approx(np.var(X, axis=0).mean() * 1e-4, rel=1e-15)
    assert kmeans.tolerance(X, 0) == 0.0


def test_random_state_forms(z):
    X, k, kw = case(z, "b")
    a = kmeans.kmeans(X, k, random_state=np.random.RandomState(3), backend="numpy")
    assert np.array_equal(a.labels, z["labels_b"].astype(np.int32))
    kmeans.kmeans(X, k, random_state=None, backend="numpy")             # fresh entropy: runs


def test_is_same_clustering():
    assert kmeans.is_same_clustering([0, 0, 1, 2], [2, 2, 0, 1], 3)
    assert not kmeans.is_same_clustering([0, 0, 1, 2], [2, 1, 0, 1], 3)


def test_domain_errors_before_any_work():
    X = np.zeros((10, 3), np.float32)
    bad = [dict(n_clusters=0), dict(n_clusters=11), dict(n_clusters=257), dict(n_clusters=2, max_iter=0),
           dict(n_clusters=2, tol=-1.0), dict(n_clusters=2, tol=float("nan")), dict(n_clusters=2, n_init=0),
           dict(n_clusters=2, init="kmeans"), dict(n_clusters=2, init=np.zeros((3, 3))), dict(n_clusters=2, random_state="x"),
           dict(n_clusters=2, backend="cpu"), dict(n_clusters=2.0)]
    for kw in bad:
        with pytest.raises(kmeans.KMeansError):
            kmeans.kmeans(X, backend=kw.pop("backend", "numpy"), **kw)
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(np.zeros((10, 2049), np.float32), 2, backend="numpy")
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(np.zeros(10, np.float32), 2, backend="numpy")
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(Xn, 2, backend="numpy")
    with pytest.raises(kmeans.KMeansError):
        kmeans.check_domain(kmeans.MAX_N + 1, 3, 2)
    with pytest.raises(kmeans.KMeansError):
        kmeans.kmeans(X, 2, init=np.full((2, 3), np.inf), backend="numpy")


def test_tool_numpy_backend(z, tmp_path):
    X, y = z["X_a"], z["y_a"].astype(np.int64)
    np.savez(tmp_path / "f.npz", factors=X)
    np.save(tmp_path / "y.npy", y)
    rc = subprocess.run([sys.executable, "-m", "cryo_ralib_amd.kmeans", str(tmp_path / "f.npz"), str(tmp_path / "o.npz"), "--k", "12",
                         "--seed", "0", "--backend", "numpy", "--truth", str(tmp_path / "y.npy")], cwd=ROOT, capture_output=True,
                        text=True)
    assert rc.returncode == 0, rc.stderr
    o = np.load(tmp_path / "o.npz")
    assert np.array_equal(o["labels"], z["labels_a1"].astype(np.int32)) and int(o["n_iter"]) == int(z["n_iter_a1"])
    assert np.array_equal(o["init_indices"], z["init_indices_a1"])
    assert float(o["purity"]) == pytest.approx(float(z["purity_a1"])) and np.array_equal(o["contingency"], z["contingency_a1"])
    # a params.txt as truth (class in the last column, rows in any order) and an init array from a file
    rows = np.zeros((2000, 6))
    rows[:, 0] = np.arange(2000)[::-1]
    rows[:, 5] = y[::-1]
    np.savetxt(tmp_path / "params.txt", rows)
    np.save(tmp_path / "init.npy", z["centers_a1"])
    assert kmeans.main([str(tmp_path / "f.npz"), str(tmp_path / "p.npz"), "--k", "12", "--backend", "numpy", "--init",
                        str(tmp_path / "init.npy"), "--truth", str(tmp_path / "params.txt")]) == 0
    p = np.load(tmp_path / "p.npz")
    assert np.array_equal(p["labels"], z["labels_a1"].astype(np.int32)) and int(p["n_iter"]) == 1
    assert float(p["c_purity"]) == pytest.approx(float(z["c_purity_a1"]))
    with pytest.raises(SystemExit):
        kmeans.main([str(tmp_path / "f.npz"), str(tmp_path / "q.npz"), "--k", "0", "--backend", "numpy"])
    with pytest.raises(SystemExit):
        kmeans.main([str(tmp_path / "f.npz"), str(tmp_path / "q.npz"), "--k", "3", "--key", "embedding", "--backend", "numpy"])
