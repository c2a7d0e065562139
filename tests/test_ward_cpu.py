"""Ward's float64 numpy backend and the host tree (cryo_ralib_amd/ward.py), without a GPU: every scipy 1.15.3 / scikit-learn 1.7.2
pin of tests/golden/ward_ref.npz, the rounds against the literal greedy definition, inertia as a prefix sum, row-permutation
invariance, duplicates, identical rows, the empty-round guard, the domain, the tool's exit statuses and keys, and the margins of
the builders the GPU suite relies on."""
import os

import numpy as np
import pytest

import ward_cases as wc
from cryo_ralib_amd import api, ward

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "ward_ref.npz"))


@pytest.fixture(scope="module")
def trees(z):
    return {c: ward.linkage(z["X_" + c], backend="numpy", details=True) for c in wc.PIN_NAMES}


def test_pin_inputs_are_the_generators(z):
    for c, X in wc.pin_inputs().items():
        assert np.array_equal(z["X_" + c], X), c


@pytest.mark.parametrize("c", wc.PIN_NAMES)
def test_pin_tree(z, trees, c):
    T, Z = trees[c], z["Z_" + c]
    assert T.margin >= wc.MARGIN and T.height_gap >= wc.MARGIN
    assert np.array_equal(T.children, Z[:, :2].astype(np.int64)) and np.array_equal(T.Z[:, :2], Z[:, :2])
    assert np.array_equal(T.Z[:, 3], Z[:, 3])
    rel = np.abs(T.heights - Z[:, 2]) / Z[:, 2]
    print(c, "heights vs scipy", rel.max())
    assert rel.max() <= max(1000 * EPS, 1e-12)
    assert T.Z.shape == (len(Z), 4) and np.all(np.diff(T.w2) >= 0)


@pytest.mark.parametrize("c", wc.PIN_NAMES)
def test_pin_cuts(z, trees, c):
    T = trees[c]
    for k, lab in zip(z["ks_" + c], z["labels_" + c]):
        got = ward.cut(T, n_clusters=int(k))
        assert got.dtype == np.int32 and got.max() + 1 == k and wc.same_partition(got, lab), (c, k)
        first = [int(np.nonzero(got == j)[0][0]) for j in range(int(k))]
        assert first == sorted(first)                       # numbered by lowest member index
    for t, lab in zip(z["thresholds_" + c], z["tlabels_" + c]):
        got = ward.cut(T, distance_threshold=float(t))
        assert got.max() + 1 == np.count_nonzero(z["Z_" + c][:, 2] >= t) + 1 and wc.same_partition(got, lab), (c, t)


@pytest.mark.parametrize("n,d,seed", [(200, 1, 1), (150, 2, 2), (200, 7, 3), (97, 1, 4), (64, 2, 5), (130, 7, 6)])
def test_rounds_build_the_greedy_tree(n, d, seed):
    X = wc.gaussian(n, d, seed)
    T = ward.linkage(X, backend="numpy", details=True)
    assert T.margin >= wc.MARGIN and T.height_gap >= wc.MARGIN
    m, w = ward.greedy_numpy(X)
    assert np.all(np.diff(w) > 0)                           # the greedy order is the sorted order on tie-free data
    assert np.array_equal(T.merges, m)
    assert np.allclose(T.w2, w, rtol=64 * EPS, atol=0)       # the centroids are formed in another order of merges


def test_inertia_is_the_within_class_sum_of_squares(z, trees):
    for c in ("gauss2", "blobs50"):
        T, X = trees[c], z["X_" + c]
        for k in (1, 2, 5, 17, 100, len(X)):
            direct = wc.inertia_direct(X, ward.cut(T, n_clusters=k))
            assert T.inertia(k) == pytest.approx(direct, rel=1e-10, abs=1e-10 * T.inertia(1)), (c, k)
        assert T.inertia(len(X)) == 0.0
    with pytest.raises(ward.WardError):
        trees["gauss2"].inertia(0)


def test_row_permutation_permutes_the_labels(z, trees):
    X = z["X_gauss5"]
    perm = np.random.default_rng(3).permutation(len(X))
    Tp = ward.linkage(X[perm], backend="numpy")
    assert np.allclose(Tp.heights, trees["gauss5"].heights, rtol=1e-12, atol=0)
    for k in (2, 5, 17):
        assert wc.same_partition(ward.cut(Tp, n_clusters=k), ward.cut(trees["gauss5"], n_clusters=k)[perm])


def test_duplicates_stay_exact():
    X, group = wc.duplicates()
    S = ward._NumpyState(X, False)
    merges, rounds, evaluated = ward._rounds(S, len(X))
    T = ward._tree(len(X), X.shape[1], merges, rounds, evaluated)
    assert np.all(T.w2[:50] == 0) and np.all(T.w2[50:] > 0)          # 25 groups of 3: two zero merges each, and they come first
    at50 = ward.cut(T, n_clusters=25)
    assert wc.same_partition(at50, group)
    # a slot is its cluster's lowest member index; after the zero merges a centroid is bitwise the point
    S2 = ward._NumpyState(X, False)
    for a, b in T.merges[:50]:
        S2.merge(np.array([a]), np.array([b]))
    live = np.nonzero(S2.size > 0)[0]
    assert len(live) == 25 and np.all(S2.size[live] == 3)
    assert np.array_equal(S2.C[live], X[live].astype(np.float64))
    assert np.array_equal(ward.cut(T, distance_threshold=1e-6), at50)


def test_identical_rows_terminate():
    X = wc.identical()
    T = ward.linkage(X, backend="numpy", details=True)
    n = len(X)
    assert np.all(T.heights == 0) and T.margin == 0 and T.height_gap == 0
    assert np.all(T.children.max(axis=1) < n + np.arange(n - 1))     # parents after children
    assert T.Z[-1, 3] == n and np.all(ward.cut(T, n_clusters=1) == 0)
    assert np.array_equal(ward.cut(T, n_clusters=n), np.arange(n))


def test_empty_round_guard(monkeypatch):
    X = wc.gaussian(90, 2, 8)
    want = ward.linkage(X, backend="numpy")
    real, calls = ward.rows_numpy, []

    def stale_once(C, size, rows, details=False):
        calls.append(len(rows))
        nn, w = real(C, size, rows, details)[:2]
        if len(calls) == 2:                                 # stale records: every row of this round still points at a consumed slot
            nn = np.full(len(rows), np.nonzero(np.asarray(size) == 0)[0][0], np.int64)
        return nn, w

    monkeypatch.setattr(ward, "rows_numpy", stale_once)
    got = ward.linkage(X, backend="numpy")
    # the round after the empty one re-evaluates every live row, and the tree is the same one round later
    assert got.n_rounds == want.n_rounds + 1 and calls[0] == 90 and calls[2] == 90 - np.count_nonzero(want.merge_round == 0)
    assert np.array_equal(got.Z, want.Z) and np.array_equal(got.merges, want.merges)

    def never(C, size, rows, details=False):
        return np.full(len(rows), -1, np.int64), np.full(len(rows), np.inf)

    monkeypatch.setattr(ward, "rows_numpy", never)
    with pytest.raises(RuntimeError):
        ward.linkage(X, backend="numpy")


def test_rows_numpy_dead_and_out_of_range():
    C, size = wc.table(65, 3, "alternate", 1)
    nn, w = ward.rows_numpy(C, size, np.array([1, -1, 65, 0, 64]))
    assert list(nn[:3]) == [-1, -1, -1] and np.all(np.isinf(w[:3])) and nn[3] >= 0 and nn[3] % 2 == 0 and nn[4] % 2 == 0
    C, size = wc.table(5, 2, "all_but_two", 2)
    live = np.nonzero(size)[0]
    nn, w = ward.rows_numpy(C, size, live)
    assert list(nn) == [live[1], live[0]] and w[0] == w[1]
    size[live[1]] = 0
    assert ward.rows_numpy(C, size, live[:1])[0][0] == -1


def test_domain_errors():
    X = wc.gaussian(10, 2, 0)
    assert issubclass(ward.WardError, ValueError)
    bad_calls = [
        lambda: ward.linkage(X[:1], backend="numpy"),
        lambda: ward.linkage(np.zeros((4, 0), np.float32), backend="numpy"),
        lambda: ward.linkage(X[0], backend="numpy"),
        lambda: ward.linkage(X, backend="cpu"),
        lambda: ward.linkage(np.where(np.arange(20).reshape(10, 2) == 3, np.nan, X), backend="numpy"),
        lambda: ward.linkage(np.where(np.arange(20).reshape(10, 2) == 3, np.inf, X), backend="numpy"),
        lambda: ward.check_domain(262145, 2),
        lambda: ward.check_domain(100, 2049),
        lambda: ward.ward(X, backend="numpy"),
        lambda: ward.ward(X, n_clusters=2, distance_threshold=1.0, backend="numpy"),
        lambda: ward.ward(X, n_clusters=0, backend="numpy"),
        lambda: ward.ward(X, n_clusters=11, backend="numpy"),
        lambda: ward.ward(X, n_clusters=2.0, backend="numpy"),
        lambda: ward.ward(X, distance_threshold=0.0, backend="numpy"),
        lambda: ward.ward(X, distance_threshold=-1.0, backend="numpy"),
        lambda: ward.ward(X, distance_threshold=float("nan"), backend="numpy"),
        lambda: ward.sweep(X, [], backend="numpy"),
        lambda: ward.sweep(X, [3, 2], backend="numpy"),
        lambda: ward.sweep(X, [1, 2], backend="numpy"),
        lambda: ward.sweep(X, [2, 10], backend="numpy"),
        lambda: ward.greedy_numpy(np.zeros((201, 2), np.float32)),
    ]
    for call in bad_calls:
        with pytest.raises(ward.WardError):
            call()
    ward.check_domain(262144, 2048)
    ward.check_domain(2, 1)
    assert {"ra_ward_nearest", "ra_ward_merge"} <= set(api.EXPORTED_SYMBOLS)
    assert all(hasattr(api, f) for f in ("ward", "ward_linkage", "ward_cut", "ward_sweep"))


def test_public_calls_numpy(z, trees):
    X = z["X_gauss2"]
    res = api.ward(X, n_clusters=5, backend="numpy")
    assert np.array_equal(res.labels, ward.cut(trees["gauss2"], n_clusters=5)) and res.n_clusters == 5
    assert np.array_equal(res.counts, np.bincount(res.labels)) and res.centers.dtype == np.float64
    for c in range(5):
        assert np.allclose(res.centers[c], X[res.labels == c].astype(np.float64).mean(axis=0), rtol=1e-12, atol=1e-14)
    assert res.inertia == trees["gauss2"].inertia(5)
    assert np.array_equal(api.ward_cut(api.ward_linkage(X, backend="numpy"), distance_threshold=2.0),
                          ward.cut(trees["gauss2"], distance_threshold=2.0))
    from cryo_ralib_amd import kmeans
    sw = api.ward_sweep(X, [2, 3, 5, 8], backend="numpy")
    assert [r.k for r in sw.rows] == [2, 3, 5, 8] and sw.best_k in (2, 3, 5, 8)
    for r in sw.rows:
        assert np.array_equal(r.labels, ward.cut(trees["gauss2"], n_clusters=r.k)) and r.inertia == trees["gauss2"].inertia(r.k)
        v = kmeans.validity(X, r.labels, r.k, backend="numpy")
        assert (r.silhouette, r.calinski_harabasz, r.davies_bouldin) == (v.silhouette, v.calinski_harabasz, v.davies_bouldin)
    best = max(sw.rows, key=lambda r: (r.silhouette, -r.k))
    assert sw.best_k == best.k and sw.table().shape == (4, 5)


def test_tool_exit_statuses_and_keys(z, trees, tmp_path, capsys):
    X = z["X_gauss2"]
    np.save(tmp_path / "x.npy", X)
    x, o, a = str(tmp_path / "x.npy"), str(tmp_path / "o.npz"), str(tmp_path / "a.npy")
    bad = [[x, o], [x, o, "--k", "3", "--distance_threshold", "1.0"], [x, o, "--sweep", ""], [x, o, "--sweep", "5,4"],
           [x, o, "--sweep", "4:2"], [x, o, "--sweep", "2,2"], [x, o, "--k", "3", "--sample_size", "50"],
           [x, o, "--k", "3", "--averages", a], [x, o, "--k", "3", "--averages", a, "--stack", x, "--ou", "12"],
           [x, o, "--k", "0"], [x, o, "--distance_threshold", "0"], [x, o, "--sweep", "2:4", "--distance_threshold", "1.0"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            ward.main(argv + ["--backend", "numpy"])
        assert e.value.code == 2, argv
        assert not os.path.exists(o)
    capsys.readouterr()
    T = trees["gauss2"]
    assert ward.main([x, o, "--backend", "numpy", "--k", "5", "--scores"]) == 0
    f = np.load(o)
    for key in ("labels", "linkage", "n_clusters", "counts", "inertia", "n_rounds", "rows_evaluated", "k", "distance_threshold", "key",
                "backend", "seed", "silhouette", "class_silhouette", "silhouette_samples", "calinski_harabasz", "davies_bouldin"):
        assert key in f.files, key
    assert np.array_equal(f["labels"], ward.cut(T, n_clusters=5)) and np.array_equal(f["linkage"], T.Z)
    assert f["n_clusters"] == 5 and f["inertia"] == T.inertia(5) and f["n_rounds"] == T.n_rounds
    assert f["rows_evaluated"] == T.rows_evaluated and np.array_equal(f["counts"], np.bincount(f["labels"]))
    from cryo_ralib_amd import tsne
    assert np.array_equal(tsne.read_fit_labels(o), f["labels"])     # the tsne tool's --fit_labels takes OUT.npz as it is
    assert ward.main([x, o, "--backend", "numpy", "--distance_threshold", "3.0"]) == 0
    f = np.load(o)
    assert np.array_equal(f["labels"], ward.cut(T, distance_threshold=3.0)) and f["distance_threshold"] == 3.0 and f["k"] == -1
    assert ward.main([x, o, "--backend", "numpy", "--sweep", "2:6:2", "--sample_size", "100", "--seed", "1"]) == 0
    f = np.load(o)
    assert f["sweep"].shape == (3, 5) and list(f["sweep"][:, 0]) == [2, 4, 6] and f["best_k"] in (2, 4, 6)
    assert np.array_equal(f["labels"], ward.cut(T, n_clusters=int(f["best_k"])))
    assert np.array_equal(f["sweep"][:, 1], [T.inertia(k) for k in (2, 4, 6)])
    assert ward.main([x, o, "--backend", "numpy", "--sweep", "2,3", "--k", "7"]) == 0
    assert np.array_equal(np.load(o)["labels"], ward.cut(T, n_clusters=7))
    with pytest.raises(SystemExit) as e:
        ward.main([x, o, "--backend", "numpy", "--k", "301"])
    assert e.value.code not in (0, 2)
    capsys.readouterr()


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 193])
def test_gpu_builders_keep_their_margin(n):
    """the row-wise margins of the states tests/test_gpu_ward.py hands to ra_ward_nearest"""
    for d in (1, 31, 32, 33, 65):
        for dead in wc.DEAD_PATTERNS:
            C, size = wc.table(n, d, dead, 1000 * n + d)
            nn, w, margin = ward.rows_numpy(C, size, np.arange(n), details=True)
            assert margin >= wc.MARGIN, (n, d, dead, margin)
            assert np.all((nn >= 0) == (size > 0)) or np.count_nonzero(size) < 2


def test_whole_tree_builders_keep_their_margin():
    T = ward.linkage(wc.line(600), backend="numpy", details=True)
    print("line: rounds", T.n_rounds, "rows / n", T.rows_evaluated / 600, "margin", T.margin, "height gap", T.height_gap)
    assert T.margin >= wc.MARGIN and T.height_gap >= wc.MARGIN and T.n_rounds >= 290
