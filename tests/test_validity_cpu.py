"""Cluster validity on the CPU: the float64 numpy backend of kmeans.silhouette_* / calinski_harabasz_score / davies_bouldin_score
against the scikit-learn 1.7 pins of tests/golden/validity_ref.npz, the errors, the sweep and the tool (no GPU)."""
import os

import numpy as np
import pytest

from cryo_ralib_amd import api, kmeans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = "abosugdt"
PARENT_KEYS = {"labels", "centers", "inertia", "n_iter", "init_indices", "k", "init", "seed", "backend"}
SCORE_KEYS = {"silhouette", "class_silhouette", "silhouette_samples", "calinski_harabasz", "davies_bouldin"}


@pytest.fixture(scope="module")
def z(golden_dir):
    with np.load(os.path.join(golden_dir, "validity_ref.npz")) as f:
        return {k: f[k] for k in f.files}


def case(z, c):
    return z["X_" + c], z["labels_" + c].astype(np.int64), int(z["k_" + c])


@pytest.mark.parametrize("c", CASES)
def test_numpy_backend_matches_sklearn(z, c):
    """s_i to 1e-12, CH and DB to 1e-10 relative.  Measured maxima over the cases: s 9.8e-16, CH 4.4e-16, DB 6.9e-12 (the case
    with +1000 on every coordinate, where sklearn's own Gram expansion of the centroid distances is the less exact side; every
    other case is below 1.2e-14)."""
    X, lab, k = case(z, c)
    sv, a, b, near = kmeans.silhouette_samples(X, lab, k, backend="numpy", details=True)
    assert sv.dtype == np.float64 and sv.shape == (len(X),)
    assert np.abs(sv - z["silhouette_samples_" + c]).max() <= 1e-12
    assert np.array_equal(sv, kmeans.silhouette_samples(X, lab, k, backend="numpy"))
    assert kmeans.silhouette_score(X, lab, k, backend="numpy") == pytest.approx(float(z["silhouette_score_" + c]), abs=1e-12)
    assert kmeans.calinski_harabasz_score(X, lab, k, backend="numpy") == pytest.approx(float(z["calinski_harabasz_score_" + c]), rel=1e-10)
    assert kmeans.davies_bouldin_score(X, lab, k, backend="numpy") == pytest.approx(float(z["davies_bouldin_score_" + c]), rel=1e-10)
    # a, b and nearest restate s; the nearest cluster is never the own one and has members
    cnt = np.bincount(lab, minlength=k)
    assert np.all(near != lab) and np.all(cnt[near] > 0)
    single = cnt[lab] == 1
    assert np.all(sv[single] == 0) and np.all(a[single] == 0)
    mx = np.maximum(a, b)
    ok = ~single & (mx > 0)
    assert np.allclose(sv[ok], ((b - a) / mx)[ok], rtol=0, atol=1e-15) and np.all(sv[~ok] == 0)
    # validity() holds the same numbers, and the mean per class (nan for the unused id)
    v = kmeans.validity(X, lab, k, backend="numpy")
    assert v.silhouette == pytest.approx(float(z["silhouette_score_" + c]), abs=1e-12) and np.array_equal(v.counts, cnt)
    assert v.calinski_harabasz == pytest.approx(float(z["calinski_harabasz_score_" + c]), rel=1e-10)
    assert v.davies_bouldin == pytest.approx(float(z["davies_bouldin_score_" + c]), rel=1e-10)
    for j in range(k):
        if cnt[j]:
            assert v.class_silhouette[j] == pytest.approx(sv[lab == j].mean(), abs=1e-14)
        else:
            assert np.isnan(v.class_silhouette[j])
    assert np.array_equal(v.samples, sv) and v.sample_indices is None


def test_special_cases_are_what_they_claim(z):
    assert np.count_nonzero(np.bincount(z["labels_u"], minlength=8) == 0) == 1
    assert np.bincount(z["labels_g"])[4] == 1 and z["silhouette_samples_g"][0] == 0
    a = kmeans.silhouette_samples(*case(z, "d"), backend="numpy", details=True)[1]
    assert np.all(a[z["labels_d"] == 0] == 0) and len(np.unique(z["X_d"], axis=0)) < 120 - 29
    assert z["X_t"].shape == (3, 2) and np.all(z["X_s"] > 900)


def test_sample_size_follows_sklearns_permutation(z):
    X, lab, k = case(z, "a")
    s = kmeans.silhouette_score(X, lab, k, sample_size=200, random_state=3, backend="numpy")
    assert s == pytest.approx(float(z["silhouette_score_ss"]), abs=1e-12)
    assert s != pytest.approx(float(z["silhouette_score_a"]), abs=1e-6)
    v = kmeans.validity(X, lab, k, sample_size=200, random_state=3, backend="numpy")
    idx = np.random.RandomState(3).permutation(700)[:200]
    assert v.silhouette == pytest.approx(s, abs=1e-15) and np.array_equal(v.sample_indices, idx)
    assert np.count_nonzero(~np.isnan(v.samples)) == 200 and not np.isnan(v.samples[idx]).any()
    assert v.calinski_harabasz == pytest.approx(float(z["calinski_harabasz_score_a"]), rel=1e-10)       # always of all points


def test_number_of_labels_errors():
    X = np.arange(12, dtype=np.float32).reshape(6, 2)
    msg = r"Number of labels is %d\. Valid values are 2 to n_samples - 1 \(inclusive\)"
    for f in (kmeans.silhouette_samples, kmeans.silhouette_score, kmeans.calinski_harabasz_score, kmeans.davies_bouldin_score,
              kmeans.validity):
        with pytest.raises(ValueError, match=msg % 1):
            f(X, np.zeros(6, np.int64), 3, backend="numpy")             # one cluster with members, whatever k says
        with pytest.raises(ValueError, match=msg % 6):
            f(X, np.arange(6), 6, backend="numpy")                      # m = n
    # the check runs on the sample: any 5 of these 6 labels hold two clusters; 3 rows of 3 clusters are m = n
    lab = np.array([0, 0, 0, 1, 1, 1])
    assert np.isfinite(kmeans.silhouette_score(X, lab, 2, sample_size=5, random_state=0, backend="numpy"))
    with pytest.raises(ValueError, match=msg % 3):
        kmeans.silhouette_score(X, np.arange(6), 6, sample_size=3, random_state=1, backend="numpy")


def test_domain_errors():
    X = np.zeros((6, 2), np.float32)
    lab = np.array([0, 0, 0, 1, 1, 1])
    E = kmeans.KMeansError
    with pytest.raises(E):
        kmeans.silhouette_samples(X, lab[:5], 2, backend="numpy")
    with pytest.raises(E):
        kmeans.silhouette_samples(X, lab.astype(np.float64), 2, backend="numpy")
    with pytest.raises(E):
        kmeans.silhouette_samples(X, lab, 1, backend="numpy")           # a label outside 0 .. k - 1
    with pytest.raises(E):
        kmeans.silhouette_samples(X, lab - 1, 2, backend="numpy")
    with pytest.raises(E):
        kmeans.silhouette_samples(X, lab, 257, backend="numpy")
    with pytest.raises(E):
        kmeans.silhouette_samples(X[:2], lab[:2], 2, backend="numpy")   # n < 3
    with pytest.raises(E):
        kmeans.silhouette_samples(np.zeros((6, 2049), np.float32), lab, 2, backend="numpy")
    with pytest.raises(E):
        kmeans.silhouette_samples(X, lab, 2, backend="cpu")
    with pytest.raises(E):
        kmeans.silhouette_score(X, lab, 2, sample_size=0, backend="numpy")
    bad = X.copy()
    bad[0, 0] = np.nan
    with pytest.raises(E):
        kmeans.calinski_harabasz_score(bad, lab, 2, backend="numpy")
    big = np.zeros((kmeans.SIL_MAX_N + 1, 1), np.float32)
    biglab = np.arange(kmeans.SIL_MAX_N + 1) % 2
    with pytest.raises(E, match="sample_size"):
        kmeans.silhouette_samples(big, biglab, 2, backend="numpy")
    with pytest.raises(E, match="sample_size"):
        kmeans.sweep(big, (2, 3), backend="numpy")
    for ks in ((), (3, 3), (5, 4), (1, 2)):
        with pytest.raises(E):
            kmeans.sweep(X, ks, backend="numpy")
    assert kmeans.SIL_MAX_N == 262144


def test_parse_sweep():
    assert kmeans.parse_sweep("2,5,9") == [2, 5, 9] and kmeans.parse_sweep("2:6") == [2, 3, 4, 5, 6]
    assert kmeans.parse_sweep("4:12:4") == [4, 8, 12] and kmeans.parse_sweep("3:3") == [3]
    for bad in ("", "5:2", "3,3", "4,2", "1:4", "2:8:0", "a,b", "2:3:4:5"):
        with pytest.raises(kmeans.KMeansError):
            kmeans.parse_sweep(bad)


def test_sweep_picks_the_planted_number_of_clusters(z):
    X = z["X_a"]
    r = kmeans.sweep(X, (3, 5, 7, 9), random_state=0, backend="numpy")
    assert [row.k for row in r.rows] == [3, 5, 7, 9] and r.best_k == 5
    t = r.table()
    assert t.shape == (4, 5) and np.array_equal(t[:, 0], [3, 5, 7, 9]) and np.argmax(t[:, 2]) == 1
    for row in r.rows:
        fit = kmeans.kmeans(X, row.k, random_state=0, backend="numpy")
        assert np.array_equal(row.labels, fit.labels) and row.inertia == fit.inertia and row.n_iter == fit.n_iter
        assert np.array_equal(row.centers, fit.centers)
        assert row.silhouette == kmeans.silhouette_score(X, fit.labels, row.k, backend="numpy")
        assert row.calinski_harabasz == kmeans.calinski_harabasz_score(X, fit.labels, row.k, backend="numpy")
        assert row.davies_bouldin == kmeans.davies_bouldin_score(X, fit.labels, row.k, backend="numpy")
    # ties go to the smaller k
    r.rows[3].silhouette = r.rows[1].silhouette
    assert kmeans.SweepResult(r.rows).best_k == 5 and kmeans.SweepResult(r.rows[::-1]).best_k == 5
    assert api.kmeans_sweep(X, (5,), random_state=0, backend="numpy").best_k == 5


def test_api_reexports(z):
    X, lab, k = case(z, "t")
    assert np.array_equal(api.silhouette_samples(X, lab, k=k, backend="numpy"), kmeans.silhouette_samples(X, lab, k, backend="numpy"))
    assert api.silhouette_score(X, lab, backend="numpy") == pytest.approx(float(z["silhouette_score_t"]), abs=1e-12)
    assert api.calinski_harabasz_score(X, lab, backend="numpy") == pytest.approx(float(z["calinski_harabasz_score_t"]), rel=1e-10)
    assert api.davies_bouldin_score(X, lab, backend="numpy") == pytest.approx(float(z["davies_bouldin_score_t"]), rel=1e-10)
    assert api.validity(X, lab, backend="numpy").silhouette == pytest.approx(float(z["silhouette_score_t"]), abs=1e-12)
    assert {"ra_kmeans_silhouette", "ra_kmeans_dispersion"} <= set(api.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("argv", [["--k", "3", "--sample_size", "10"], [], ["--sweep", "5:2"], ["--sweep", "3,3"], ["--sweep", ""],
                                  ["--sweep", "4,2", "--k", "3"]])
def test_tool_usage_errors_exit_2_before_anything_is_read(argv, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        kmeans.main([str(tmp_path / "absent.npy"), str(tmp_path / "o.npz"), "--backend", "numpy"] + argv)
    assert e.value.code == 2 and capsys.readouterr().err.strip() and not (tmp_path / "o.npz").exists()


def test_tool_numpy_backend(z, tmp_path, capsys):
    X = z["X_b"]
    np.save(tmp_path / "x.npy", X)
    base = [str(tmp_path / "x.npy")]
    # without the new options: the keys and the one line of the tool as it was
    assert kmeans.main(base + [str(tmp_path / "p.npz"), "--k", "4", "--seed", "0", "--backend", "numpy"]) == 0
    p = np.load(tmp_path / "p.npz")
    fit = kmeans.kmeans(X, 4, random_state=0, backend="numpy")
    assert set(p.files) == PARENT_KEYS and np.array_equal(p["labels"], fit.labels) and float(p["inertia"]) == fit.inertia
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
    # --scores
    assert kmeans.main(base + [str(tmp_path / "s.npz"), "--k", "4", "--seed", "0", "--backend", "numpy", "--scores"]) == 0
    s = np.load(tmp_path / "s.npz")
    assert set(s.files) == PARENT_KEYS | SCORE_KEYS and np.array_equal(s["labels"], fit.labels)
    assert np.array_equal(s["silhouette_samples"], kmeans.silhouette_samples(X, fit.labels, 4, backend="numpy"))
    assert float(s["silhouette"]) == pytest.approx(s["silhouette_samples"].mean(), abs=1e-15) and s["class_silhouette"].shape == (4,)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 5 and all(ln.startswith("class") for ln in lines[:4])
    # --sweep without --k writes best_k's result; with --k that one's
    assert kmeans.main(base + [str(tmp_path / "w.npz"), "--sweep", "6:10:2", "--seed", "0", "--backend", "numpy", "--sample_size",
                               "300", "--scores"]) == 0
    w = np.load(tmp_path / "w.npz")
    assert set(w.files) == PARENT_KEYS | SCORE_KEYS | {"sweep", "best_k"}
    assert w["sweep"].shape == (3, 5) and np.array_equal(w["sweep"][:, 0], [6, 8, 10])
    best = int(w["best_k"])
    assert best == int(w["sweep"][np.argmax(w["sweep"][:, 2]), 0]) == int(w["k"]) == w["centers"].shape[0]
    assert np.array_equal(w["labels"], kmeans.kmeans(X, best, random_state=0, backend="numpy").labels)
    assert np.count_nonzero(~np.isnan(w["silhouette_samples"])) == 300
    assert float(w["silhouette"]) == float(w["sweep"][:, 2].max())
    out = capsys.readouterr().out
    assert "silhouette" in out.splitlines()[0] and "<- best" in out
    assert kmeans.main(base + [str(tmp_path / "v.npz"), "--sweep", "6,8", "--k", "8", "--seed", "0", "--backend", "numpy"]) == 0
    v = np.load(tmp_path / "v.npz")
    assert set(v.files) == PARENT_KEYS | {"sweep", "best_k"} and int(v["k"]) == 8 and int(v["best_k"]) == 6
    assert np.array_equal(v["labels"], kmeans.kmeans(X, 8, random_state=0, backend="numpy").labels)
