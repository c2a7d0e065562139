"""Gaussian mixtures, the float64 numpy backend (no GPU): every case of tests/golden/gmm_ref.npz (scikit-learn 1.7 values, written
by tests/golden/make_gmm_pins.py) within the stored bars, the ill-defined-covariance error, the convergence warning, every domain
error, sweep / best_k and the command-line tool."""
import os
import warnings

import numpy as np
import pytest

from cryo_ralib_amd import api, gmm, kmeans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_ref.npz")
CASES = ["full3", "diag3", "full16", "diag50", "full33", "full1", "random3", "maxiter5"]
PINNED = ("means", "covariances", "weights", "lower_bound")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def case(z, c):
    """(X float32, k, keyword arguments of gmm.gmm) of pin case c"""
    X = z[c + "_x64"].astype(np.float32) / np.float32(64.0)
    k, n_init, max_iter, seed = (int(v) for v in z[c + "_opts"])
    return X, k, dict(covariance_type=str(z[c + "_cov"]), init_params=str(z[c + "_init"]), n_init=n_init, max_iter=max_iter,
                      random_state=seed)


def check_against_pins(z, c, r, X, backend):
    """labels, n_iter, converged and init_labels exact; parameters, bic, aic and score_samples within the stored bars"""
    assert r.labels.dtype == np.int32 and r.means.dtype == np.float64
    assert np.array_equal(r.labels, z[c + "_labels"].astype(np.int32)), c
    assert r.n_iter == int(z[c + "_n_iter"]) and r.converged == bool(z[c + "_converged"]), (c, r.n_iter)
    if z[c + "_init_labels"].size:
        assert np.array_equal(r.init_labels, z[c + "_init_labels"].astype(np.int32)), c
    else:
        assert r.init_labels is None
    got = dict(means=r.means, covariances=r.covariances, weights=r.weights, lower_bound=r.lower_bound,
               score_samples=gmm.score_samples(X, r, backend=backend), bic=gmm.bic(X, r, backend=backend),
               aic=gmm.aic(X, r, backend=backend))
    for key, v in got.items():
        err = float(np.max(np.abs(np.asarray(v) - z["%s_%s" % (c, key)])))
        print("%s %s %s: error %.3e, bar %.3e" % (backend, c, key, err, float(z["%s_tol_%s" % (c, key)])))
    for key, v in got.items():
        err = float(np.max(np.abs(np.asarray(v) - z["%s_%s" % (c, key)])))
        assert err <= float(z["%s_tol_%s" % (c, key)]), (c, key, err, float(z["%s_tol_%s" % (c, key)]))
    assert len(r.lower_bounds) == r.n_iter and r.lower_bounds[-1] == r.lower_bound
    assert np.array_equal(r.log_prob, got["score_samples"])


def fit(X, k, kw, backend, expect_warning):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = gmm.gmm(X, k, backend=backend, **kw)
    got = [x for x in w if issubclass(x.category, kmeans.ConvergenceWarning)]
    assert bool(got) == expect_warning
    if got:
        assert str(got[0].message) == gmm.NOT_CONVERGED
    return r


@pytest.mark.parametrize("c", CASES)
def test_numpy_backend_matches_sklearn_pins(z, c):
    X, k, kw = case(z, c)
    r = fit(X, k, kw, "numpy", not bool(z[c + "_converged"]))
    check_against_pins(z, c, r, X, "numpy")
    proba = gmm.predict_proba(X, r, backend="numpy")
    assert proba.shape == (X.shape[0], k) and np.allclose(proba.sum(axis=1), 1.0, atol=1e-12)
    assert np.array_equal(gmm.predict(X, r, backend="numpy"), r.labels)
    assert np.array_equal(np.max(proba, axis=1), r.proba_max)
    assert gmm.score(X, r, backend="numpy") >= r.lower_bound - 1e-9        # EM never lowers the likelihood


def test_full_and_diag_differ_and_parameter_counts(z):
    rf = gmm.gmm(*case(z, "full3")[:2], backend="numpy", **case(z, "full3")[2])
    rd = gmm.gmm(*case(z, "diag3")[:2], backend="numpy", **case(z, "diag3")[2])
    assert rf.covariances.shape == (4, 3, 3) and rd.covariances.shape == (4, 3)
    assert np.sum(rf.labels != rd.labels) > 0
    assert gmm.n_parameters(rf) == 4 * 3 * 4 // 2 + 4 * 3 + 3 and gmm.n_parameters(rd) == 2 * 4 * 3 + 3
    pc = rf.precisions_cholesky
    assert np.all(np.tril(pc, -1) == 0.0)
    for c in range(4):
        assert np.allclose(pc[c] @ pc[c].T, np.linalg.inv(rf.covariances[c]), rtol=1e-9, atol=1e-9)


def test_given_labels_start_a_fit(z):
    X, k, kw = case(z, "full3")
    km = kmeans.kmeans(X, k, random_state=kw["random_state"], backend="numpy")
    kw2 = dict(kw, init_params=km.labels)
    a = gmm.gmm(X, k, backend="numpy", **kw2)
    b = gmm.gmm(X, k, backend="numpy", **kw)
    assert np.array_equal(a.init_labels, km.labels) and np.array_equal(a.labels, b.labels) and a.n_iter == b.n_iter


def test_ill_defined_covariance_raises_sklearns_error():
    X = np.repeat(np.array([[0.0, 0.0], [4.0, 4.0]], np.float32), 10, axis=0)
    lab = np.repeat(np.array([0, 1]), 10)
    for cov in ("full", "diag"):
        with pytest.raises(ValueError, match="ill-defined empirical covariance") as e:
            gmm.gmm(X, 2, covariance_type=cov, reg_covar=0.0, init_params=lab, backend="numpy")
        assert str(e.value) == gmm.ILL_DEFINED and not isinstance(e.value, gmm.GmmError)
    r = gmm.gmm(X, 2, covariance_type="full", init_params=lab, backend="numpy")        # reg_covar = 1e-6 rescues it
    assert np.array_equal(r.labels, lab)


def test_domain_errors():
    X = np.zeros((40, 3), np.float32)
    bad = [dict(n_components=0), dict(n_components=41), dict(n_components=257), dict(n_components=2, covariance_type="tied"),
           dict(n_components=2, covariance_type="spherical"), dict(n_components=2, max_iter=0), dict(n_components=2, n_init=0),
           dict(n_components=2, tol=-1.0), dict(n_components=2, tol=float("nan")), dict(n_components=2, reg_covar=-1e-6),
           dict(n_components=2, init_params="k-means++"), dict(n_components=2, init_params="random_from_data"),
           dict(n_components=2, init_params=np.zeros(39, np.int64)), dict(n_components=2, init_params=np.full(40, 2)),
           dict(n_components=2, init_params=np.zeros(40)), dict(n_components=2, random_state="x"), dict(n_components=2.0),
           dict(n_components=2, backend="cuda")]
    for kw in bad:
        kw.setdefault("backend", "numpy")
        with pytest.raises(gmm.GmmError):
            gmm.gmm(X, **kw)
    for shape, cov in (((300, 257), "full"), ((10, 2049), "diag")):
        with pytest.raises(gmm.GmmError):
            gmm.gmm(np.zeros(shape, np.float32), 2, covariance_type=cov, backend="numpy")
    gmm.check_domain(300, 257, 2, "diag")
    gmm.check_domain(1 << 20, 4, 256)
    with pytest.raises(gmm.GmmError):
        gmm.check_domain((1 << 20) + 1, 4, 256)             # n k > 2^28
    with pytest.raises(gmm.GmmError):
        gmm.check_domain(4194305, 4, 2)
    with pytest.raises(gmm.GmmError):
        gmm.gmm(np.zeros((40,), np.float32), 2, backend="numpy")
    for v in (np.nan, np.inf):
        Xb = X.copy()
        Xb[3, 1] = v
        with pytest.raises(gmm.GmmError):
            gmm.gmm(Xb, 2, backend="numpy")
    r = gmm.gmm(np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32), 2, random_state=0, backend="numpy")
    with pytest.raises(gmm.GmmError):
        gmm.predict(np.zeros((40, 4), np.float32), r, backend="numpy")


def test_sweep_and_best_k(z):
    X, k, kw = case(z, "full3")
    s = gmm.sweep(X, [2, 3, 4, 5], backend="numpy", random_state=0)
    assert [r.k for r in s.rows] == [2, 3, 4, 5] and s.table().shape == (4, 6)
    assert s.best_k == min(s.rows, key=lambda r: (r.bic, r.k)).k
    for r in s.rows:
        assert r.bic == gmm.bic(X, r.model, backend="numpy") and r.aic == gmm.aic(X, r.model, backend="numpy")
        assert r.labels.shape == (600,) and r.bic - r.aic == pytest.approx(gmm.n_parameters(r.model) * (np.log(600) - 2.0))
    # ties: the smaller k
    a, b = s.rows[1], s.rows[2]
    b2 = gmm.SweepRow(b.k, b.model)
    b2.bic = a.bic
    assert gmm.SweepResult([a, b2]).best_k == a.k and gmm.SweepResult([b2, a]).best_k == a.k
    for ks in ([], [3, 3], [4, 2], [0, 1]):
        with pytest.raises(gmm.GmmError):
            gmm.sweep(X, ks, backend="numpy")
    assert api.gmm(X, 2, backend="numpy", random_state=0).means.shape == (2, 3)
    assert api.gmm_sweep(X, [2], backend="numpy", random_state=0).best_k == 2
    m = api.gmm(X, 2, backend="numpy", random_state=0)
    assert api.gmm_predict_proba(X, m, backend="numpy").shape == (600, 2)


def test_tool_writes_the_documented_keys_and_rejects_bad_options(z, tmp_path, capsys):
    X, k, kw = case(z, "full3")
    np.save(tmp_path / "x.npy", X)
    np.savez(tmp_path / "f.npz", factors=X)
    truth = z["full3_labels"].astype(np.int64)
    np.save(tmp_path / "truth.npy", truth)
    out = str(tmp_path / "o.npz")
    assert gmm.main([str(tmp_path / "f.npz"), out, "--k", "4", "--seed", "0", "--backend", "numpy", "--truth", str(tmp_path / "truth.npy"),
                     "--min_proba", "0.9"]) == 0
    o = np.load(out)
    for key in ("weights", "means", "covariances", "precisions_cholesky", "labels", "proba_max", "log_likelihood", "lower_bound", "n_iter",
                "converged", "bic", "aic", "k", "cov", "init", "n_init", "max_iter", "tol", "reg_covar", "seed", "backend", "keep",
                "min_proba", "purity", "c_purity", "contingency"):
        assert key in o.files, key
    assert np.array_equal(o["labels"], truth) and float(o["purity"]) == 1.0 and int(o["n_iter"]) == int(z["full3_n_iter"])
    assert np.array_equal(o["keep"], o["proba_max"] >= 0.9) and o["log_likelihood"].shape == (600,)
    assert "kept" in capsys.readouterr().out
    assert gmm.main([str(tmp_path / "x.npy"), out, "--sweep", "2:5", "--cov", "diag", "--seed", "0", "--backend", "numpy"]) == 0
    o = np.load(out)
    assert o["sweep"].shape == (4, 6) and int(o["best_k"]) == int(o["k"]) and str(o["cov"]) == "diag"
    assert o["covariances"].shape == (int(o["k"]), 3)
    np.save(tmp_path / "lab.npy", truth)
    assert gmm.main([str(tmp_path / "x.npy"), out, "--k", "4", "--init", str(tmp_path / "lab.npy"), "--backend", "numpy"]) == 0
    o = np.load(out)
    assert str(o["init"]).endswith("lab.npy") and kmeans.purity_score(truth, o["labels"]) >= 0.95
    assert gmm.main([str(tmp_path / "x.npy"), out, "--k", "4", "--sweep", "2,3", "--seed", "0", "--backend", "numpy"]) == 0
    o = np.load(out)
    assert int(o["k"]) == 4 and int(o["best_k"]) in (2, 3) and o["means"].shape == (4, 3)
    for argv in ([], ["--k", "3", "--min_proba", "0"], ["--k", "3", "--min_proba", "1.5"], ["--sweep", "5:2"], ["--sweep", "3,3"],
                 ["--sweep", ""], ["--k", "3", "--cov", "tied"]):
        with pytest.raises(SystemExit) as e:
            gmm.main([str(tmp_path / "missing.npy"), out] + argv + ["--backend", "numpy"])
        assert e.value.code == 2, argv
    with pytest.raises(SystemExit) as e:
        gmm.main([str(tmp_path / "x.npy"), out, "--k", "601", "--backend", "numpy"])
    assert "error" in str(e.value.code)
