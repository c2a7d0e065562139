"""DBSCAN without a GPU (cryo_ralib_amd/dbscan.py): the float64 numpy backend against every scikit-learn 1.7 pin of
tests/golden/dbscan_ref.npz (exact equality: the pins' data is quantised so that every decision is exact), the k-distance
identity, the row-permutation property, the domain errors, the binding's symbols and the tool."""
import os

import numpy as np
import pytest

from cryo_ralib_amd import api, dbscan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan_ref.npz")
CASES = "abcdefgh"


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def case(z, c):
    return z["X_" + c], float(z["eps_" + c]), int(z["min_samples_" + c])


@pytest.fixture(scope="module")
def fits(z):
    """the numpy backend's result of every pin, computed once"""
    return {c: dbscan.dbscan(*case(z, c), backend="numpy") for c in CASES}


@pytest.mark.parametrize("c", CASES)
def test_numpy_backend_equals_sklearn(z, fits, c):
    X, eps, ms = case(z, c)
    r = fits[c]
    lab, core = z["labels_" + c], z["core_sample_indices_" + c]
    assert r.labels.dtype == np.int32 and r.core_mask.dtype == np.bool_ and r.counts.dtype == np.int32
    assert np.array_equal(r.labels, lab)
    assert np.array_equal(r.core_sample_indices, core) and np.array_equal(np.nonzero(r.core_mask)[0], core)
    assert r.n_clusters == int(lab.max()) + 1 and r.n_noise == np.count_nonzero(lab < 0)
    assert np.array_equal(r.core_mask, r.counts >= ms) and r.counts.min() >= 1 and r.n_rounds >= 1


def test_pins_cover_what_they_are_for(z, fits):
    assert fits["b"].n_noise > 100 and np.count_nonzero((fits["b"].labels >= 0) & ~fits["b"].core_mask) > 200
    assert fits["d"].n_clusters > 50 and fits["e"].n_clusters == 1 and fits["e"].core_mask.all()
    assert fits["f"].n_noise == 0 and fits["f"].core_mask.all()
    assert fits["g"].n_clusters == 0 and fits["g"].n_noise == 60 and fits["g"].n_rounds == 1
    assert fits["h"].n_clusters == 4 and np.array_equal(np.unique(fits["h"].counts), [40, 80])
    X, eps, _ = case(z, "a")
    Xd = X.astype(np.float64)
    D2 = ((Xd[:, None, :] - Xd[None, :, :]) ** 2).sum(-1)
    assert np.count_nonzero(np.triu(D2 == eps * eps, 1)) > 100          # pairs at exactly eps: the test is inclusive


@pytest.mark.parametrize("c", CASES)
def test_kdistances_identity(z, fits, c):
    X, eps, ms = case(z, c)
    kd = dbscan.kdistances(X, ms, backend="numpy")
    assert kd.dtype == np.float64 and kd.shape == (len(X),)
    assert np.array_equal(fits[c].core_mask, kd <= eps)
    if ms == 1:
        assert np.all(kd == 0.0)
    if ms > len(X):
        assert np.all(np.isinf(kd))


def same_partition(a, b):
    """two labelings of the same points split them alike"""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("c", "bdh")
def test_row_permutation(z, fits, c):
    """the noise set and the partition of the core points do not depend on the order of the rows (border labels may move)"""
    X, eps, ms = case(z, c)
    perm = np.random.default_rng(11).permutation(len(X))
    r, rp = fits[c], dbscan.dbscan(X[perm], eps, ms, backend="numpy")
    assert np.array_equal(rp.core_mask, r.core_mask[perm]) and np.array_equal(rp.counts, r.counts[perm])
    assert np.array_equal(rp.labels < 0, r.labels[perm] < 0)
    cm = rp.core_mask
    assert rp.n_clusters == r.n_clusters and same_partition(rp.labels[cm], r.labels[perm][cm])


def test_border_point_takes_the_lower_cluster():
    """two far clusters joined by one border point that touches a core point of each: the cluster opened first wins"""
    hi, lo, mid = [[10.0], [10.25], [10.5], [10.75]], [[8.0], [7.75], [7.5], [7.25]], [[9.0]]      # 9 is at exactly eps from 10 and from 8
    for first, second in ((hi, lo), (lo, hi)):
        r = dbscan.dbscan(np.array(first + mid + second, np.float32), 1.0, 4, backend="numpy")
        assert r.labels.tolist() == [0] * 5 + [1] * 4 and r.n_clusters == 2
        assert r.core_mask.tolist() == [True] * 4 + [False] + [True] * 4 and r.counts[4] == 3


def test_domain_errors():
    X = np.zeros((8, 3), np.float32)
    for eps in (0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(dbscan.DbscanError):
            dbscan.dbscan(X, eps, 5, backend="numpy")
    for ms in (0, -3, 2.5, "4", True):
        with pytest.raises(dbscan.DbscanError):
            dbscan.dbscan(X, 1.0, ms, backend="numpy")
        with pytest.raises(dbscan.DbscanError):
            dbscan.kdistances(X, ms, backend="numpy")
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(np.zeros((0, 3), np.float32), 1.0, backend="numpy")
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(np.zeros((8, 0), np.float32), 1.0, backend="numpy")
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(np.zeros((4, 2049), np.float32), 1.0, backend="numpy")
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(np.zeros(8, np.float32), 1.0, backend="numpy")
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(X, 1.0, backend="host")
    bad = X.copy()
    bad[3, 1] = np.inf
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(bad, 1.0, backend="numpy")
    with pytest.raises(dbscan.DbscanError):
        dbscan.check_domain(262145, 2, 1.0, 5)
    assert issubclass(dbscan.DbscanError, ValueError)
    assert dbscan.dbscan(X, 1.0, 10 ** 12, backend="numpy").n_noise == 8          # any integer min_samples >= 1 is inside the domain


def test_binding_declares_the_entries():
    assert {"ra_dbscan_count", "ra_dbscan_step"} <= set(api.EXPORTED_SYMBOLS)
    assert api.dbscan(np.zeros((3, 2), np.float32), 1.0, min_samples=2, backend="numpy").n_clusters == 1
    assert np.all(api.dbscan_kdistances(np.zeros((3, 2), np.float32), 2, backend="numpy") == 0.0)


def run_tool(args):
    try:
        return dbscan.main([str(a) for a in args])
    except SystemExit as e:
        return e.code


def test_tool_exit_2_cases(tmp_path, capsys):
    np.save(tmp_path / "x.npy", np.zeros((10, 2), np.float32))
    x, o = tmp_path / "x.npy", tmp_path / "o.npz"
    assert run_tool([x, o, "--backend", "numpy"]) == 2                                      # neither --eps nor --kdist
    assert run_tool([x, o, "--backend", "numpy", "--eps", "0"]) == 2
    assert run_tool([x, o, "--backend", "numpy", "--eps", "-0.5"]) == 2
    assert run_tool([x, o, "--backend", "numpy", "--eps", "1", "--averages", tmp_path / "r.npy"]) == 2
    assert run_tool([x, o, "--backend", "numpy", "--eps", "1", "--averages", tmp_path / "r.npy", "--stack", x, "--ou", "3"]) == 2
    assert not o.exists()
    capsys.readouterr()


def test_tool_kdist_and_truth(z, tmp_path, capsys):
    X, eps, ms = case(z, "b")
    np.save(tmp_path / "x.npy", X)
    x, o = tmp_path / "x.npy", tmp_path / "o.npz"
    assert run_tool([x, o, "--backend", "numpy", "--kdist", "--min_samples", ms]) == 0
    w = np.load(o)
    kd = dbscan.kdistances(X, ms, backend="numpy")
    assert np.array_equal(w["kdist"], np.sort(kd)) and "labels" not in w.files and np.isnan(float(w["eps"]))
    out = capsys.readouterr().out
    assert all("%d %%" % q in out for q in (50, 75, 90, 95, 99))
    truth = (np.arange(len(X)) % 3).astype(np.int64)
    truth[z["labels_b"] >= 0] = z["labels_b"][z["labels_b"] >= 0] // 2
    np.save(tmp_path / "t.npy", truth)
    assert run_tool([x, o, "--backend", "numpy", "--eps", eps, "--min_samples", ms, "--truth", tmp_path / "t.npy", "--kdist"]) == 0
    w = np.load(o)
    lab = z["labels_b"]
    assert np.array_equal(w["labels"], lab) and int(w["n_clusters"]) == lab.max() + 1 and int(w["n_noise"]) == np.count_nonzero(lab < 0)
    assert {"core_mask", "counts", "n_rounds", "eps", "min_samples", "key", "backend", "kdist", "purity", "c_purity", "contingency"} <= set(w.files)
    assert float(w["eps"]) == eps and int(w["min_samples"]) == ms and str(w["backend"]) == "numpy"
    assert float(w["purity"]) == 1.0 and w["contingency"].sum() == np.count_nonzero(lab >= 0)          # noise is left out
    assert w["contingency"].shape == (4, 8) and float(w["c_purity"]) < 1.0
    lines = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("cluster") for ln in lines) == lab.max() + 1
    assert any(ln.startswith("noise: %d" % np.count_nonzero(lab < 0)) for ln in lines)
