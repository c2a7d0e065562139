"""HDBSCAN's float64 numpy backend and the host tree (cryo_ralib_amd/hdbscan.py), without a GPU: every scikit-learn 1.7.2 pin of
tests/golden/hdbscan_ref.npz, rule 5's tree against a literal Kruskal, row-permutation invariance, hand-built hierarchies for the
multi-way merge, the min_cluster_size threshold, duplicates, identical points, the numbering, the "eom" tie, the host side of a
Boruvka round, the domain and the tool's exit statuses.

The hand-built cases are one-dimensional with min_samples = 1 (core distance 0, so w is the plain distance) on multiples of 1/8:
every lambda is a power of two or a small multiple and every stability is exact."""
import os

import numpy as np
import pytest

from cryo_ralib_amd import api, hdbscan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan_ref.npz")


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def case(z, c):
    ms = int(z["min_samples_" + c])
    return z["X_" + c], int(z["min_cluster_size_" + c]), None if ms < 0 else ms, str(z["method_" + c])


def same_partition(a, b):
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def line(*xs):
    return np.array(xs, np.float32)[:, None]


def run(X, mcs, ms=1, method="eom"):
    return hdbscan.hdbscan(np.asarray(X, np.float32), mcs, ms, method, backend="numpy")


CASES = "abcdefghi"


def test_pins_cover_the_issue_cases(z):
    assert "".join(z["cases"].tolist()) == CASES
    shapes = {c: (len(z["X_" + c]),) + case(z, c)[1:] for c in CASES}
    assert shapes == {"a": (600, 15, 5, "eom"), "b": (1500, 25, 10, "eom"), "c": (500, 10, None, "eom"), "d": (130, 5, 5, "eom"),
                      "e": (700, 20, 5, "eom"), "f": (1200, 10, 3, "eom"), "g": (65, 5, 3, "eom"), "h": (300, 10, 1, "eom"),
                      "i": (600, 15, 5, "leaf")}
    for c in CASES:
        X = z["X_" + c]
        assert X.dtype == np.float32 and np.all(np.abs(X) <= 16) and np.array_equal(X * 1024, np.round(X * 1024))
        assert z["tie_mask_" + c].sum() <= 0.03 * len(X)
    assert any(z["tie_mask_" + c].any() for c in CASES)


@pytest.mark.parametrize("c", CASES)
def test_checker_equals_the_pins_and_sklearn_outside_the_tie_set(z, c):
    X, mcs, ms, method = case(z, c)
    r = run(X, mcs, ms, method)
    assert r.labels.dtype == np.int32 and r.probabilities.dtype == np.float64 and r.tie_mask.dtype == np.bool_
    assert np.array_equal(r.labels, z["labels_" + c]) and np.array_equal(r.probabilities, z["probabilities_" + c])
    assert np.array_equal(r.tie_mask, z["tie_mask_" + c])
    T = r.tie_mask
    bound = max(1000 * float(z["discrepancy_" + c]), 1e-12)
    for alg in ("brute", "kd"):
        assert same_partition(r.labels[~T], z["sk_labels_%s_%s" % (alg, c)][~T])
        assert np.abs(r.probabilities - z["sk_prob_%s_%s" % (alg, c)])[~T].max() <= bound
    n = len(X)
    lo, hi, dist = r.mst
    assert len(lo) == n - 1 and np.all(lo < hi) and np.all(np.diff(dist) >= 0)
    assert r.n_clusters == r.labels.max() + 1 == len(r.stabilities) and np.all(r.probabilities[r.labels < 0] == 0)
    assert np.all((r.probabilities[r.labels >= 0] > 0) & (r.probabilities <= 1)[r.labels >= 0])
    par, child, lam, size = r.condensed
    assert np.array_equal(np.sort(child[child < n]), np.arange(n)) and par.min() == n and np.all(size[child < n] == 1)


def test_core_distances_are_dbscan_kdistances(z):
    from cryo_ralib_amd import dbscan
    for c in "adh":
        X, mcs, ms, _ = case(z, c)
        assert np.array_equal(run(X, mcs, ms).core_distances, dbscan.kdistances(X, mcs if ms is None else ms, backend="numpy"))


@pytest.mark.parametrize("c", "dg")
def test_tree_is_kruskal_over_the_total_order(z, c):
    """rule 5 literally: all n (n - 1) / 2 edges sorted by (w2, lo, hi), taken when they join two components"""
    X, mcs, ms, _ = case(z, c)
    n = len(X)
    Xd = X.astype(np.float64)
    D2 = np.zeros((n, n))
    for t in range(X.shape[1]):
        df = Xd[:, t, None] - Xd[None, :, t]
        D2 += df * df
    core2 = np.sort(D2, axis=1)[:, ms - 1]
    assert np.array_equal(core2, hdbscan.core2_numpy(X, ms))
    lo, hi = np.triu_indices(n, 1)
    w2 = np.maximum(np.maximum(core2[lo], core2[hi]), D2[lo, hi])
    uf = list(range(n))

    def find(a):
        while uf[a] != a:
            a = uf[a]
        return a
    want = []
    for e in np.lexsort((hi, lo, w2)):
        a, b = find(lo[e]), find(hi[e])
        if a != b:
            uf[a] = b
            want.append((lo[e], hi[e], w2[e]))
    glo, ghi, gw2 = hdbscan.mst_numpy(X, core2)
    assert [(a, b, w) for a, b, w in zip(glo, ghi, gw2)] == want
    assert len(np.unique(gw2)) < n - 1          # the pins do hold equal weights


def test_row_permutation_invariance(z):
    X, mcs, ms, method = case(z, "c")
    r = run(X, mcs, ms, method)
    assert r.tie_mask.sum() > 0
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(X))
        q = run(X[perm], mcs, ms, method)
        assert np.array_equal(q.tie_mask, r.tie_mask[perm]) and np.array_equal(q.probabilities, r.probabilities[perm])
        assert same_partition(q.labels, r.labels[perm]) and q.n_clusters == r.n_clusters
        assert np.array_equal(np.sort(q.stabilities), np.sort(r.stabilities))
        assert np.array_equal(q.mst[2], r.mst[2]) and np.array_equal(q.core_distances, r.core_distances[perm])


def test_three_way_merge_at_equal_weight():
    """two blobs of four and one bridge point 3 away from each: one level node with three children; the bridge is in T, in neither
    blob, and stays so however the rows are ordered"""
    X = line(0, 1, 2, 3, 6, 9, 10, 11, 12)
    r = run(X, 3)
    assert r.labels.tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1] and r.tie_mask.tolist() == [False] * 4 + [True] + [False] * 4
    assert r.probabilities.tolist() == [1.0] * 4 + [0.0] + [1.0] * 4
    assert np.array_equal(r.mst[2], [1.0] * 6 + [3.0] * 2)
    assert np.array_equal(r.stabilities, [(1.0 - 1.0 / 3.0) * 4] * 2)
    par, child, lam, size = r.condensed
    n = len(X)
    assert sorted(zip(par[child >= n].tolist(), lam[child >= n].tolist(), size[child >= n].tolist())) == [(n, 1.0 / 3.0, 4)] * 2
    assert par[child == 4].tolist() == [n] and lam[child == 4].tolist() == [1.0 / 3.0]
    for order in ([4, 0, 1, 2, 3, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1, 0], [5, 0, 6, 1, 4, 7, 2, 8, 3]):
        q = run(X[order], 3)
        assert q.tie_mask.tolist() == [i == 4 for i in order] and [q.labels[order.index(4)]] == [-1]
        assert same_partition(q.labels, r.labels[order])


def threshold_case(k):
    return line(*([0, 1, 2, 3, 4] + [9, 10, 11, 12, 13] + [16 + i for i in range(k)]))


def test_child_of_exactly_min_cluster_size_minus_one_and_min_cluster_size():
    """A = 5 points, B = 5 points 5 away, S = k points 3 away from B, min_cluster_size = 4"""
    r = run(threshold_case(3), 4)                   # S leaves B's cluster at lambda 1 / 3 and keeps its label
    assert r.labels.tolist() == [0] * 5 + [1] * 8 and r.n_clusters == 2 and not r.tie_mask.any()
    assert r.probabilities.tolist() == [1.0] * 10 + [1.0 / 3.0] * 3
    assert np.allclose(r.stabilities, [(1 - 0.2) * 5, (1 - 0.2) * 5 + (1.0 / 3.0 - 0.2) * 3], rtol=1e-14, atol=0)    # 1/3 and 1/5 round
    r = run(threshold_case(4), 4)                   # a true split: (1 - 1/3) 9 > (1/3 - 1/5) 9
    assert r.labels.tolist() == [0] * 5 + [1] * 5 + [2] * 4 and r.n_clusters == 3 and not r.tie_mask.any()
    assert np.all(r.probabilities == 1.0)
    r = run(threshold_case(4), 4, method="leaf")
    assert r.labels.tolist() == [0] * 5 + [1] * 5 + [2] * 4
    r = run(threshold_case(3), 4, method="leaf")
    assert r.labels.tolist() == [0] * 5 + [1] * 8


def test_duplicates():
    """two piles of five equal points: w = 0 inside a pile, lambda = inf, probability 1, and no cluster born at inf"""
    X = line(*([0.0] * 5 + [10.0] * 5))
    r = run(X, 3)
    assert r.labels.tolist() == [0] * 5 + [1] * 5 and np.all(r.probabilities == 1.0) and not r.tie_mask.any()
    assert np.array_equal(r.mst[2], [0.0] * 8 + [10.0]) and np.all(np.isinf(r.stabilities))
    par, child, lam, size = r.condensed
    assert np.all(np.isinf(lam[child < 10])) and np.all(lam[child >= 10] == 0.1)
    # piles of two below min_cluster_size 3: the pile is a child smaller than min_cluster_size, and leaves as noise
    r = run(line(0, 0, 10, 10, 20, 20), 3)
    assert np.all(r.labels == -1) and np.all(r.probabilities == 0)


def test_all_points_identical():
    n = 70
    r = run(np.full((n, 3), 1.25, np.float32), 5, 5)
    assert np.all(r.labels == -1) and np.all(r.probabilities == 0) and r.n_clusters == 0 and not r.tie_mask.any()
    assert np.array_equal(r.mst[0], np.zeros(n - 1)) and np.array_equal(r.mst[1], np.arange(1, n)) and np.all(r.mst[2] == 0)
    assert np.all(r.core_distances == 0) and len(r.stabilities) == 0
    assert np.all(run(np.full((n, 3), 1.25, np.float32), 5, 5, "leaf").labels == -1)


def test_numbering_by_lowest_member_index():
    X = line(9, 0, 10, 1, 11, 2, 12, 3, 20, 21, 22, 23)
    r = run(X, 3)
    assert r.labels.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2]
    r = run(X[::-1].copy(), 3)
    assert r.labels.tolist() == [0, 0, 0, 0, 1, 2, 1, 2, 1, 2, 1, 2]


def test_eom_tie_keeps_the_parent():
    """C1 and C2 (6 points at spacing 1/2, 1 apart), S (4 points, 2 away) and Q (6 points, 8 away).  P = C1 + C2 + S is born at
    lambda 1/8, sheds S at 1/2 and splits at 1: stability 4 (1/2 - 1/8) + 12 (1 - 1/8) = 12; C1 and C2 have 6 (2 - 1) each.
    12 > 12 is false: the parent stays"""
    c1 = [0.5 * i for i in range(6)]
    c2 = [3.5 + 0.5 * i for i in range(6)]
    s = [8 + 0.5 * i for i in range(4)]
    q = [17.5 + 0.5 * i for i in range(6)]
    r = run(line(*(c1 + c2 + s + q)), 5)
    assert r.labels.tolist() == [0] * 16 + [1] * 6 and np.array_equal(r.stabilities, [12.0, (2 - 0.125) * 6])
    assert r.probabilities.tolist() == [1.0] * 12 + [0.5] * 4 + [1.0] * 6 and not r.tie_mask.any()
    # one more point in C2 tips the sum: 6 + 7 > 4 (3 / 8) + 13 (7 / 8) = 12.875
    r = run(line(*(c1 + c2 + [6.5] + [x + 0.5 for x in s] + [x + 0.5 for x in q])), 5)
    assert r.labels.tolist() == [0] * 6 + [1] * 7 + [-1] * 4 + [2] * 6
    assert run(line(*(c1 + c2 + s + q)), 5, method="leaf").labels.tolist() == [0] * 6 + [1] * 6 + [-1] * 4 + [2] * 6


def test_host_side_of_a_round():
    """boruvka_merge: roots' entries -> new components by lowest index and the new edges, a mutual choice once"""
    comp = np.array([0, 0, 2, 3, 3, 5])
    inf = np.inf
    w2 = np.array([4.0, inf, 4.0, 1.0, inf, 1.0])
    lo = np.array([1, -1, 1, 4, -1, 4])
    hi = np.array([2, -1, 2, 5, -1, 5])
    new, elo, ehi, ew = hdbscan.boruvka_merge(comp, w2, lo, hi)
    assert new.tolist() == [0, 0, 0, 3, 3, 3] and list(zip(elo.tolist(), ehi.tolist(), ew.tolist())) == [(1, 2, 4.0), (4, 5, 1.0)]
    one = np.zeros(4, np.int64)
    new, elo, ehi, ew = hdbscan.boruvka_merge(one, np.full(4, inf), np.full(4, -1), np.full(4, -1))
    assert new.tolist() == [0] * 4 and len(elo) == 0
    with pytest.raises(RuntimeError):
        hdbscan.boruvka_merge(comp, np.full(6, inf), np.full(6, -1), np.full(6, -1))
    with pytest.raises(RuntimeError):
        hdbscan.boruvka_merge(comp, w2, lo, np.array([2, -1, 2, 9, -1, 5]))


def test_deepest_dendrogram():
    """a chain of 20 000 points at growing gaps: every merge adds one point, the dendrogram is n - 1 deep, and the pointer
    jumping still ends; every point leaves the root one by one and all is noise"""
    n = 20000
    lo, hi = np.arange(n - 1), np.arange(1, n)
    labels, prob, tie, cond, stab = hdbscan.tree_from_mst(n, lo, hi, np.arange(1, n, dtype=np.float64) ** 2, 5)
    assert np.all(labels == -1) and len(cond[0]) == n and not tie.any()


def test_domain_errors():
    X = np.zeros((10, 2), np.float32)
    bad = [dict(min_cluster_size=1), dict(min_cluster_size=11), dict(min_cluster_size=2.0), dict(min_cluster_size=True),
           dict(min_samples=0), dict(min_samples=11), dict(min_samples=2.5), dict(cluster_selection_method="dbscan"),
           dict(backend="cuda")]
    for kw in bad:
        with pytest.raises(hdbscan.HdbscanError):
            hdbscan.hdbscan(X, **{"backend": "numpy", **kw})
    for Xb in (np.zeros((1, 2), np.float32), np.zeros((10, 0), np.float32), np.zeros(10, np.float32), np.zeros((3, 2049), np.float32)):
        with pytest.raises(hdbscan.HdbscanError):
            hdbscan.hdbscan(Xb, 2, backend="numpy")
    Xn = X.copy()
    Xn[3, 1] = np.inf
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(Xn, 2, backend="numpy")
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.check_domain(262145, 2)
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.check_domain(1000, 2, 5, 303)
    assert hdbscan.check_domain(1000, 2, 400, 302) == 302 and hdbscan.check_domain(262144, 2048, 7) == 7
    assert issubclass(hdbscan.HdbscanError, ValueError)
    assert {"ra_hdbscan_core", "ra_hdbscan_round"} <= set(api.EXPORTED_SYMBOLS)
    assert np.array_equal(api.hdbscan(line(0, 1, 2, 3, 6, 9, 10, 11, 12), min_cluster_size=3, min_samples=1, backend="numpy").labels,
                          [0, 0, 0, 0, -1, 1, 1, 1, 1])


def test_tool_exit_statuses(z, tmp_path, capsys):
    X = z["X_d"]
    np.save(tmp_path / "x.npy", X)
    x, o = str(tmp_path / "x.npy"), str(tmp_path / "o.npz")
    bad = [[x, o, "--min_cluster_size", "1"], [x, o, "--min_cluster_size", "131"], [x, o, "--min_samples", "0"],
           [x, o, "--min_samples", "303"], [x, o, "--min_samples", "131"], [x, o, "--method", "dbscan"],
           [x, o, "--min_proba", "0"], [x, o, "--min_proba", "1.5"], [x, o, "--min_proba", "nan"],
           [x, o, "--averages", str(tmp_path / "a.npy")], [x, o, "--averages", str(tmp_path / "a.npy"), "--stack", x, "--ou", "12"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            hdbscan.main(argv + ["--backend", "numpy"])
        assert e.value.code == 2, argv
        assert not os.path.exists(o)
    capsys.readouterr()
    assert hdbscan.main([x, o, "--backend", "numpy", "--min_cluster_size", "5", "--min_samples", "5", "--min_proba", "0.5"]) == 0
    f = np.load(o)
    assert np.array_equal(f["labels"], z["labels_d"]) and np.array_equal(f["probabilities"], z["probabilities_d"])
    assert np.array_equal(f["tie_mask"], z["tie_mask_d"]) and np.array_equal(f["keep"], z["probabilities_d"] >= 0.5)
    assert int(f["n_clusters"]) == z["labels_d"].max() + 1 and str(f["backend"]) == "numpy" and int(f["n_rounds"]) == 0
    assert f["mst_lo"].shape == (len(X) - 1,) and len(f["condensed_parent"]) == len(f["condensed_lambda"])
    lines = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("cluster") for ln in lines) == int(f["n_clusters"]) and any(ln.startswith("noise: ") for ln in lines)
    assert all("stability" in ln and "median probability" in ln for ln in lines if ln.startswith("cluster"))
