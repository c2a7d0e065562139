"""cryo_ralib_amd.quality without a GPU: the float64 numpy backend against the scikit-learn 1.7.2 pins of
tests/golden/quality_ref.npz and against sklearn itself on fresh tie-free data, rule 2 on hand-built ties, the scores' identities,
the co-ranking curve against a brute-force set intersection, the sample, every domain error and every usage error of both tools."""
import os

import numpy as np
import pytest

from cryo_ralib_amd import api, quality, tsne

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_ref.npz")


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("c", "abcd")
def test_checker_equals_the_pins(z, c):
    X, Y, k = z["X_" + c], z["Y_" + c], int(z["k_" + c])
    t = quality.trustworthiness(X, Y, k, backend="numpy", details=True)
    cc = quality.continuity(X, Y, k, backend="numpy", details=True)
    assert np.array_equal(t.ranks, z["rank_t_" + c]) and np.array_equal(cc.ranks, z["rank_c_" + c])
    assert abs(t.score - float(z["T_" + c])) <= 1e-12 and abs(cc.score - float(z["C_" + c])) <= 1e-12
    assert t.ranks.dtype == np.int32 and t.ranks.min() >= 1 and t.ranks.max() <= X.shape[0] - 1


def test_pins_hold_the_cases_the_fixture_promises(z):
    shapes = {c: (z["X_" + c].shape[0], z["X_" + c].shape[1], int(z["k_" + c])) for c in "abcd"}
    assert {(300, 8, 10), (257, 50, 31), (130, 3, 64)} <= set(shapes.values())
    assert z["X_d"].shape[1] == 1 and z["Y_d"].shape[1] == 2
    for c in "abcd":
        for A in (z["X_" + c], z["Y_" + c]):
            assert np.array_equal(A * 1024, np.round(A * 1024))


@pytest.mark.parametrize("n, d, k", [(50, 2, 5), (120, 7, 12), (300, 50, 64)])
def test_checker_equals_sklearn_on_fresh_data(n, d, k):
    sk = pytest.importorskip("sklearn.manifold")
    rng = np.random.default_rng(n + d + k)
    X = rng.normal(size=(n, d)).astype(np.float32)              # continuous: no exact ties
    Y = (X[:, :2] + 0.3 * rng.normal(size=(n, 2))).astype(np.float32)
    T, C = quality.trustworthiness(X, Y, k, backend="numpy"), quality.continuity(X, Y, k, backend="numpy")
    assert abs(T - sk.trustworthiness(X.astype(np.float64), Y.astype(np.float64), n_neighbors=k)) <= 1e-12
    assert abs(C - sk.trustworthiness(Y.astype(np.float64), X.astype(np.float64), n_neighbors=k)) <= 1e-12


def brute_rank(A, i, j):
    A = np.asarray(A, np.float64)
    d2 = lambda a, b: float(sum((A[a, t] - A[b, t]) ** 2 for t in range(A.shape[1])))      # noqa: E731
    return 1 + sum(1 for l in range(A.shape[0]) if l != i and (d2(i, l), l) < (d2(i, j), j))


def test_rule_2_on_hand_built_ties():
    A = np.array([[0, 0], [1, 0], [0, 0], [-1, 0], [0, 1], [0, 0], [3, 3]], np.float32)          # rows 0, 2, 5 are equal
    n = A.shape[0]
    idx = np.array([[2, 5, 1, 3, 4, 6, 2, -1, n, 0]] + [[(i + s) % n for s in range(1, 8)] + [i, -1, n] for i in range(1, n)])
    R = quality.neighbor_ranks(A, idx, backend="numpy")
    for i in range(n):
        for t, j in enumerate(idx[i]):
            assert R[i, t] == (0 if j < 0 or j >= n or j == i else brute_rank(A, i, j)), (i, t)
    assert list(R[0]) == [1, 2, 3, 4, 5, 6, 1, 0, 0, 0]          # duplicates first by index; equal distances by index; repeat equal
    E = np.ones((5, 3), np.float32)                              # all points equal: the order is the index order
    RE = quality.neighbor_ranks(E, np.tile(np.arange(5), (5, 1)), backend="numpy")
    assert np.array_equal(RE, np.array([[0, 1, 2, 3, 4], [1, 0, 2, 3, 4], [1, 2, 0, 3, 4], [1, 2, 3, 0, 4], [1, 2, 3, 4, 0]]))
    assert np.array_equal(quality.knn_numpy(E, 2), np.array([[1, 2], [0, 2], [0, 1], [0, 1], [0, 1]]))
    assert quality.trustworthiness(E, E, 2, backend="numpy") == 1.0


def test_scores_and_curve_identities(z):
    X, Y, k = z["X_a"], z["Y_a"], 10
    n = X.shape[0]
    r = quality.embedding_quality(X, Y, k, backend="numpy")
    t = quality.trustworthiness(X, Y, k, backend="numpy", details=True)
    assert r.trustworthiness == t.score and np.array_equal(r.trust_point, t.point) and r.sample_indices is None
    assert abs(r.trustworthiness - r.trust_point.mean()) <= 1e-14 and abs(r.continuity - r.cont_point.mean()) <= 1e-14
    pen = quality.penalties(t.ranks, k)
    assert pen.dtype == np.int64 and np.array_equal(r.trust_point, 1.0 - pen * (2.0 / (k * (2.0 * n - 3.0 * k - 1.0))))
    nx, ny = quality.knn_numpy(X, n - 1), t.neighbors
    for K in range(1, k + 1):                                    # Q_NX(K): shared K-neighbourhoods (tie-free data)
        shared = sum(len(set(nx[i, :K]) & set(ny[i, :K])) for i in range(n))
        assert r.qnx[K - 1] == shared / (n * float(K))
    assert np.array_equal(r.lcmc, r.qnx - np.arange(1, k + 1) / (n - 1.0)) and r.k_best == int(np.argmax(r.lcmc)) + 1
    q, l, kb = quality.coranking(np.array([[1, 2], [1, 0], [2, 1]]))         # one invalid entry; K = 1: 2 hits, K = 2: 5 hits
    assert np.array_equal(q, [2 / 3.0, 5 / 6.0]) and np.array_equal(l, q - np.array([1, 2]) / 2.0) and kb == 1


def test_sample_indices_and_nan_outside(z):
    X, Y = z["X_a"], z["Y_a"]
    r = quality.embedding_quality(X, Y, 6, sample_size=100, random_state=3, backend="numpy")
    s = np.sort(np.random.RandomState(3).permutation(300)[:100])
    assert np.array_equal(r.sample_indices, s) and np.array_equal(quality.draw_sample(300, 100, 3), s)
    g = quality.embedding_quality(X[s], Y[s], 6, backend="numpy")
    assert r.trustworthiness == g.trustworthiness and np.array_equal(r.trust_point[s], g.trust_point)
    assert np.all(np.isnan(np.delete(r.trust_point, s))) and np.all(np.isnan(np.delete(r.cont_point, s)))
    big = np.zeros((quality.MAX_N + 1, 1), np.float32)
    with pytest.raises(quality.QualityError, match="need 3 <= n <= 262144"):
        quality.embedding_quality(big, big, 5, backend="numpy")
    with pytest.raises(quality.QualityError, match="sample_size"):
        quality.embedding_quality(X, Y, 5, sample_size=301, backend="numpy")


def blobs():
    """the recovery case of tests/test_gpu_quality.py"""
    rng = np.random.default_rng(600)
    centres = np.zeros((3, 10))
    centres[:, :2] = 40.0 * np.array([[1.0, 0.0], [-0.5, 0.75 ** 0.5], [-0.5, -0.75 ** 0.5]])
    lab = np.repeat(np.arange(3), 200)
    X = (centres[lab] + rng.normal(size=(600, 10))).astype(np.float32)
    Y = X[:, :2].copy()
    moved = np.sort(rng.permutation(600)[:30])
    Y[moved] = (centres[(lab[moved] + 1) % 3, :2] + rng.normal(size=(30, 2))).astype(np.float32)
    return X, Y, moved


def test_recovery_of_misplaced_points():
    X, Y, moved = blobs()
    r = quality.embedding_quality(X, Y, 10, backend="numpy")
    assert np.array_equal(np.sort(np.argsort(r.trust_point, kind="stable")[:30]), moved)
    assert r.trust_point[moved].max() < np.delete(r.trust_point, moved).min()


def test_domain_errors():
    X, Y = np.zeros((20, 3), np.float32), np.zeros((20, 2), np.float32)
    bad = [((X[:2], Y[:2], 1), "need 3 <= n"), ((X, Y[:19], 5), "X has 20 rows, Y 19"), ((X, Y, 10), r"n_neighbors \(10\) should be less than"),
           ((X, Y, 0), "need 1 <= n_neighbors <= 301"), ((X, Y, 2.0), "must be an integer"),
           ((np.zeros((20, 0), np.float32), Y, 5), "features in X"), ((X, np.zeros((20, 2049), np.float32), 5), "features in Y"),
           ((X, np.zeros(20, np.float32), 5), r"\[n\]\[d\]")]
    for fn in (quality.trustworthiness, quality.continuity, quality.embedding_quality):
        for args, msg in bad:
            with pytest.raises(quality.QualityError, match=msg):
                fn(*args, backend="numpy")
    Z = np.zeros((700, 1), np.float32)
    with pytest.raises(quality.QualityError, match="need 1 <= n_neighbors <= 301"):
        quality.trustworthiness(Z, Z, 302, backend="numpy")
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(quality.QualityError, match="NaN or infinite"):
        quality.trustworthiness(Xn, Y, 5, backend="numpy")
    with pytest.raises(quality.QualityError, match="NaN or infinite"):
        quality.continuity(X, Y + np.inf, 5, backend="numpy")
    with pytest.raises(quality.QualityError, match="backend is"):
        quality.trustworthiness(X, Y, 5, backend="cuda")
    with pytest.raises(quality.QualityError, match="integer array"):
        quality.neighbor_ranks(X, np.zeros((20, 2)), backend="numpy")
    with pytest.raises(quality.QualityError, match="integer array"):
        quality.neighbor_ranks(X, np.zeros((19, 2), np.int64), backend="numpy")
    with pytest.raises(quality.QualityError, match="list entries"):
        quality.neighbor_ranks(X, np.zeros((20, 302), np.int64), backend="numpy")
    assert issubclass(quality.QualityError, ValueError)
    try:
        quality.trustworthiness(X, Y, 10, backend="numpy")
    except ValueError as e:
        assert str(e) == "n_neighbors (10) should be less than n_samples / 2 (10.0)"         # sklearn's message


def test_api_reexports_and_the_old_restatement_stays(z):
    X, Y = z["X_d"], z["Y_d"]
    assert api.trustworthiness(X, Y, n_neighbors=5, backend="numpy") == quality.trustworthiness(X, Y, 5, backend="numpy")
    assert api.continuity(X, Y, n_neighbors=5, backend="numpy") == quality.continuity(X, Y, 5, backend="numpy")
    assert api.embedding_quality(X, Y, n_neighbors=5, backend="numpy").k_best >= 1
    assert np.array_equal(api.neighbor_ranks(X, z["rank_t_d"] * 0 + 1, backend="numpy")[1:, 0], quality.ranks_numpy(X, np.ones((60, 1)))[1:, 0])
    assert "ra_embed_ranks" in api.EXPORTED_SYMBOLS
    assert abs(tsne.trustworthiness(X, Y, 5) - float(z["T_d"])) <= 1e-12


def usage(fn, argv, capsys, text):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_tool_and_its_usage_errors(z, tmp_path, capsys):
    X, Y = z["X_c"], z["Y_c"]
    hi, lo, out = str(tmp_path / "x.npy"), str(tmp_path / "y.npz"), str(tmp_path / "q.npz")
    np.save(hi, X)
    np.savez(lo, embedding=Y)
    np.save(tmp_path / "short.npy", Y[:100])
    np.save(tmp_path / "huge.npy", np.zeros((quality.MAX_N + 1, 1), np.float32))
    assert quality.main([hi, lo, out, "--k", "7", "--backend", "numpy", "--worst", "4", "--sample_size", "90", "--seed", "2"]) == 0
    text = capsys.readouterr().out
    o = np.load(out)
    ref = quality.embedding_quality(X, Y, 7, 90, 2, backend="numpy")
    assert float(o["trustworthiness"]) == ref.trustworthiness and float(o["continuity"]) == ref.continuity
    assert np.array_equal(o["sample_indices"], ref.sample_indices) and np.array_equal(o["trust_point"], ref.trust_point, equal_nan=True)
    assert np.array_equal(o["lcmc"], ref.lcmc) and int(o["k_best"]) == ref.k_best and int(o["k"]) == 7 and int(o["seed"]) == 2
    assert text.count("row ") == 4 and "k_best" in text
    usage(quality.main, [hi, str(tmp_path / "short.npy"), out, "--backend", "numpy"], capsys, "differ in rows")
    usage(quality.main, [hi, lo, out, "--k", "65"], capsys, "K < n / 2")
    usage(quality.main, [hi, lo, out, "--k", "45", "--sample_size", "90"], capsys, "K < n / 2")
    usage(quality.main, [str(tmp_path / "huge.npy"), str(tmp_path / "huge.npy"), out], capsys, "need a sample size")
    usage(quality.main, [hi, lo, out, "--sample_size", "131"], capsys, "sample size")
    usage(quality.main, [hi, lo, out, "--seed", "1"], capsys, "--seed goes with --sample_size")
    with pytest.raises(SystemExit, match="has no array 'factors'"):
        quality.main([lo, lo, out, "--backend", "numpy"])


def test_tsne_tool_quality_option(z, tmp_path, capsys):
    X = z["X_c"]
    src = str(tmp_path / "x.npy")
    np.save(src, X)
    np.save(tmp_path / "huge.npy", np.zeros((quality.MAX_N + 1, 2), np.float32))
    common = ["--backend", "numpy", "--max_iter", "250", "--perplexity", "10"]
    usage(tsne.main, [src, str(tmp_path / "o.npz"), "--quality_sample", "50"] + common, capsys, "--quality_sample needs --quality")
    usage(tsne.main, [src, str(tmp_path / "o.npz"), "--quality", "65"] + common, capsys, "K < n / 2")
    usage(tsne.main, [str(tmp_path / "huge.npy"), str(tmp_path / "o.npz"), "--quality", "--fit_size", "100"] + common, capsys,
          "need a sample size")
    assert tsne.main([src, str(tmp_path / "t0.npz")] + common) == 0
    assert tsne.main([src, str(tmp_path / "t1.npz"), "--quality", "--quality_sample", "80", "--seed", "4", "--init", "random"] + common) == 0
    t0, t1 = np.load(tmp_path / "t0.npz"), np.load(tmp_path / "t1.npz")
    assert sorted(t0.files) == sorted(["embedding", "kl_divergence", "n_iter", "errors", "perplexity", "early_exaggeration",
                                       "learning_rate", "max_iter", "init", "seed", "backend"])
    assert set(t1.files) - set(t0.files) == {"trustworthiness", "continuity", "trust_point", "cont_point", "quality_sample_indices"}
    q = quality.embedding_quality(X, t1["embedding"], 10, 80, 4, backend="numpy")
    assert float(t1["trustworthiness"]) == q.trustworthiness and np.array_equal(t1["trust_point"], q.trust_point, equal_nan=True)
    assert np.array_equal(t1["quality_sample_indices"], q.sample_indices)
