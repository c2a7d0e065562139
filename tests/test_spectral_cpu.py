"""The spectral embedding's float64 numpy backend (cryo_ralib_amd/spectral.py), without a GPU: every pin of
tests/golden/spectral_ref.npz (the graph against sklearn's entry for entry; theta and the unit vectors against the dense
definition and against sklearn within Davis-Kahan's bound with the stored gap), the rules that have no pin (components, density
normalisation, breakdown at n_sub - 1, the constant column, diffusion time, clustering), the domain and the tool's exit statuses.

Bounds.  A unit vector y with residual r = |M y - theta y| has an eigenvalue within r of theta, and with the gap of that eigenvalue
to the rest of the spectrum sin(angle) <= r / gap, so |y - u| <= 2 r / gap; n 2^-52 covers the rounding of the two unit vectors.
Against sklearn both vectors are approximate, so both residuals are added."""
import warnings

import numpy as np
import pytest

import spectral_cases as sc
from cryo_ralib_amd import api, spectral

PINS = tuple(sc.pin_cases())


@pytest.fixture(scope="module")
def z():
    with np.load(sc.GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def cases():
    return sc.pin_cases()


@pytest.fixture(scope="module")
def graphs(cases):
    return {c: spectral.graph(X, backend="numpy", **sc.graph_options(opt)) for c, (X, opt, _) in cases.items()}


@pytest.fixture(scope="module")
def solved(cases):
    return {c: spectral.embedding(X, backend="numpy", **opt) for c, (X, opt, _) in cases.items()}


def test_pin_inputs_are_the_generators(z, cases):
    for c, (X, _, with_sklearn) in cases.items():
        if with_sklearn:
            assert np.array_equal(z["X_" + c], X), c
    assert np.array_equal(z["arcs_X"], sc.arcs(sc.ARCS["n"], sc.ARCS["seed"], sc.ARCS["noise"])[0])


@pytest.mark.parametrize("c", [c for c in PINS if sc.pin_cases()[c][2]])
def test_pin_graph_is_sklearns(z, graphs, c):
    indptr, indices, a, component = graphs[c]
    assert indptr.dtype == np.int32 and indices.dtype == np.int32 and a.dtype == np.float64 and component.dtype == np.int32
    assert np.array_equal(indptr, z["sk_indptr_" + c]) and np.array_equal(indices, z["sk_indices_" + c].astype(np.int32))
    assert np.array_equal(a, 0.5 * z["sk_twice_" + c].astype(np.float64))
    assert not component.any()


@pytest.mark.parametrize("c", PINS)
def test_pin_embedding(z, cases, graphs, solved, c):
    sc.check_against_pins(z, c, solved[c], graphs[c], cases[c][2])
    assert solved[c].residuals.max() <= 1e-9            # tol = 1e-10 on the estimate; the computed residual is of that size
    assert np.array_equal(solved[c].rows, np.arange(len(cases[c][0])))


def test_embedding_from_graph_is_embedding(cases, graphs, solved):
    X, opt, _ = cases["alpha1"]
    plain = spectral.graph(X, backend="numpy", n_neighbors=opt["n_neighbors"])
    res = spectral.embedding_from_graph(*plain[:3], n_components=opt["n_components"], alpha=1.0, backend="numpy")
    assert np.array_equal(res.embedding, solved["alpha1"].embedding) and np.array_equal(res.eigenvalues, solved["alpha1"].eigenvalues)
    norm = spectral.graph(X, backend="numpy", n_neighbors=opt["n_neighbors"], alpha=1.0)
    assert np.array_equal(norm[2], graphs["alpha1"][2]) and not np.array_equal(norm[2], plain[2])


def test_alpha_zero_is_alpha_omitted(cases):
    X, opt, _ = cases["gauss3"]
    a = spectral.embedding(X, backend="numpy", **opt)
    b = spectral.embedding(X, backend="numpy", alpha=0.0, **opt)
    c = spectral.embedding(X, backend="numpy", alpha=0, **opt)
    assert np.array_equal(a.embedding, b.embedding) and np.array_equal(a.embedding, c.embedding)
    assert np.array_equal(spectral.graph(X, backend="numpy")[2], spectral.graph(X, alpha=0.0, backend="numpy")[2])


def test_two_blobs_embed_the_larger_one_bitwise():
    X, first = sc.two_blobs(90, 150, 3, 7)
    with pytest.warns(spectral.SpectralWarning, match="Graph is not fully connected, spectral embedding may not work as expected.*90 rows"):
        res = spectral.embedding(X, 3, n_neighbors=8, backend="numpy")
    alone = spectral.embedding(X[~first], 3, n_neighbors=8, backend="numpy")
    assert res.n_dropped == 90 and np.array_equal(res.rows, np.nonzero(~first)[0])
    assert np.array_equal(res.embedding[~first], alone.embedding) and np.all(np.isnan(res.embedding[first]))
    assert np.array_equal(res.eigenvalues, alone.eigenvalues) and res.n_steps == alone.n_steps
    # numbered by lowest member
    want = np.where(first == first[0], 0, 1).astype(np.int32)
    assert np.array_equal(res.component, want)
    with pytest.raises(spectral.SpectralError, match="2 connected components"):
        spectral.embedding(X, 3, n_neighbors=8, on_disconnected="error", backend="numpy")
    # a tie of sizes goes to the lower number
    Xt, ft = sc.two_blobs(60, 60, 2, 8)
    with pytest.warns(spectral.SpectralWarning):
        tie = spectral.embedding(Xt, 2, n_neighbors=6, backend="numpy")
    assert np.array_equal(tie.rows, np.nonzero(tie.component == 0)[0]) and tie.component[0] == 0
    with pytest.raises(spectral.SpectralError, match="n_components \\+ 2"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spectral.embedding(Xt, 59, n_neighbors=6, max_steps=100, backend="numpy")


def test_components_numpy_on_small_graphs():
    for n in (3, 17, 300):
        ip, ix, _ = sc.path_graph(n)
        assert not spectral.components_numpy(ip, ix).any()
    ip, ix, _ = sc.edges_to_csr(9, [(0, 4), (4, 8), (1, 2), (5, 7), (7, 2)])
    assert spectral.components_numpy(ip, ix).tolist() == [0, 1, 1, 3, 0, 1, 6, 1, 0]
    assert spectral._number(spectral.components_numpy(ip, ix)).tolist() == [0, 1, 1, 2, 0, 1, 3, 1, 0]


def test_drop_first_false_has_the_constant_column(cases, graphs):
    X, opt, _ = cases["gauss3"]
    keep = spectral.embedding(X, 4, n_neighbors=10, drop_first=False, backend="numpy")
    drop = spectral.embedding(X, 3, n_neighbors=10, backend="numpy")
    indptr, indices, a, _ = graphs["gauss3"]
    assert keep.embedding.shape == (400, 4)
    assert np.array_equal(keep.embedding[:, 0], np.full(400, 1.0 / np.sqrt(np.sum(1.0 / sc.degree_scale(indptr, a) ** 2))))
    assert np.array_equal(keep.embedding[:, 1:], drop.embedding)
    assert keep.eigenvalues[0] == 1.0 and keep.residuals[0] == 0.0 and np.array_equal(keep.eigenvalues[1:], drop.eigenvalues)
    one = spectral.embedding(X, 1, n_neighbors=10, drop_first=False, backend="numpy")
    assert one.embedding.shape == (400, 1) and one.n_steps == 0 and np.array_equal(one.embedding[:, 0], keep.embedding[:, 0])


def test_sign_rule_and_diffusion_time(cases, solved):
    X, opt, _ = cases["gauss3"]
    E = solved["gauss3"].embedding
    top = np.argmax(np.abs(E), axis=0)
    assert np.all(E[top, np.arange(E.shape[1])] > 0)
    assert np.array_equal(spectral.sign_flip(np.array([[1.0, -2.0], [-3.0, 2.0], [3.0, 1.0]])), np.array([[-1.0, 2.0], [3.0, -2.0], [-3.0, -1.0]]))
    th = solved["gauss3"].eigenvalues
    for tau in (1.0, 2.5):
        D = spectral.embedding(X, diffusion_time=tau, backend="numpy", **opt)
        assert np.array_equal(D.embedding, E * th ** tau) and np.array_equal(D.eigenvalues, th)
    Z = spectral.embedding(X, diffusion_time=0, backend="numpy", **opt)
    assert np.array_equal(Z.embedding, E)
    # a negative theta is clamped: the path of 3 rows has the spectrum 1, 0, -1
    ip, ix, a = sc.path_graph(4)
    R = spectral.embedding_from_graph(ip, ix, a, 2, diffusion_time=1.0, backend="numpy")
    plain = spectral.embedding_from_graph(ip, ix, a, 2, backend="numpy")
    assert np.all(np.abs(R.embedding - plain.embedding * np.maximum(plain.eigenvalues, 0.0)) <= 1e-15)


def test_n_equals_three_breaks_down_at_n_sub_minus_one():
    X = np.array([[0.0, 0.0], [1.0, 0.25], [0.5, 2.0]], np.float32)
    res = spectral.embedding(X, 1, n_neighbors=3, backend="numpy")
    ip, ix, a, comp = spectral.graph(X, n_neighbors=3, backend="numpy")
    assert ix.tolist() == [1, 2, 0, 2, 0, 1] and not comp.any()
    # the triangle: M = (J - I) / 2 has the spectrum 1, -1/2, -1/2; the complement of q0 is its eigenspace
    assert res.converged and res.n_steps <= 2 and abs(res.eigenvalues[0] + 0.5) <= 4 * sc.EPS and res.residuals[0] <= 8 * sc.EPS
    assert abs(res.embedding[:, 0].sum()) <= 8 * sc.EPS
    # a weighted path of 5 rows: 4 distinct non-trivial eigenvalues, so the basis is complete at n_sub - 1 = 4 steps
    ip, ix, a = sc.weighted_path(5)
    res = spectral.embedding_from_graph(ip, ix, a, 3, backend="numpy")
    E, theta, _, _ = spectral.dense_numpy(ip, ix, a, 3)
    assert res.converged and res.n_steps <= 4 and np.all(np.abs(res.eigenvalues - theta) <= 8 * sc.EPS)
    assert np.all(np.abs(res.embedding - E) <= 64 * sc.EPS)


def test_max_steps_without_convergence_warns(cases):
    X, opt, _ = cases["gauss5"]
    with pytest.warns(spectral.SpectralWarning, match="did not reach tol"):
        res = spectral.embedding(X, 4, n_neighbors=15, max_steps=16, backend="numpy")
    assert not res.converged and res.n_steps == 16 and res.residuals.max() > 1e-10


def test_selftuning_weights(cases, graphs):
    from cryo_ralib_amd import tsne
    X, opt, _ = cases["selftune"]
    indptr, indices, a, _ = graphs["selftune"]
    idx, d2 = tsne.knn_numpy(X, 9)
    sigma = np.sqrt(d2[:, 6])
    i, p = 17, int(indptr[17])
    j = int(indices[p])
    w_ij = np.exp(-d2[i][idx[i] == j] / (sigma[i] * sigma[j])).sum()
    w_ji = np.exp(-d2[j][idx[j] == i] / (sigma[i] * sigma[j])).sum()
    assert abs(a[p] - 0.5 * (w_ij + w_ji)) <= 2 * sc.EPS and np.all((a > 0) & (a <= 1))
    dup = np.concatenate([X[:50], np.repeat(X[60:61], 9, axis=0)])
    with pytest.raises(spectral.SpectralError, match="row 50 has sigma = 0"):
        spectral.graph(dup, n_neighbors=10, affinity="gaussian", local_scale=7, backend="numpy")


def test_cluster_equals_the_pinned_partition(z):
    res = spectral.cluster(z["arcs_X"], 2, n_neighbors=sc.ARCS["n_neighbors"], backend="numpy")
    assert res.labels.dtype == np.int32 and sc.same_partition(res.labels, z["arcs_labels"])
    assert res.embedding.shape == (sc.ARCS["n"], 2) and len(np.unique(res.embedding[:, 0])) == 1
    X, first = sc.two_blobs(40, 80, 2, 9)
    with pytest.warns(spectral.SpectralWarning):
        part = spectral.cluster(X, 2, n_neighbors=6, backend="numpy")
    assert np.all(part.labels[first] == -1) and set(part.labels[~first]) == {0, 1}
    assert api.spectral_cluster is not None and api.spectral_embedding is not None and api.spectral_graph is not None


def test_dense_numpy_refuses_large_and_disconnected():
    ip, ix, a = sc.path_graph(4001)
    with pytest.raises(spectral.SpectralError, match="n <= 4000"):
        spectral.dense_numpy(ip, ix, a, 2)
    ip, ix, a = sc.edges_to_csr(6, [(0, 1), (1, 2), (3, 4), (4, 5)])
    with pytest.raises(spectral.SpectralError, match="connected"):
        spectral.dense_numpy(ip, ix, a, 2)


def test_domain_errors():
    X = sc.gaussian(40, 3, 0)
    bad = [
        lambda: spectral.embedding(X[:2], 1, n_neighbors=2, backend="numpy"),
        lambda: spectral.check_domain(262145, 3),
        lambda: spectral.check_domain(100, 2049),
        lambda: spectral.check_domain(100, 0),
        lambda: spectral.embedding(X, 2, n_neighbors=1, backend="numpy"),
        lambda: spectral.embedding(X, 2, n_neighbors=41, backend="numpy"),
        lambda: spectral.check_domain(1000, 3, n_neighbors=303),
        lambda: spectral.embedding(X, 2, n_neighbors=7.0, backend="numpy"),
        lambda: spectral.embedding(X, 0, backend="numpy"),
        lambda: spectral.embedding(X, 65, backend="numpy"),
        lambda: spectral.embedding(X, 2, affinity="rbf", backend="numpy"),
        lambda: spectral.embedding(X, 2, affinity="gaussian", local_scale=0, backend="numpy"),
        lambda: spectral.embedding(X, 2, affinity="gaussian", local_scale=15, backend="numpy"),
        lambda: spectral.embedding(X, 2, alpha=-0.1, backend="numpy"),
        lambda: spectral.embedding(X, 2, alpha=1.5, backend="numpy"),
        lambda: spectral.embedding(X, 2, alpha=float("nan"), backend="numpy"),
        lambda: spectral.embedding(X, 2, tol=0.0, backend="numpy"),
        lambda: spectral.embedding(X, 2, max_steps=2, backend="numpy"),
        lambda: spectral.embedding(X, 2, max_steps=4097, backend="numpy"),
        lambda: spectral.embedding(X, 2, diffusion_time=-1.0, backend="numpy"),
        lambda: spectral.embedding(X, 2, random_state=None, backend="numpy"),
        lambda: spectral.embedding(X, 2, on_disconnected="drop", backend="numpy"),
        lambda: spectral.embedding(X, 2, backend="cpu"),
        lambda: spectral.embedding(X[0], 2, backend="numpy"),
        lambda: spectral.embedding(np.where(np.arange(120).reshape(40, 3) == 5, np.nan, X), 2, backend="numpy"),
        lambda: spectral.cluster(X, 1, backend="numpy"),
        lambda: spectral.cluster(X, 65, backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 1, 2, 2], [1, 0], [1.0, 1.0, 1.0], backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 1, 2, 2], [1, 3], [1.0, 1.0], backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 1, 2, 3], [1, 0, 2], [1.0, 1.0, 1.0], backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 1, 2, 3], [1, 2, 0], [1.0, 1.0, 1.0], backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 2, 3, 4], [2, 1, 0, 0], [1.0, 1.0, 1.0, 1.0], backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 2, 3, 4], [1, 2, 0, 0], [1.0, 2.0, 1.0, 1.0], backend="numpy"),
        lambda: spectral.embedding_from_graph([0, 2, 3, 4], [1, 2, 0, 0], [1.0, -1.0, 1.0, -1.0], backend="numpy"),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(spectral.SpectralError):
            f()
            pytest.fail("case %d did not raise" % k)
    assert issubclass(spectral.SpectralError, ValueError)
    spectral.check_domain(262144, 2048, n_neighbors=302)
    spectral.check_domain(3, 1, n_neighbors=3)
    spectral.check_solver(64, max_steps=4096)


def test_tool_exit_statuses_and_keys(z, tmp_path, capsys):
    x, o = str(tmp_path / "x.npy"), str(tmp_path / "out.npz")
    np.save(x, z["X_gauss3"])
    usage = [
        [x, o, "--averages", "refs.npy", "--k", "3"],
        [x, o, "--truth", "t.npy"],
        [x, o, "--k", "3", "--averages", "refs.npy", "--stack", "s.npy"],
        [x, o, "--averages", "refs.npy", "--stack", "s.npy", "--params", "p.txt", "--ou", "20"],
        [x, o, "--n_components", "0"],
        [x, o, "--n_components", "65"],
        [x, o, "--n_neighbors", "1"],
        [x, o, "--alpha", "2"],
        [x, o, "--tol", "0"],
        [x, o, "--max_steps", "2"],
        [x, o, "--diffusion_time", "-1"],
        [x, o, "--affinity", "rbf"],
        [x, o, "--affinity", "gaussian", "--local_scale", "0"],
        [x, o, "--on_disconnected", "drop"],
        [x, o, "--k", "1"],
        [x, o, "--quality", "0"],
        [x, o, "--seed", "-1"],
    ]
    for argv in usage:
        with pytest.raises(SystemExit) as e:
            spectral.main(argv + ["--backend", "numpy"])
        assert e.value.code == 2, argv
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        spectral.main([x, o, "--backend", "numpy", "--n_neighbors", "401"])
    assert e.value.code != 2 and "n_neighbors" in str(e.value.code)
    assert spectral.main([x, o, "--backend", "numpy", "--n_components", "5", "--n_neighbors", "10"]) == 0
    with np.load(o) as f:
        for key in ("embedding", "eigenvalues", "laplacian_eigenvalues", "residuals", "component", "n_steps", "converged", "n_dropped",
                    "n_components", "n_neighbors", "affinity", "local_scale", "alpha", "diffusion_time", "tol", "max_steps", "seed",
                    "on_disconnected", "key", "backend"):
            assert key in f.files, key
        assert "labels" not in f.files and f["embedding"].shape == (400, 5) and bool(f["converged"])
        direct = spectral.embedding(z["X_gauss3"], 5, n_neighbors=10, backend="numpy")
        assert np.array_equal(f["embedding"], direct.embedding)
    truth = str(tmp_path / "truth.npy")
    np.save(truth, (np.arange(400) % 3).astype(np.int64))
    assert spectral.main([x, o, "--backend", "numpy", "--n_neighbors", "10", "--k", "3", "--truth", truth, "--quality", "5"]) == 0
    with np.load(o) as f:
        assert f["labels"].shape == (400,) and f["centers"].shape == (3, 3) and "inertia" in f.files and "purity" in f.files
        assert 0.0 < float(f["trustworthiness"]) <= 1.0 and 0.0 < float(f["continuity"]) <= 1.0
    # the kmeans tool reads the file with --key embedding
    from cryo_ralib_amd import kmeans
    assert kmeans.read_input(o, "embedding").shape == (400, 2)
