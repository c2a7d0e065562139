"""t-SNE without a GPU: the numpy backend (the CPU checker) against scikit-learn 1.7's values (tests/golden/tsne_ref.npz, made
by tests/golden/make_tsne_pins.py), the optimiser's schedule and stopping rules, the random init, trustworthiness, the domain
errors and the tool."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cryo_ralib_amd import tsne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_ref.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def csr(z, c, p):
    return (z["indptr_%s_%d" % (c, p)].astype(np.int64), z["indices_%s_%d" % (c, p)].astype(np.int64),
            z["P_%s_%d" % (c, p)].astype(np.float64))


@pytest.mark.parametrize("c,p", [("a", 30), ("a", 5), ("b", 30), ("b", 5)])
def test_affinities_match_sklearn(z, c, p):
    indptr, indices, P = tsne.affinities(z["X_" + c], float(p), backend="numpy")
    ri, rx, rP = csr(z, c, p)
    assert np.array_equal(indptr, ri) and np.array_equal(indices, rx)
    # sklearn's kNN distances are float32 (1e-7 relative), and the perplexity search stops at an entropy tolerance of 1e-5, so
    # exact distances move P by up to ~1e-5 of its maximum; with equal inputs the search agrees to 1e-6 (the next test)
    assert np.abs(P - rP).max() <= 2e-5 * rP.max()


def test_perplexity_search_matches_sklearns_routine(z):
    _utils = pytest.importorskip("sklearn.manifold._utils")
    X = z["X_a"]
    idx, d2 = tsne.knn_numpy(X, 91)
    ours = tsne.binary_search_perplexity(d2, 30.0)
    ref = _utils._binary_search_perplexity(d2.astype(np.float32), 30.0, 0)
    assert np.abs(ours - ref).max() <= 1e-6 * ref.max()


def test_knn_matches_brute_force():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(300, 7)).astype(np.float32)
    idx, d2 = tsne.knn_numpy(X, 40)
    D = ((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    ref = np.argsort(D, axis=1, kind="stable")[:, :40]
    assert np.array_equal(idx, ref)
    assert np.allclose(d2, np.take_along_axis(D, ref, 1), rtol=1e-12)


@pytest.mark.parametrize("s", ["init", "early", "late"])
def test_gradient_and_error_match_sklearn(z, s):
    e, g = tsne.gradient_numpy(z["state_a_" + s], csr(z, "a", 30), float(z["exag_a_" + s]))
    gr = z["grad_a_" + s]
    # sklearn computes in float32: at the converged state the forces cancel to ~1e-4 of their size
    assert np.abs(g - gr).max() <= (1e-5 if s != "late" else 1e-3) * np.abs(gr).max()
    assert abs(np.linalg.norm(g) - np.linalg.norm(gr)) <= (1e-5 if s != "late" else 1e-3) * np.linalg.norm(gr)
    assert abs(e - float(z["error_a_" + s])) <= 1e-5 * abs(float(z["error_a_" + s]))


def test_learning_rate_auto():
    assert tsne.resolve_learning_rate("auto", 1000, 12.0) == 50.0
    assert tsne.resolve_learning_rate("auto", 50000, 12.0) == 50000 / 12.0 / 4
    assert tsne.resolve_learning_rate(200.0, 50000, 12.0) == 200.0


class _Recorder:
    """a state that records the schedule it is driven with and returns set errors"""

    def __init__(self, errors=None, grad_norm2=1.0):
        self.calls, self.resets, self.errors, self.gn2 = [], 0, errors, grad_norm2

    def reset(self):
        self.resets += 1

    def step(self, exaggeration, momentum, learning_rate, want):
        self.calls.append((exaggeration, momentum, want))
        if not want:
            return None
        return (self.errors(len(self.calls) - 1) if self.errors else 1.0 / len(self.calls)), self.gn2


def test_schedule_switches_at_250():
    r = _Recorder()
    err, it, errors = tsne._optimise(r, 1000, 12.0, 200.0, 300, 1e-7)
    assert it == 999 and r.resets == 2 and len(r.calls) == 1000 and len(errors) == 20
    assert all(c[:2] == (12.0, 0.5) for c in r.calls[:250]) and all(c[:2] == (1.0, 0.8) for c in r.calls[250:])
    assert [i for i, c in enumerate(r.calls) if c[2]] == [i for i in range(1000) if (i + 1) % 50 == 0]


def test_large_min_grad_norm_stops_at_first_check():
    r = _Recorder()
    err, it, errors = tsne._optimise(r, 1000, 12.0, 200.0, 300, 1e9)
    # sklearn: the exploration stops at iteration 49, the second run starts at 50 and stops at its first check, 99
    assert it == 99 and len(r.calls) == 100 and len(errors) == 2
    assert all(c[0] == 12.0 for c in r.calls[:50]) and all(c[0] == 1.0 for c in r.calls[50:])


def test_no_progress_stops():
    r = _Recorder(errors=lambda i: 1.0)       # never improves after its first check
    err, it, errors = tsne._optimise(r, 2000, 12.0, 200.0, 300, 0.0)
    # second run: best at 299; i - best > 300 first at the check 649
    assert it == 649


def test_max_iter_250_returns_like_sklearn():
    r = _Recorder()
    err, it, errors = tsne._optimise(r, 250, 12.0, 200.0, 300, 1e-7)
    assert it == 250 and err == np.finfo(float).max and len(r.calls) == 250


def test_full_run_matches_sklearn_small(z):
    X = z["X_b"]
    r = tsne.tsne(X, init=z["init_b"], backend="numpy")
    # 160 points: trajectories part chaotically, and the small case's final KL scatters more than the 800-point one's
    assert abs(r.kl_divergence - float(z["kl_b"])) <= 0.05 * float(z["kl_b"])
    assert abs(r.n_iter - int(z["n_iter_b"])) <= tsne.N_ITER_CHECK
    assert tsne.trustworthiness(X, r.embedding) >= float(z["trust_b"]) - 0.01
    assert len(r.errors) == (r.n_iter + 1) // tsne.N_ITER_CHECK


def test_pca_init_matches_sklearn(z):
    for c in "ab":
        Y = tsne.initial_embedding(z["X_" + c], "pca", backend="numpy")
        assert np.abs(Y - z["init_" + c]).max() <= 1e-3 * np.abs(z["init_" + c]).max()


def test_random_init_is_sklearns_bit_for_bit():
    man = pytest.importorskip("sklearn.manifold")
    X = np.random.default_rng(0).normal(size=(60, 4)).astype(np.float32)
    for seed in (0, 5, 123):
        ts = man.TSNE(init="random", random_state=seed, max_iter=250, perplexity=5.0, method="barnes_hut", angle=0.0)
        ts._validate_params()
        rs = np.random.RandomState(seed)
        ref = 1e-4 * rs.standard_normal(size=(60, 2)).astype(np.float32)
        got = tsne.random_init(60, seed)
        assert got.dtype == np.float32 and np.array_equal(got, ref)


def test_trustworthiness_matches_sklearn():
    man = pytest.importorskip("sklearn.manifold")
    rng = np.random.default_rng(11)
    for n, d, k in ((50, 5, 5), (120, 10, 10), (200, 3, 7)):
        X = rng.normal(size=(n, d))
        Y = X[:, :2] + 0.3 * rng.normal(size=(n, 2))
        assert abs(tsne.trustworthiness(X, Y, k) - man.trustworthiness(X, Y, n_neighbors=k)) < 1e-12


@pytest.mark.parametrize("kw", [dict(perplexity=0.0), dict(perplexity=101.0), dict(perplexity=20.0, n=20), dict(max_iter=249),
                                dict(n_components=3), dict(n=1), dict(d=2049), dict(early_exaggeration=0.5),
                                dict(learning_rate=-1.0), dict(learning_rate="fast")])
def test_domain_errors(kw):
    n, d = kw.pop("n", 40), kw.pop("d", 3)
    with pytest.raises(tsne.TsneError):
        tsne.tsne(np.zeros((n, d), np.float32), backend="numpy", **kw)


def test_non_finite_and_bad_init_rejected():
    X = np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32)
    Xn = X.copy()
    Xn[3, 1] = np.nan
    for bad in (dict(X=Xn), dict(init=np.zeros((39, 2))), dict(init="spectral"), dict(X=X[:, :1], init="pca"),
                dict(backend="cuda")):
        args = dict(X=X, perplexity=5.0, backend="numpy")
        args.update(bad)
        with pytest.raises(tsne.TsneError):
            tsne.tsne(args.pop("X"), **args)


def test_tool_numpy_backend(tmp_path, z):
    src = tmp_path / "sdr.npz"
    np.savez(src, factors=z["X_b"])
    out = tmp_path / "emb.npz"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "cryo_ralib_amd.tsne", str(src), str(out), "--backend", "numpy", "--perplexity",
                        "10", "--max_iter", "300", "--init", "random", "--seed", "3"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    o = np.load(out)
    assert o["embedding"].shape == (160, 2) and np.all(np.isfinite(o["embedding"]))
    assert int(o["n_iter"]) == 299 and float(o["perplexity"]) == 10.0 and int(o["seed"]) == 3
    assert len(o["errors"]) == 6 and float(o["kl_divergence"]) == float(o["errors"][-1])
    bad = subprocess.run([sys.executable, "-m", "cryo_ralib_amd.tsne", str(src), str(out), "--backend", "numpy", "--perplexity",
                          "500"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "perplexity" in bad.stderr
