"""Golden t-SNE values from scikit-learn 1.7 (TSNE with method="barnes_hut", angle=0), for tests/test_tsne_cpu.py and
tests/test_gpu_tsne.py, which never import sklearn for them:

    python tests/golden/make_tsne_pins.py

Two inputs: case a, a seeded set of 800 x 20 float32 points in four Gaussian clusters (`X_a`, `labels_a`), and case b, the
2SDR factors of sdr_ref.npz case 0 (`X_b`, 160 x 5).  Per case c and perplexity p in (30, 5): sklearn's own kNN graph and
_joint_probabilities_nn as CSR (`indptr_c_p`, `indices_c_p` int16, `P_c_p` float32).  Per case at perplexity 30: the scaled PCA
init of sklearn (`init_c`), the final embedding of TSNE(init=init_c, max_iter=1000) (`emb_c`) with `kl_c`, `n_iter_c` and
`trust_c` = trustworthiness(X, emb, n_neighbors=10).  Case a also holds three states at which _kl_divergence_bh(angle=0) was
evaluated, `state_a_s` for s in (init, early, late) with `exag_a_s`, `error_a_s` and `grad_a_s` [n][2]: the init, the
embedding after the 250 exaggerated iterations (evaluated with exaggeration 12) and the final embedding (exaggeration 1).
"""
import os

import numpy as np
import sklearn
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE, trustworthiness
from sklearn.manifold._t_sne import _joint_probabilities_nn, _kl_divergence_bh
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))


def clustered(n=800, d=20, ncl=4, seed=7):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (ncl, d))
    labels = rng.integers(0, ncl, n)
    X = centres[labels] + rng.normal(0.0, 1.0, (n, d)) * rng.uniform(0.5, 1.5, ncl)[labels, None]
    return X.astype(np.float32), labels.astype(np.int16)


def joint_p(X, perplexity):
    n = X.shape[0]
    k = min(n - 1, int(3.0 * perplexity + 1))
    g = NearestNeighbors(n_neighbors=k).fit(X).kneighbors_graph(mode="distance")
    g.data **= 2
    return _joint_probabilities_nn(g, perplexity, 0)


def pca_init(X):
    E = PCA(n_components=2, svd_solver="randomized", random_state=0).fit_transform(X).astype(np.float32)
    return E / np.std(E[:, 0]) * 1e-4


def bh(Y, P, exag):
    err, g = _kl_divergence_bh(np.asarray(Y, np.float32).ravel(), P * exag, 1, Y.shape[0], 2, angle=0.0, verbose=0,
                               compute_error=True, num_threads=1)
    return float(err), g.reshape(-1, 2).astype(np.float64)


def main():
    assert sklearn.__version__.startswith("1.7"), sklearn.__version__
    out = {}
    Xa, labels = clustered()
    Xb = np.load(os.path.join(HERE, "sdr_ref.npz"))["factors_0"].astype(np.float32)
    out["X_a"], out["labels_a"], out["X_b"] = Xa, labels, Xb
    for c, X in (("a", Xa), ("b", Xb)):
        for p in (30, 5):
            P = joint_p(X, float(p))
            out["indptr_%s_%d" % (c, p)] = P.indptr.astype(np.int32)
            out["indices_%s_%d" % (c, p)] = P.indices.astype(np.int16)
            out["P_%s_%d" % (c, p)] = P.data.astype(np.float32)
        init = pca_init(X)
        ts = TSNE(n_components=2, perplexity=30.0, method="barnes_hut", angle=0.0, init=init, max_iter=1000, random_state=0)
        emb = ts.fit_transform(X)
        out["init_" + c], out["emb_" + c] = init, emb.astype(np.float32)
        out["kl_" + c], out["n_iter_" + c] = np.float64(ts.kl_divergence_), np.int64(ts.n_iter_)
        out["trust_" + c] = np.float64(trustworthiness(X, emb, n_neighbors=10))
        if c == "a":
            early = TSNE(n_components=2, perplexity=30.0, method="barnes_hut", angle=0.0, init=init, max_iter=250,
                         random_state=0).fit_transform(X)
            P = joint_p(X, 30.0)
            for s, Y, e in (("init", init, 12.0), ("early", early, 12.0), ("late", emb, 1.0)):
                err, g = bh(Y, P, e)
                out["state_a_" + s], out["exag_a_" + s] = np.asarray(Y, np.float32), np.float64(e)
                out["error_a_" + s], out["grad_a_" + s] = np.float64(err), g
        print(c, X.shape, "kl %.6f n_iter %d trust %.4f" % (ts.kl_divergence_, ts.n_iter_, out["trust_" + c]))
    path = os.path.join(HERE, "tsne_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
