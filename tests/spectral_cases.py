"""What the spectral suites (tests/test_spectral_cpu.py, tests/test_gpu_spectral.py) and tests/golden/make_spectral_pins.py share:
the data generators, the list of pins, the Davis-Kahan comparison of eigenvectors and the builders of the kernel tests."""
import os

import numpy as np

from ward_cases import same_partition  # noqa: F401 -- labels equal up to a renaming

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_ref.npz")
EPS = 2.0 ** -52
MIN_GAP = 1e-4              # the least distance of a pinned eigenvalue to the rest of the spectrum
KNN_MARGIN = 1e-9           # the least D2 margin between the last listed neighbour and the first one left out


def gaussian(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def ring(n, seed, noise=0.05):
    """a noisy ring in 2-D, sampled unevenly (so that the cos / sin pairs of a uniform ring split)"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, n)
    phi = 2.0 * np.pi * (u + 0.12 * np.sin(2.0 * np.pi * u) + 0.05 * np.sin(4.0 * np.pi * u + 1.0))
    r = 1.0 + noise * rng.normal(size=n)
    return np.stack([r * np.cos(phi), 0.8 * r * np.sin(phi)], axis=1).astype(np.float32)


def blobs(n, d, centers, seed, spread=1.0, box=1.0):
    """overlapping blobs: centres in a small box, so that the kNN graph is connected; on a grid of 1 / 256 (the pin file stays small)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-box, box, (centers, d))
    which = rng.integers(0, centers, n)
    return (np.round((c[which] + spread * rng.normal(size=(n, d))) * 256.0) / 256.0).astype(np.float32)


def two_blobs(n_a, n_b, d, seed, apart=100.0):
    """two far-apart Gaussian blobs, interleaved: (X, mask of the first blob)"""
    rng = np.random.default_rng(seed)
    A, B = rng.normal(size=(n_a, d)), rng.normal(size=(n_b, d)) + apart
    perm = rng.permutation(n_a + n_b)
    return np.concatenate([A, B])[perm].astype(np.float32), (perm < n_a)


def arcs(n, seed, noise=0.04):
    """two interleaved half circles (two moons): (X, truth)"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, np.pi, n)
    y = (np.arange(n) % 2).astype(np.int64)
    x = np.where(y == 0, np.cos(t), 1.0 - np.cos(t))
    z = np.where(y == 0, np.sin(t), 0.5 - np.sin(t))
    return (np.stack([x, z], axis=1) + noise * rng.normal(size=(n, 2))).astype(np.float32), y


# name -> (X, options of spectral.embedding, compared with sklearn)
def pin_cases():
    g3 = gaussian(400, 3, 1)
    return {
        "gauss3": (g3, dict(n_components=5, n_neighbors=10), True),
        "gauss5": (gaussian(1500, 5, 2), dict(n_components=4, n_neighbors=15), True),
        "ring": (ring(1200, 3), dict(n_components=4, n_neighbors=12), True),
        "blobs50": (blobs(600, 50, 8, 4), dict(n_components=4, n_neighbors=15), True),
        "selftune": (g3, dict(n_components=4, n_neighbors=10, affinity="gaussian", local_scale=7), False),
        "alpha1": (g3, dict(n_components=4, n_neighbors=10, alpha=1.0), False),
    }


ARCS = dict(n=600, seed=6, noise=0.08, n_neighbors=10)      # noisy enough for the two arcs to touch: one component


def graph_options(opt):
    return {k: v for k, v in opt.items() if k in ("n_neighbors", "affinity", "local_scale", "alpha")}


def unit_vectors(E, s):
    """the unit eigenvectors of M behind the columns of an embedding E = y s: [c][n]"""
    Y = (E / s[:, None]).T
    return Y / np.linalg.norm(Y, axis=1)[:, None]


def degree_scale(indptr, a):
    """s = 1 / sqrt(deg) of a CSR graph, a row's entries added in row order"""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return 1.0 / np.sqrt(np.bincount(rows, weights=a, minlength=len(indptr) - 1))


def vector_bound(r, gap, n):
    """Davis-Kahan with the stored gap: a unit vector with residual r lies within 2 r / gap of the eigenvector (sin <= r / gap and
    |y - u| <= sqrt(2) sin for an acute angle), plus the rounding of a unit vector of n entries"""
    return 2.0 * np.asarray(r) / np.asarray(gap) + n * EPS


def check_against_pins(z, c, res, graph, with_sklearn):
    """the bounds of tests/test_spectral_cpu.py's docstring on a SpectralResult of pin c; prints every figure before it asserts"""
    indptr, indices, a, _ = graph
    n = len(indptr) - 1
    s = degree_scale(indptr, a)
    gap, theta = z["gap_" + c], z["theta_" + c]
    assert res.converged and np.all(np.isfinite(res.embedding)) and res.n_dropped == 0
    dth = np.abs(res.eigenvalues - theta)
    print(c, "steps", res.n_steps, "residuals", res.residuals, "|theta - dense|", dth)
    assert np.all(dth <= res.residuals)
    assert np.array_equal(res.laplacian_eigenvalues, 1.0 - res.eigenvalues)
    Y = unit_vectors(res.embedding, s)
    d_dense = np.linalg.norm(Y - unit_vectors(z["dense_E_" + c], s), axis=1)
    print(c, "|y - dense|", d_dense, "bound", vector_bound(res.residuals, gap, n))
    assert np.all(d_dense <= vector_bound(res.residuals, gap, n))
    if with_sklearn:
        d_sk = np.linalg.norm(Y - unit_vectors(z["sk_E_" + c], s), axis=1)
        print(c, "|y - sklearn|", d_sk, "bound", vector_bound(res.residuals + z["sk_res_" + c], gap, n))
        assert np.all(d_sk <= vector_bound(res.residuals + z["sk_res_" + c], gap, n))


def random_csr(lengths, n_cols, seed):
    """a CSR with the given row lengths, ascending distinct columns in 0 .. n_cols - 1 and Gaussian values"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    idx = [np.sort(rng.choice(n_cols, int(L), replace=False)) for L in lengths]
    indices = (np.concatenate(idx) if len(idx) else np.zeros(0)).astype(np.int32)
    return indptr, indices, rng.normal(size=len(indices))


def path_graph(n):
    """0 - 1 - 2 - ... - (n - 1): the worst case for the rounds of label propagation"""
    return edges_to_csr(n, np.stack([np.arange(n - 1), np.arange(1, n)], axis=1))


def weighted_path(n):
    """the path with the weight i + 1 on the edge (i, i + 1): no symmetry, so no two entries of an eigenvector tie in magnitude"""
    indptr, indices, _ = path_graph(n)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    return indptr, indices, (np.minimum(rows, indices) + 1).astype(np.float64)


def edges_to_csr(n, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    both = np.concatenate([e, e[:, ::-1]])
    keys = np.unique(both[:, 0] * n + both[:, 1])
    indptr = np.searchsorted(keys // n, np.arange(n + 1)).astype(np.int32)
    return indptr, (keys % n).astype(np.int32), np.ones(len(keys))
