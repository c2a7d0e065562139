"""Spectral embedding (Laplacian eigenmaps / diffusion maps) of factors X [n][d] and spectral clustering on the GPU (after
scikit-learn 1.7 SpectralEmbedding / SpectralClustering with affinity="nearest_neighbors"; Coifman and Lafon's density
normalisation; Zelnik-Manor and Perona's self-tuning weights).

    python -m cryo_ralib_amd.spectral IN OUT.npz [--n_components 2] [--n_neighbors 15] [--affinity connectivity|gaussian]
                                      [--local_scale 7] [--alpha 0] [--diffusion_time 0] [--tol 1e-10] [--max_steps 1024] [--seed 0]
                                      [--on_disconnected largest|error] [--key factors] [--backend device|numpy] [--quality [K]]
                                      [--k K [--truth FILE] [--stack STACK --params PARAMS --ou R --averages REFS.{hdf,mrcs,npy}]]

IN is the OUT.npz of the sdr tool (--key factors, the default) or an [n][d] .npy.  OUT.npz holds embedding [n][c] (nan rows outside
the embedded component), eigenvalues, laplacian_eigenvalues, residuals, component, n_steps, converged, n_dropped and the options;
with --k also labels (-1 outside the embedded component), centers and inertia of the spectral clustering into K classes (--truth and
--averages leave label -1 out, as the density tools leave noise out); with --quality trustworthiness and continuity of the embedded
rows.  The kmeans, gmm, dbscan, hdbscan and ward tools read the file with --key embedding (they refuse nan: embed a connected graph,
or raise --n_neighbors), and with --k the tsne tool's --fit_labels takes it as it is.

The coordinates are a deterministic function of the data; they order particles along a continuous coordinate, and k-means on them
(spectral clustering) separates arcs and rings with a chosen k.

The contract, rule by rule.  Everything after the neighbour lists is float64.
  1. Neighbours.  N(i) is the n_neighbors - 1 nearest OTHER rows: exactly ra_tsne_knn(X, k = n_neighbors - 1), ordered by (D2, j),
     D2 in double from the differences of the float32 values.  This is sklearn's kneighbors_graph(X, n_neighbors,
     include_self=True), whose self-loop csgraph_laplacian discards.
  2. Weights.  Directed w_ij for j in N(i).  affinity="connectivity" (sklearn's): w_ij = 1.  affinity="gaussian" (self-tuning):
     w_ij = exp(-D2_ij / (sigma_i sigma_j)), sigma_i = sqrt(D2 to the local_scale-th neighbour of i), 1 <= local_scale <=
     n_neighbors - 1; a row with sigma_i = 0 (duplicates) raises, naming the first such row.  a_ij = (w_ij [j in N(i)] + w_ji [i in
     N(j)]) / 2, a_ii = 0: a CSR with the columns of a row ascending, built by _graph.py's stable sort (no scatter), so
     a_ij == a_ji bit for bit.
  3. Components.  The connected components of a are numbered by lowest member: component [n] int32.  on_disconnected="largest"
     (default) embeds the largest component (ties: the lower number); its rows keep their order and are compacted to n_sub rows;
     every other row gets nan coordinates, and one warning carries sklearn's text plus the number of rows left out.
     on_disconnected="error" raises.  n_sub >= n_components + 2, else an error.
  4. Density normalisation.  0 <= alpha <= 1.  q_i = sum_j a_ij, a_ij <- a_ij / (q_i^alpha q_j^alpha).  alpha = 0 leaves the values
     untouched, bit for bit.
  5. Operator.  deg_i = sum_j a_ij, s_i = 1 / sqrt(deg_i), M_ij = (s_i a_ij) s_j stored once as CSR values.  (The checker adds a
     row's entries in row order; the device in spec_spmv_kernel's order with x = 1, fixed by the row's length.)  The eigenvalues of
     M lie in [-1, 1]; the top one is 1 with vector q0 = sqrt(deg) / |sqrt(deg)|.
  6. Solver.  Lanczos on M in the complement of q0.  Start: RandomState(random_state).uniform(-1, 1, n_sub), random_state = 0 by
     default (the result is a pure function of the arguments), orthogonalised against q0 and normalised on the host.  Step j:
     w = M v_j; alpha_j = v_j . w; twice h = Q^T w, w -= Q h with Q = [q0, v_0 .. v_j]; beta_j = |w|; v_{j+1} = w / beta_j.
     Check every CHECK = 8 steps from m >= c, and at m_max = min(max_steps, n_sub - 1): the host reads alpha and beta, takes
     numpy.linalg.eigh of the tridiagonal and accepts when |beta_{m-1} S[m-1][t]| <= tol for each of the c largest Ritz values; tol is
     absolute since |M| <= 1.  Between checks the host reads nothing.  A recorded beta_j <= 2^-40 truncates the basis at v_0 .. v_j
     (an invariant subspace: its Ritz pairs are exact) and is accepted.  At m_max without acceptance: converged = False and a warning.
  7. Ritz vectors and scaling.  y_t = sum_j S[j][t] v_j in j order, theta descending (Laplacian eigenvalue 1 - theta).  E[:, t] =
     y_t s (sklearn's embedding / dd), then sklearn's _deterministic_vector_sign_flip: the entry of largest magnitude of each
     column is positive, the first on ties.  diffusion_time = tau >= 0 multiplies column t by max(theta_t, 0)^tau; at 0 nothing is
     multiplied.  drop_first=True (default) returns the c non-trivial columns; drop_first=False puts the analytic constant column
     1 / sqrt(sum deg) first and computes c - 1 others (what sklearn's SpectralClustering feeds to k-means).
  8. Residuals.  r_t = |M y_t - theta_t y_t|_2 is computed on the result, not estimated.  A degenerate eigenvalue gives an arbitrary
     basis of its eigenspace: compare such columns as a subspace, not vector by vector.
  9. Determinism.  Every sum over rows or over basis vectors has an order fixed by the sizes alone; no floating-point atomics; no
     workgroup waits for another.  The same call gives the same bits on any stream.
 10. Spectral clustering.  cluster(X, n_clusters) is rules 1 - 8 with n_components = n_clusters, drop_first=False, then
     kmeans.kmeans on the embedded rows rounded to float32 once.  Rows outside the embedded component get label -1.
Domain: 3 <= n <= 262144, 1 <= d <= 2048, 2 <= n_neighbors <= min(302, n), 1 <= n_components <= 64, 0 <= alpha <= 1, tol > 0,
n_components + 1 <= max_steps <= 4096, diffusion_time >= 0, finite X.  Anything else raises SpectralError (a ValueError) before
anything is launched.  The kNN's float32 screen has its documented limit on uncentred data.
Not built: Nystrom out-of-sample extension; restarted, Chebyshev-filtered or block solvers; rbf or precomputed dense affinities;
assign_labels="discretize" / "cluster_qr"; more than 262144 points; multi-GPU.

On the device the neighbour lists come from ra_tsne_knn, the graph is torch plumbing (one stable sort), a component round is
ra_spectral_components (one int read per round), and the solve is ra_spectral_lanczos (csrc/ralign_spectral.h: the CSR product, the
partial dots [runs][j + 2], their reduction in run order, the update in t order, the norm and the scale, enqueued CHECK steps at a
time), ra_spectral_ritz and ra_spectral_spmv for the residuals.  The basis V [m_max + 1][n_sub] stays in device memory.
backend="numpy" is the float64 checker: the same rules, unfused, with no [n][n] array and no GPU.  dense_numpy is the literal
definition (numpy.linalg.eigh of the dense M) for tests and pins, n <= 4000.
"""
import argparse
import sys
import warnings

import numpy as np

from . import _common, _graph
from ._common import Launcher, is_int, is_real, ptr

MAX_N, MAX_D = 262144, 2048
MAX_NEIGHBORS = 302             # ra_tsne_knn takes at most 301 others
MAX_COMPONENTS = 64
MAX_STEPS = 4096
MAX_DENSE_N = 4000
MAX_AVERAGES = 256              # kmeans.class_averages' limit on the number of classes
CHECK = 8
BREAKDOWN = 2.0 ** -40
NOT_CONNECTED = "Graph is not fully connected, spectral embedding may not work as expected."


class SpectralError(ValueError):
    """an input outside the supported domain"""


class SpectralWarning(UserWarning):
    """a disconnected graph, or a solve that stopped at max_steps"""


def _need(ok, msg):
    if not ok:
        raise SpectralError(msg)


def check_domain(n, d, n_neighbors=15, affinity="connectivity", local_scale=7, alpha=0.0):
    """raise SpectralError unless the shape and the graph options are inside the supported domain"""
    _need(3 <= n <= MAX_N, "need 3 <= n <= %d points, got %d" % (MAX_N, n))
    _need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    _need(is_int(n_neighbors) and 2 <= n_neighbors <= min(MAX_NEIGHBORS, n),
          "need an integer 2 <= n_neighbors <= min(%d, n = %d), got %r" % (MAX_NEIGHBORS, n, n_neighbors))
    _need(affinity in ("connectivity", "gaussian"), "affinity is 'connectivity' or 'gaussian', got %r" % (affinity,))
    if affinity == "gaussian":
        _need(is_int(local_scale) and 1 <= local_scale <= n_neighbors - 1,
              "need an integer 1 <= local_scale <= n_neighbors - 1 = %d, got %r" % (n_neighbors - 1, local_scale))
    check_alpha(alpha)


def check_alpha(alpha):
    _need(is_real(alpha) and 0 <= alpha <= 1, "need 0 <= alpha <= 1, got %r" % (alpha,))


def check_solver(n_components, diffusion_time=0.0, tol=1e-10, max_steps=1024, random_state=0, on_disconnected="largest"):
    """raise SpectralError unless the solver options are inside the supported domain"""
    _need(is_int(n_components) and 1 <= n_components <= MAX_COMPONENTS,
          "need an integer 1 <= n_components <= %d, got %r" % (MAX_COMPONENTS, n_components))
    _need(is_real(diffusion_time) and diffusion_time >= 0, "need a finite diffusion_time >= 0, got %r" % (diffusion_time,))
    _need(is_real(tol) and tol > 0, "need a finite tol > 0, got %r" % (tol,))
    _need(is_int(max_steps) and n_components + 1 <= max_steps <= MAX_STEPS,
          "need an integer n_components + 1 <= max_steps <= %d, got %r" % (MAX_STEPS, max_steps))
    _need(is_int(random_state) and 0 <= random_state < 2 ** 32, "random_state is an integer in 0 .. 2^32 - 1, got %r" % (random_state,))
    _need(on_disconnected in ("largest", "error"), "on_disconnected is 'largest' or 'error', got %r" % (on_disconnected,))


class SpectralResult:
    """embedding float64 [n][c] (nan rows outside the embedded component); eigenvalues (theta, descending) and laplacian_eigenvalues
    (1 - theta) float64 [c]; residuals float64 [c] (rule 8; with drop_first=False the first, analytic, column has eigenvalue 1 and
    residual 0); n_steps (the basis size used), converged; component int32 [n]; rows int64 [n_sub] (the embedded rows); n_dropped"""

    def __init__(self, embedding, eigenvalues, residuals, n_steps, converged, component, rows):
        self.embedding, self.eigenvalues, self.residuals = embedding, eigenvalues, residuals
        self.laplacian_eigenvalues = 1.0 - eigenvalues
        self.n_steps, self.converged, self.component, self.rows = int(n_steps), bool(converged), component, rows
        self.n_dropped = int(len(component) - len(rows))


class SpectralClusterResult:
    """labels int32 [n] (-1 outside the embedded component), the SpectralResult as .embedding_result, its coordinates as .embedding
    and the kmeans.KMeansResult of the embedded rows as .kmeans"""

    def __init__(self, labels, emb, km):
        self.labels, self.embedding_result, self.embedding, self.kmeans = labels, emb, emb.embedding, km


# ---- rules 1 - 5 in numpy: the checker

def _weights_numpy(idx, d2, affinity, local_scale):
    if affinity == "connectivity":
        return np.ones(idx.shape, np.float64)
    sigma = np.sqrt(d2[:, local_scale - 1])
    zero = np.nonzero(~(sigma > 0))[0]
    _need(not len(zero), "row %d has sigma = 0: its %d nearest rows are duplicates of it" % (zero[0] if len(zero) else -1, local_scale))
    return np.exp(-d2 / (sigma[:, None] * sigma[idx]))


def _symmetrize_numpy(idx, w):
    indptr, indices, a, b = _graph.symmetrize_numpy(idx, w)
    return indptr.astype(np.int32), indices.astype(np.int32), 0.5 * (a + b)


def _row_sums_numpy(indptr, a):
    """sum_j a_ij with a row's entries added in row order (bincount adds in index order)"""
    return np.bincount(_graph.row_ids_numpy(indptr), weights=a, minlength=len(indptr) - 1)


def _density_numpy(indptr, indices, a, alpha):
    if alpha == 0:
        return a
    q = _row_sums_numpy(indptr, a) ** alpha
    return a / (q[_graph.row_ids_numpy(indptr)] * q[indices])


def components_numpy(indptr, indices):
    """int64 [n]: the lowest member of every row's connected component, by the device's rounds (minimum-label hooking, pointer
    compression).  Apart from dbscan._components, which hooks over an edge list and counts its rounds."""
    n = len(indptr) - 1
    rows, cols = _graph.row_ids_numpy(indptr), np.asarray(indices, np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:
        m = label.copy()
        np.minimum.at(m, rows, label[cols])
        P = label.copy()
        hook = np.nonzero(m < label)[0]
        np.minimum.at(P, label[hook], m[hook])
        np.minimum.at(P, hook, m[hook])
        new = _graph.jump(P)
        if np.array_equal(new, label):
            return label
        label = new


def _number(root):
    """components numbered by lowest member"""
    return np.searchsorted(np.unique(root), root).astype(np.int32)


def check_graph(indptr, indices, a):
    """(indptr int32, indices int32, a float64) of a symmetric CSR with ascending columns, or SpectralError"""
    indptr, indices, a = np.asarray(indptr), np.asarray(indices), np.asarray(a, np.float64)
    _need(indptr.ndim == 1 and indices.ndim == 1 and a.ndim == 1 and len(indptr) >= 2, "indptr [n + 1], indices [nnz] and a [nnz] are 1-D")
    for v, name in ((indptr, "indptr"), (indices, "indices")):
        _need(np.issubdtype(v.dtype, np.integer), "%s holds integers" % name)
    n = len(indptr) - 1
    _need(3 <= n <= MAX_N, "need 3 <= n <= %d rows, got %d" % (MAX_N, n))
    _need(indptr[0] == 0 and np.all(np.diff(indptr) >= 0) and indptr[-1] == len(indices) == len(a) and len(a) < 2 ** 31,
          "indptr ascends from 0 to nnz = len(indices) = len(a) < 2^31")
    _need(len(indices) > 0, "the graph has no edges")
    _need(indices.min() >= 0 and indices.max() < n, "a column index is outside 0 .. n - 1")
    rows = _graph.row_ids_numpy(indptr)
    keys = rows * n + indices.astype(np.int64)
    _need(np.all(np.diff(keys) > 0), "the columns of a row ascend strictly")
    _need(not np.any(rows == indices), "the diagonal is not stored (a_ii = 0)")
    _need(bool(np.all(np.isfinite(a))) and bool(np.all(a >= 0)), "the weights are finite and >= 0")
    back = np.searchsorted(keys, indices.astype(np.int64) * n + rows)
    ok = (back < len(keys))
    ok[ok] = keys[back[ok]] == (indices.astype(np.int64) * n + rows)[ok]
    _need(bool(np.all(ok)) and np.array_equal(a[np.minimum(back, len(a) - 1)], a), "the matrix is symmetric: a_ij == a_ji")
    return indptr.astype(np.int32), indices.astype(np.int32), a


# ---- the same on the device

class _Device(Launcher):
    """rules 2 - 5 on the current stream of X's device: torch plumbing, ra_spectral_components and ra_spectral_spmv (rule 1's lists
    are _graph.knn's)"""

    def weights(self, idx, d2, affinity, local_scale):
        torch = self.torch
        if affinity == "connectivity":
            return torch.ones(idx.shape, dtype=torch.float64, device=self.dev)
        sigma = torch.sqrt(d2[:, local_scale - 1])
        zero = torch.nonzero(~(sigma > 0))
        if zero.numel():
            raise SpectralError("row %d has sigma = 0: its %d nearest rows are duplicates of it" % (int(zero[0, 0].item()), local_scale))
        return torch.exp(-d2 / (sigma[:, None] * sigma[idx.long()]))

    def symmetrize(self, idx, w):
        indptr, indices, a, b = _graph.symmetrize_torch(idx, w)
        return indptr.to(self.torch.int32), indices.to(self.torch.int32), 0.5 * (a + b)

    def spmv(self, indptr, indices, val, x):
        y = self.torch.empty_like(x)
        self.call("ra_spectral_spmv", ptr(indptr), ptr(indices), ptr(val), int(x.numel()), ptr(x), ptr(y))
        return y

    def row_sums(self, indptr, indices, a):
        n = int(indptr.numel()) - 1
        return self.spmv(indptr, indices, a, self.torch.ones(n, dtype=self.torch.float64, device=self.dev))

    def density(self, indptr, indices, a, alpha):
        if alpha == 0:
            return a
        q = self.row_sums(indptr, indices, a) ** alpha
        return a / (q[_graph.row_ids_torch(indptr)] * q[indices.long()])

    def components(self, indptr, indices):
        torch = self.torch
        n = int(indptr.numel()) - 1
        label = torch.arange(n, dtype=torch.int32, device=self.dev)
        changed = torch.zeros(1, dtype=torch.int32, device=self.dev)
        for _ in range(n + 1):
            self.call("ra_spectral_components", ptr(indptr), ptr(indices), n, ptr(label), ptr(changed))
            if int(changed.item()) == 0:                    # the round's one read
                return label.cpu().numpy().astype(np.int64)
        raise RuntimeError("spectral: the component labels still move after n rounds")


def _graph_device(X, n_neighbors, affinity, local_scale, alpha):
    D = _Device(X)
    with D.torch.cuda.device(D.dev):
        idx, d2 = _graph.knn(D, X, n_neighbors - 1)
        indptr, indices, a = D.symmetrize(idx, D.weights(idx, d2, affinity, local_scale))
        a = D.density(indptr, indices, a, alpha)
        root = D.components(indptr, indices)
    return D, indptr, indices, a, root


def _graph_numpy(X, n_neighbors, affinity, local_scale, alpha):
    from . import tsne
    idx, d2 = tsne.knn_numpy(X, n_neighbors - 1)
    indptr, indices, a = _symmetrize_numpy(idx, _weights_numpy(idx, d2, affinity, local_scale))
    a = _density_numpy(indptr, indices, a, alpha)
    return indptr, indices, a, components_numpy(indptr, indices)


def _graph_input(X, n_neighbors, affinity, local_scale, alpha, backend):
    X = _common.as_input(X, backend, SpectralError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, n_neighbors, affinity, local_scale, alpha)
    _common.check_finite(X, backend, SpectralError)
    return X


def graph(X, n_neighbors=15, affinity="connectivity", local_scale=7, alpha=0.0, backend="device"):
    """rules 1 - 4 of X [n][d]: (indptr int32 [n + 1], indices int32 [nnz], a float64 [nnz], component int32 [n]) as numpy arrays"""
    X = _graph_input(X, n_neighbors, affinity, local_scale, alpha, backend)
    if backend == "numpy":
        indptr, indices, a, root = _graph_numpy(X, n_neighbors, affinity, local_scale, alpha)
        return indptr, indices, a, _number(root)
    _, indptr, indices, a, root = _graph_device(X, n_neighbors, affinity, local_scale, alpha)
    return indptr.cpu().numpy(), indices.cpu().numpy(), a.cpu().numpy(), _number(root)


# ---- rules 5 - 8: the operator of one component and its two solvers

class _NumpyOperator:
    """M of the compacted component, rule 6's step unfused"""

    def __init__(self, indptr, indices, a):
        self.indptr, self.indices, self.n = indptr, indices.astype(np.int64), len(indptr) - 1
        self.rows = _graph.row_ids_numpy(indptr)
        self.deg = _row_sums_numpy(indptr, a)
        _need(bool(np.all(self.deg > 0)), "a row of the embedded component has degree 0 (weights that underflow)")
        self.s = 1.0 / np.sqrt(self.deg)
        self.val = (self.s[self.rows] * a) * self.s[self.indices]

    def mv(self, x):
        return np.bincount(self.rows, weights=self.val * x[self.indices], minlength=self.n)

    def start(self, q0, v0, m_max):
        self.q0, self.m_max = q0, m_max
        self.Q = np.zeros((m_max + 2, self.n))
        self.Q[0], self.Q[1] = q0, v0
        self.alpha, self.beta = np.zeros(m_max), np.zeros(m_max)

    def run(self, j0, steps):
        for j in range(j0, j0 + steps):
            Q = self.Q[:j + 2]
            w = self.mv(Q[j + 1])
            self.alpha[j] = Q[j + 1] @ w
            for _ in range(2):
                w = w - (Q @ w) @ Q
            self.beta[j] = b = np.sqrt(w @ w)
            self.Q[j + 2] = w / b if b > BREAKDOWN else 0.0

    def read(self, m):
        return self.alpha[:m].copy(), self.beta[:m].copy()

    def ritz(self, S):
        return S.T @ self.Q[1:1 + S.shape[0]]

    def residuals(self, Y, theta):
        return np.array([np.linalg.norm(self.mv(y) - t * y) for y, t in zip(Y, theta)])


class _DeviceOperator:
    """M of the compacted component in device memory; ra_spectral_lanczos, ra_spectral_ritz and ra_spectral_spmv on the stream"""

    def __init__(self, D, indptr, indices, a):
        self.D, self.indptr, self.indices, self.n = D, indptr, indices, int(indptr.numel()) - 1
        deg = D.row_sums(indptr, indices, a)
        self.deg = deg.cpu().numpy()
        _need(bool(np.all(self.deg > 0)), "a row of the embedded component has degree 0 (weights that underflow)")
        s = 1.0 / D.torch.sqrt(deg)
        self.s = s.cpu().numpy()
        self.val = ((s[_graph.row_ids_torch(indptr)] * a) * s[indices.long()]).contiguous()

    def start(self, q0, v0, m_max):
        torch, D = self.D.torch, self.D
        self.q0 = torch.from_numpy(q0).to(D.dev)
        self.V = torch.zeros((m_max + 1, self.n), dtype=torch.float64, device=D.dev)
        self.V[0] = torch.from_numpy(v0).to(D.dev)
        self.ab = torch.zeros((2, m_max), dtype=torch.float64, device=D.dev)
        self.work = torch.empty(max(1, int(D.lib.ra_spectral_work_bytes(self.n, m_max))), dtype=torch.uint8, device=D.dev)

    def run(self, j0, steps):
        self.D.call("ra_spectral_lanczos", ptr(self.indptr), ptr(self.indices), ptr(self.val), self.n, ptr(self.q0), ptr(self.V), self.n,
                    j0, steps, ptr(self.ab[0]), ptr(self.ab[1]), ptr(self.work))

    def read(self, m):
        ab = self.ab[:, :m].cpu().numpy()
        return ab[0].copy(), ab[1].copy()

    def ritz(self, S):
        torch, D = self.D.torch, self.D
        m, c = S.shape
        Sd = torch.from_numpy(np.ascontiguousarray(S)).to(D.dev)
        self.Y = torch.empty((c, self.n), dtype=torch.float64, device=D.dev)
        D.call("ra_spectral_ritz", ptr(self.V), self.n, m, self.n, ptr(Sd), c, ptr(self.Y))
        return self.Y.cpu().numpy()

    def residuals(self, Y, theta):
        out = np.empty(len(theta))
        for t in range(len(theta)):
            my = self.D.spmv(self.indptr, self.indices, self.val, self.Y[t]).cpu().numpy()
            out[t] = np.linalg.norm(my - theta[t] * Y[t])
        return out


def _check_points(c, m_max):
    """rule 6: every CHECK steps from m >= c, and m_max"""
    pts = [m for m in range(CHECK, m_max, CHECK) if m >= c]
    return pts + [m_max]


def _tridiagonal_eigh(alpha, beta, m):
    T = np.diag(alpha[:m])
    if m > 1:
        T += np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    return np.linalg.eigh(T)


def _solve(op, c, tol, max_steps, random_state):
    """rules 6 - 8 on an operator: (Y [c][n_sub] unit Ritz vectors, theta [c] descending, residuals [c], n_steps, converged)"""
    n = op.n
    q0 = np.sqrt(op.deg)
    q0 /= np.sqrt(np.sum(op.deg))
    v0 = np.random.RandomState(random_state).uniform(-1.0, 1.0, n)
    for _ in range(2):
        v0 = v0 - (q0 @ v0) * q0
    v0 /= np.sqrt(v0 @ v0)
    m_max = min(max_steps, n - 1)
    op.start(q0, v0, m_max)
    done, converged = 0, False
    for m in _check_points(c, m_max):
        op.run(done, m - done)
        done = m
        alpha, beta = op.read(m)
        small = np.nonzero(~(beta > BREAKDOWN))[0]             # also a NaN: nothing after it is used
        broke = len(small) > 0
        if broke:
            m = int(small[0]) + 1
        if m < c:
            raise SpectralError("the Krylov space of the start vector has %d dimensions, fewer than the %d components asked for "
                                "(a graph with very few distinct eigenvalues)" % (m, c))
        lam, S = _tridiagonal_eigh(alpha, beta, m)
        top = np.argsort(-lam, kind="stable")[:c]
        est = np.abs(beta[m - 1] * S[m - 1, top])
        if broke or bool(np.all(est <= tol)):
            converged = True
            break
    if not converged:
        warnings.warn("spectral embedding: %d Lanczos steps did not reach tol = %g (largest estimated residual %.3g)"
                      % (m, tol, float(est.max())), SpectralWarning, stacklevel=3)
    theta, S = lam[top], np.ascontiguousarray(S[:, top])
    Y = op.ritz(S)
    return Y, theta, op.residuals(Y, theta), m, converged


def sign_flip(E):
    """sklearn's _deterministic_vector_sign_flip on the columns of E: the entry of largest magnitude is positive, the first on ties"""
    pos = np.argmax(np.abs(E), axis=0)
    sg = np.sign(E[pos, np.arange(E.shape[1])])
    return E * np.where(sg == 0, 1.0, sg)


def _finish(Y, theta, res, s, deg, diffusion_time, drop_first):
    """rule 7 from the unit Ritz vectors"""
    E = Y.T * s[:, None]
    if not drop_first:
        E = np.column_stack([np.full(len(s), 1.0 / np.sqrt(np.sum(deg))), E])
        theta, res = np.concatenate([[1.0], theta]), np.concatenate([[0.0], res])
    E = sign_flip(E)
    if diffusion_time != 0:
        E = E * np.maximum(theta, 0.0) ** diffusion_time
    return E, theta, res


def _pick_component(root, n_components, on_disconnected):
    """rule 3: (component int32 [n], rows int64 [n_sub] of the component to embed)"""
    comp = _number(root)
    sizes = np.bincount(comp)
    if len(sizes) > 1 and on_disconnected == "error":
        raise SpectralError("the graph has %d connected components (on_disconnected='error')" % len(sizes))
    rows = np.nonzero(comp == int(np.argmax(sizes)))[0]         # the first largest: the lower number
    _need(len(rows) >= n_components + 2, "the embedded component has %d rows, fewer than n_components + 2 = %d" % (len(rows), n_components + 2))
    if len(rows) < len(comp):
        warnings.warn("%s  The largest of %d components (%d rows) is embedded; %d rows are left out."
                      % (NOT_CONNECTED, len(sizes), len(rows), len(comp) - len(rows)), SpectralWarning, stacklevel=4)
    return comp, rows


def _sub_numpy(indptr, indices, a, rows, n):
    if len(rows) == n:
        return indptr, indices, a
    new = np.full(n, -1, np.int64)
    new[rows] = np.arange(len(rows))
    keep = new[_graph.row_ids_numpy(indptr)] >= 0
    cnt = np.diff(indptr)[rows]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), new[indices[keep]].astype(np.int32), a[keep]


def _sub_device(D, indptr, indices, a, rows, n):
    if len(rows) == n:
        return indptr, indices, a
    torch = D.torch
    new = torch.full((n,), -1, dtype=torch.int64, device=D.dev)
    r = torch.from_numpy(rows).to(D.dev)
    new[r] = torch.arange(len(rows), dtype=torch.int64, device=D.dev)
    keep = new[_graph.row_ids_torch(indptr)] >= 0
    cnt = (indptr[1:] - indptr[:-1]).long()[r]
    sub = torch.cat([torch.zeros(1, dtype=torch.int64, device=D.dev), torch.cumsum(cnt, 0)])
    return sub.to(torch.int32), new[indices.long()[keep]].to(torch.int32), a[keep].contiguous()


def _embed(make_op, root, n_components, diffusion_time, drop_first, tol, max_steps, random_state, on_disconnected):
    n = len(root)
    comp, rows = _pick_component(root, n_components, on_disconnected)
    c = n_components if drop_first else n_components - 1
    op = make_op(rows)
    if c > 0:
        Y, theta, res, m, converged = _solve(op, c, tol, min(max_steps, MAX_STEPS), random_state)
    else:
        Y, theta, res, m, converged = np.zeros((0, op.n)), np.zeros(0), np.zeros(0), 0, True
    E, theta, res = _finish(Y, theta, res, op.s, op.deg, diffusion_time, drop_first)
    full = np.full((n, E.shape[1]), np.nan)
    full[rows] = E
    return SpectralResult(full, theta, res, m, converged, comp, rows)


def embedding_from_graph(indptr, indices, a, n_components=2, alpha=0.0, diffusion_time=0.0, drop_first=True, tol=1e-10, max_steps=1024,
                         random_state=0, on_disconnected="largest", backend="device"):
    """rules 3 - 8 on a symmetric CSR graph from anywhere (numpy arrays; columns ascending, no diagonal, a >= 0): a SpectralResult"""
    _need(backend in ("device", "numpy"), "backend is 'device' or 'numpy', got %r" % (backend,))
    check_solver(n_components, diffusion_time, tol, max_steps, random_state, on_disconnected)
    check_alpha(alpha)
    indptr, indices, a = check_graph(indptr, indices, a)
    n = len(indptr) - 1
    if backend == "numpy":
        a = _density_numpy(indptr, indices, a, alpha)
        root = components_numpy(indptr, indices)
        return _embed(lambda rows: _NumpyOperator(*_sub_numpy(indptr, indices, a, rows, n)), root, n_components, diffusion_time, drop_first,
                      tol, max_steps, random_state, on_disconnected)
    import torch
    D = _Device(torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(D.dev):
        ip, ix, av = (torch.from_numpy(np.ascontiguousarray(v)).to(D.dev) for v in (indptr, indices, a))
        av = D.density(ip, ix, av, alpha)
        root = D.components(ip, ix)
        return _embed(lambda rows: _DeviceOperator(D, *_sub_device(D, ip, ix, av, rows, n)), root, n_components, diffusion_time,
                      drop_first, tol, max_steps, random_state, on_disconnected)


def embedding(X, n_components=2, n_neighbors=15, affinity="connectivity", local_scale=7, alpha=0.0, diffusion_time=0.0, drop_first=True,
              tol=1e-10, max_steps=1024, random_state=0, on_disconnected="largest", backend="device"):
    """the spectral embedding of X [n][d] by the rules at the top of this module: a SpectralResult.  backend="device" takes a
    contiguous float32 CUDA tensor (a numpy array is copied)."""
    X = _graph_input(X, n_neighbors, affinity, local_scale, alpha, backend)
    check_solver(n_components, diffusion_time, tol, max_steps, random_state, on_disconnected)
    n = int(X.shape[0])
    if backend == "numpy":
        indptr, indices, a, root = _graph_numpy(X, n_neighbors, affinity, local_scale, alpha)
        return _embed(lambda rows: _NumpyOperator(*_sub_numpy(indptr, indices, a, rows, n)), root, n_components, diffusion_time, drop_first,
                      tol, max_steps, random_state, on_disconnected)
    D, indptr, indices, a, root = _graph_device(X, n_neighbors, affinity, local_scale, alpha)
    with D.torch.cuda.device(D.dev):
        return _embed(lambda rows: _DeviceOperator(D, *_sub_device(D, indptr, indices, a, rows, n)), root, n_components, diffusion_time,
                      drop_first, tol, max_steps, random_state, on_disconnected)


def cluster(X, n_clusters, n_neighbors=15, affinity="connectivity", local_scale=7, alpha=0.0, diffusion_time=0.0, tol=1e-10,
            max_steps=1024, random_state=0, on_disconnected="largest", backend="device", **kmeans_kwargs):
    """rule 10: a SpectralClusterResult (labels, embedding, kmeans).  random_state also seeds k-means unless kmeans_kwargs has one."""
    from . import kmeans
    _need(is_int(n_clusters) and 2 <= n_clusters <= MAX_COMPONENTS, "need an integer 2 <= n_clusters <= %d, got %r" % (MAX_COMPONENTS, n_clusters))
    X = _graph_input(X, n_neighbors, affinity, local_scale, alpha, backend)
    emb = embedding(X, n_clusters, n_neighbors, affinity, local_scale, alpha, diffusion_time, False, tol, max_steps, random_state,
                    on_disconnected, backend)
    E = np.ascontiguousarray(emb.embedding[emb.rows], np.float32)
    if backend == "device":
        E = _common.to_device(E, X.device.index)
    kmeans_kwargs.setdefault("random_state", random_state)
    km = kmeans.kmeans(E, n_clusters, backend=backend, **kmeans_kwargs)
    labels = np.full(len(emb.component), -1, np.int32)
    labels[emb.rows] = km.labels
    return SpectralClusterResult(labels, emb, km)


def dense_numpy(indptr, indices, a, n_components, alpha=0.0, diffusion_time=0.0, drop_first=True):
    """the literal definition on a CONNECTED graph, for tests and pins (n <= 4000): numpy.linalg.eigh of the dense M.  Returns
    (embedding [n][c], theta [c], Y [c][n] (the unit eigenvectors behind the columns, without the constant one), spectrum [n]
    (every eigenvalue of M, descending; spectrum[0] is the trivial 1))."""
    indptr, indices, a = check_graph(indptr, indices, a)
    n = len(indptr) - 1
    _need(n <= MAX_DENSE_N, "dense_numpy takes n <= %d rows, got %d" % (MAX_DENSE_N, n))
    check_solver(n_components, diffusion_time)
    check_alpha(alpha)
    _need(len(np.unique(components_numpy(indptr, indices))) == 1, "dense_numpy takes a connected graph")
    _need(n >= n_components + 2, "need n >= n_components + 2")
    op = _NumpyOperator(indptr, indices, _density_numpy(indptr, indices, a, alpha))
    M = np.zeros((n, n))
    M[op.rows, op.indices] = op.val
    lam, U = np.linalg.eigh(M)
    lam, U = lam[::-1], U[:, ::-1]
    c = n_components if drop_first else n_components - 1
    Y, theta = np.ascontiguousarray(U[:, 1:1 + c].T), lam[1:1 + c].copy()
    E, theta_out, _ = _finish(Y, theta, np.zeros(c), op.s, op.deg, diffusion_time, drop_first)
    return E, theta_out, Y, lam.copy()


# ---- command line

def main(argv=None):
    from . import kmeans
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.spectral")
    _common.add_cluster_arguments(ap, ("input", "output"), "factors", True)
    ap.add_argument("--n_components", type=int, default=2)
    ap.add_argument("--n_neighbors", type=int, default=15, help="sklearn's n_neighbors: the row itself and n_neighbors - 1 others")
    ap.add_argument("--affinity", default="connectivity", choices=("connectivity", "gaussian"))
    ap.add_argument("--local_scale", type=int, default=7, help="the neighbour whose distance is sigma_i (gaussian)")
    ap.add_argument("--alpha", type=float, default=0.0, help="density normalisation: 0 none, 1 Laplace-Beltrami")
    ap.add_argument("--diffusion_time", type=float, default=0.0, help="column t is multiplied by max(theta_t, 0)^tau")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max_steps", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0, help="random_state of the start vector (and of k-means with --k)")
    ap.add_argument("--on_disconnected", default="largest", choices=("largest", "error"))
    ap.add_argument("--k", type=int, default=None, help="also cluster: k-means on the k-column embedding (spectral clustering)")
    ap.add_argument("--quality", type=int, nargs="?", const=10, default=None, metavar="K",
                    help="trustworthiness and continuity of the embedded rows at K neighbours (default 10)")
    _common.add_cluster_arguments(ap, ("--key", "--backend", "--truth", "--stack", "--params", "--ou", "--averages", "--device"), "factors", True)
    args = ap.parse_args(argv)
    if (args.truth or args.averages) and args.k is None:
        ap.error("--truth and --averages need --k")
    _common.check_averages_arguments(ap, args)
    if args.quality is not None and args.quality < 1:
        ap.error("--quality K is an integer >= 1")
    try:
        check_solver(args.n_components, args.diffusion_time, args.tol, args.max_steps, args.seed, args.on_disconnected)
        check_alpha(args.alpha)
        if args.k is not None:
            _need(2 <= args.k <= MAX_COMPONENTS, "need 2 <= --k <= %d, got %d" % (MAX_COMPONENTS, args.k))
            check_solver(args.k, args.diffusion_time, args.tol, args.max_steps, args.seed, args.on_disconnected)
        _need(args.n_neighbors >= 2, "need --n_neighbors >= 2, got %d" % args.n_neighbors)
        if args.affinity == "gaussian":
            _need(1 <= args.local_scale <= args.n_neighbors - 1, "need 1 <= --local_scale <= n_neighbors - 1, got %d" % args.local_scale)
    except SpectralError as e:
        ap.error(str(e))
    try:
        X = kmeans.read_input(args.input, args.key)
        n, d = X.shape
        check_domain(n, d, args.n_neighbors, args.affinity, args.local_scale, args.alpha)
        truth = kmeans.read_truth(args.truth, n) if args.truth else None
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device" or args.averages:
        _common.require_gpu(_common.NO_GPU)
    kw = dict(n_neighbors=args.n_neighbors, affinity=args.affinity, local_scale=args.local_scale, alpha=args.alpha,
              diffusion_time=args.diffusion_time, tol=args.tol, max_steps=args.max_steps, random_state=args.seed,
              on_disconnected=args.on_disconnected, backend=args.backend)
    clu = None
    try:
        Xb = _common.to_device(X, args.device) if args.backend == "device" else X
        res = embedding(Xb, args.n_components, **kw)
        if args.k is not None:
            clu = cluster(Xb, args.k, **kw)
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    out = dict(embedding=res.embedding, eigenvalues=res.eigenvalues, laplacian_eigenvalues=res.laplacian_eigenvalues,
               residuals=res.residuals, component=res.component, n_steps=np.int64(res.n_steps), converged=np.bool_(res.converged),
               n_dropped=np.int64(res.n_dropped), n_components=np.int64(args.n_components), n_neighbors=np.int64(args.n_neighbors),
               affinity=np.str_(args.affinity), local_scale=np.int64(args.local_scale), alpha=np.float64(args.alpha),
               diffusion_time=np.float64(args.diffusion_time), tol=np.float64(args.tol), max_steps=np.int64(args.max_steps),
               seed=np.int64(args.seed), on_disconnected=np.str_(args.on_disconnected), key=np.str_(args.key), backend=np.str_(args.backend),
               k=np.int64(-1 if args.k is None else args.k))
    msg = "%s: %d points x %d -> %d components, %d of %d rows embedded, %d Lanczos steps%s, largest residual %.3g" % (
        args.output, n, d, res.embedding.shape[1], len(res.rows), n, res.n_steps, "" if res.converged else " (NOT converged)",
        float(res.residuals.max()))
    if args.quality is not None:
        from . import quality
        try:
            Xq, Yq = X[res.rows], np.ascontiguousarray(res.embedding[res.rows], np.float32)
            if args.backend == "device":
                Xq, Yq = _common.to_device(Xq, args.device), _common.to_device(Yq, args.device)
            q = quality.embedding_quality(Xq, Yq, args.quality, backend=args.backend)
        except ValueError as e:
            raise SystemExit("error: %s" % e)
        out["trustworthiness"], out["continuity"] = np.float64(q.trustworthiness), np.float64(q.continuity)
        out["quality_neighbors"] = np.int64(args.quality)
        msg += ", trustworthiness %.4f, continuity %.4f" % (q.trustworthiness, q.continuity)
    if clu is not None:
        km = clu.kmeans
        out["labels"], out["centers"], out["inertia"] = clu.labels, km.centers, np.float64(km.inertia)
        keep = clu.labels >= 0
        msg += ", %d classes, inertia %.6g" % (args.k, km.inertia)
        if truth is not None:
            msg += _common.truth_scores(out, truth, clu.labels, keep)
        if args.averages:
            msg += _common.write_averages(args, n, clu.labels, args.k, keep, SpectralError, MAX_AVERAGES)
    np.savez(args.output, **out)
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
