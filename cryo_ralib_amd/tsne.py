"""t-SNE of factors X [n][d] on the GPU (notebook 03's embedding step; scikit-learn 1.7 TSNE with method="barnes_hut", angle=0).

    python -m cryo_ralib_amd.tsne IN OUT.npz [--key factors] [--perplexity 30] [--early_exaggeration 12] [--learning_rate auto]
                                  [--max_iter 1000] [--init pca|random|FILE.npy] [--seed S] [--backend device|numpy]

The contract is sklearn's TSNE(method="barnes_hut", angle=0.0, n_components=2, metric="euclidean"): with angle 0 the tree is
walked to its leaves, so it computes sparse kNN affinities plus the exact all-pairs repulsion, which is what runs here.
  Affinities: k = min(n - 1, int(3 perplexity + 1)) nearest neighbours (itself excluded, by (squared distance, index)), the
  conditional P of each row by sklearn's _binary_search_perplexity, P = (P_c + P_c^T) / max(sum, eps), CSR with sorted columns.
  Gradient: grad_i = 4 (sum_nbr e p_ij w_ij (y_i - y_j) - sum_{j != i} w_ij^2 (y_i - y_j) / Z), w_ij = 1 / (1 + |y_i - y_j|^2),
  Z = sum_{i != j} w_ij; e = early_exaggeration for the first 250 iterations, then 1.
  Error: sum over the stored entries of e p_ij log(max(e p_ij, tiny) / max(w_ij / Z, tiny)), tiny = float32's smallest normal.
  Optimiser: sklearn's _gradient_descent, run twice as sklearn's _tsne does (250 iterations at momentum 0.5 with exaggeration,
  then to max_iter at momentum 0.8; each run starts with zero update and unit gains), checking the error and the gradient norm
  every 50 iterations.  n_iter is sklearn's n_iter_ (the last iteration index run).

The kNN, the perplexity search and every iteration run in the HIP kernels behind ra_tsne_* (csrc/ralign_tsne.h); symmetrising P
(once per call) is torch plumbing on the device.  The host syncs only at the checks.  backend="numpy" runs the same loop in float64
numpy, chunking the all-pairs step: it is the CPU checker.

Domain: 2 <= n <= 262144, 1 <= d <= 2048, 0 < perplexity <= 100 and perplexity < n, max_iter >= 250, n_components = 2; init "pca"
needs d >= 2.  Anything else raises TsneError before anything is launched; so does non-finite input.

Out-of-sample placement (transform, tsne_large; the tool's --fit_size and --place_into): new rows X_new [n][d] are placed into a
fixed embedding Y_fit [m][2] of fitted rows X_fit [m][d] (any embedding of X_fit, normally tsne()'s).  Each new point interacts
with the fitted points only, so the work is n m pairs per iteration and batches without limit.  The rules:
  1. Neighbours.  k = min(m, int(3 perplexity + 1)).  For new row i the k fitted rows of least D2(i, j) = sum_t (xnew_it -
     xfit_jt)^2, formed in double from the differences of the float32 values with the features in order, ordered by (D2, j).  No
     row is excluded: a new row equal to a fitted row lists it first at distance 0.
  2. Affinities.  p_i. = binary_search_perplexity(D2 row, perplexity), each row searched on its own (the fit's rule and kernel).
     No symmetrisation and no global normalisation.  The device rounds p to float32 once.
  3. Objective, per point.  w_ij = 1 / (1 + |y_i - Y_j|^2), Z_i = sum_{j < m} w_ij over every fitted point, KL_i = sum_{j in N(i)}
     p_ij log(max(p_ij, tiny) / max(w_ij / Z_i, tiny)), tiny = float32's smallest normal.  The normalisation is per point, so a
     point's result does not depend on which other points were placed with it.
  4. Gradient.  g_i = 4 (e sum_{j in N(i)} p_ij w_ij (y_i - Y_j) - sum_{j < m} w_ij^2 (y_i - Y_j) / Z_i).  |w d| <= 1/2, sum p <= 1
     and the repulsion is a weighted mean of w d, so |g_i|_inf <= 2 (e + 1): nothing is clipped.
  5. Start.  init="weighted": y_i = sum_j p_ij Y_N(i,j) in double in list order, rounded to float32; init="nearest": Y of the
     first neighbour; or an [n][2] array.
  6. Optimiser.  Exactly n_iter iterations of the fit's rule from update = 0 and gains = 1: inc = update g < 0; gains = inc ?
     gains + 0.2 : gains 0.8, floored at 0.01; update = momentum update - learning_rate gains g; y += update.  No checks, no early
     stop, no host sync inside the loop.  Defaults: perplexity 30, learning_rate 0.1, momentum 0.8, exaggeration e = 1, n_iter 250.
  7. Independence and determinism.  Everything returned for point i is a function of (x_i, X_fit, Y_fit, parameters) alone,
     bitwise the same whatever n, the batch size, the point's position in the batch or the stream.  No floating-point atomics;
     every sum over j runs in an order fixed by m (and k) only.
  8. Label vote (vote_labels).  score_i(c) = sum_{j: label = c} p_ij in double in list order over the fitted points' integer
     labels (-1, noise, counts as a label); the label is the largest score, the lowest label on ties; the confidence is the
     winning score.
Rules 1, 2 and 3-6 run in ra_tsne_knn_query, ra_tsne_affinity_rows and ra_tsne_place (one launch for all iterations); rules 5 and
8 are torch and numpy plumbing.  backend="numpy" is the float64 checker, chunked, without a GPU.  Domain: X_fit and Y_fit agree in
m, X_new and X_fit in d; 2 <= m <= 262144, 1 <= d <= 2048, 0 < perplexity <= 100 and perplexity < m, n >= 0 (n = 0 returns empty
arrays without a launch), batch <= 262144, finite input; tsne_large: 2 <= fit_size <= min(n, 262144), n <= 4194304.

    python -m cryo_ralib_amd.tsne IN OUT.npz --fit_size M [--seed S] ...            fit M drawn rows, place the rest (tsne_large)
    python -m cryo_ralib_amd.tsne IN OUT.npz --place_into FIT_OUT.npz --fit_input FILE [--fit_key factors] ...
    both: [--place_iter 250] [--place_lr 0.1] [--place_exaggeration 1] [--place_perplexity P] [--batch 65536] [--fit_labels FILE]

Every mode takes --quality [K] (default 10) [--quality_sample N]: trustworthiness, continuity, trust_point and cont_point of the
written embedding against the input rows (quality.embedding_quality) join OUT.npz; more than 262144 rows need --quality_sample (the
drawn rows, by --seed, are stored as quality_sample_indices).
"""
import argparse
import collections
import math
import sys

import numpy as np

from . import _common, _graph
from ._common import Launcher, ptr
from .sdr import fix_signs

N_ITER_CHECK = 50          # sklearn TSNE._N_ITER_CHECK
EXPLORATION_ITER = 250     # sklearn TSNE._EXPLORATION_MAX_ITER
MACHINE_EPSILON = np.finfo(np.double).eps
FLOAT32_TINY = float(np.finfo(np.float32).tiny)
MAX_N, MAX_D = 262144, 2048


class TsneError(ValueError):
    """an input outside the supported domain"""


class TsneResult:
    """embedding [n][2] float32, kl_divergence (sklearn's kl_divergence_), n_iter (sklearn's n_iter_), errors (the KL at each
    check, float64)"""

    def __init__(self, embedding, kl_divergence, n_iter, errors):
        self.embedding, self.kl_divergence, self.n_iter, self.errors = embedding, kl_divergence, n_iter, errors


def n_neighbors(n, perplexity):
    """sklearn's neighbour count for n points"""
    return min(n - 1, int(3.0 * perplexity + 1))


def check_domain(n, d, perplexity=30.0, max_iter=1000, n_components=2, early_exaggeration=12.0, learning_rate="auto"):
    """raise TsneError unless the shape and parameters are inside the supported domain"""
    def need(ok, msg):
        if not ok:
            raise TsneError(msg)
    for name, v in (("n", n), ("d", d), ("max_iter", max_iter), ("n_components", n_components)):
        need(isinstance(v, (int, np.integer)) and not isinstance(v, bool), "%s must be an integer, got %r" % (name, v))
    need(2 <= n <= MAX_N, "need 2 <= n <= %d points, got %d" % (MAX_N, n))
    need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    need(n_components == 2, "only n_components = 2 is built, got %d" % n_components)
    need(isinstance(perplexity, (int, float, np.number)) and 0 < perplexity <= 100, "need 0 < perplexity <= 100, got %r" % (perplexity,))
    need(perplexity < n, "perplexity (%g) must be less than the number of points (%d)" % (perplexity, n))
    need(max_iter >= EXPLORATION_ITER, "need max_iter >= %d, got %d" % (EXPLORATION_ITER, max_iter))
    need(isinstance(early_exaggeration, (int, float, np.number)) and early_exaggeration >= 1,
         "need early_exaggeration >= 1, got %r" % (early_exaggeration,))
    need(learning_rate == "auto" or (isinstance(learning_rate, (int, float, np.number)) and math.isfinite(learning_rate)
                                     and learning_rate > 0), "learning_rate is 'auto' or a number > 0, got %r" % (learning_rate,))


def resolve_learning_rate(learning_rate, n, early_exaggeration):
    """sklearn: 'auto' is max(n / early_exaggeration / 4, 50)"""
    if learning_rate == "auto":
        return float(np.maximum(n / early_exaggeration / 4, 50))
    return float(learning_rate)


def check_random_state(seed):
    """sklearn.utils.check_random_state; a bool counts as the integer it is"""
    return _common.check_random_state(int(seed) if isinstance(seed, bool) else seed, TsneError)


def random_init(n, random_state=None):
    """sklearn's init="random": 1e-4 standard normals in float32, drawn from check_random_state(random_state)"""
    return 1e-4 * check_random_state(random_state).standard_normal(size=(n, 2)).astype(np.float32)


def _scale_pca(F):
    F = np.asarray(F, np.float32)
    return F / np.std(F[:, 0]) * 1e-4


# ---- CPU checker (float64 numpy)

def knn_numpy(X, k):
    """(idx [n][k] int64, dist2 [n][k] float64): float64 brute force, itself excluded, ordered by (squared distance, index).  A Gram
    screen plus a re-rank, as the kernel: apart from knn_query_numpy and quality.knn_numpy, which form difference chains only."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    nrm = np.einsum("ij,ij->i", X, X)
    C = min(n - 1, k + 32)
    idx = np.empty((n, k), np.int64)
    d2 = np.empty((n, k), np.float64)
    ch = max(1, (1 << 22) // max(n, 1))
    for s in range(0, n, ch):
        e = min(n, s + ch)
        D = nrm[s:e, None] + nrm[None, :] - 2.0 * (X[s:e] @ X.T)
        D[np.arange(e - s), np.arange(s, e)] = np.inf
        cand = np.argsort(D, axis=1, kind="stable")[:, :C]
        for r in range(e - s):
            c = cand[r]
            ex = np.sum((X[s + r] - X[c]) ** 2, axis=1)
            o = np.lexsort((c, ex))[:k]
            idx[s + r], d2[s + r] = c[o], ex[o]
    return idx, d2


def binary_search_perplexity(dist2, perplexity):
    """sklearn's _binary_search_perplexity (_utils.pyx) on [n][k] squared distances, all rows at once, in double"""
    D = np.asarray(dist2, np.float32).astype(np.float64)
    n = D.shape[0]
    desired = math.log(float(np.float32(perplexity)))
    tol, floor_sum = float(np.float32(1e-5)), float(np.float32(1e-8))
    beta = np.ones(n)
    bmin = np.full(n, -np.inf)
    bmax = np.full(n, np.inf)
    P = np.zeros_like(D)
    live = np.ones(n, bool)
    for _ in range(100):
        r = np.nonzero(live)[0]
        if r.size == 0:
            break
        p = np.exp(-D[r] * beta[r, None])
        s = p.sum(axis=1)
        s[s == 0.0] = floor_sum
        p /= s[:, None]
        P[r] = p
        diff = np.log(s) + beta[r] * np.sum(D[r] * p, axis=1) - desired
        done = np.abs(diff) <= tol
        up = ~done & (diff > 0)
        dn = ~done & ~(diff > 0)
        ru, rd = r[up], r[dn]
        bmin[ru] = beta[ru]
        beta[ru] = np.where(bmax[ru] == np.inf, beta[ru] * 2.0, (beta[ru] + bmax[ru]) / 2.0)
        bmax[rd] = beta[rd]
        beta[rd] = np.where(bmin[rd] == -np.inf, beta[rd] / 2.0, (beta[rd] + bmin[rd]) / 2.0)
        live[r[done]] = False
    return P


def _symmetrize_numpy(idx, pcond):
    indptr, indices, a, b = _graph.symmetrize_numpy(idx, pcond)
    v = a + b
    return indptr, indices, v / max(float(np.sum(v)), MACHINE_EPSILON)


def gradient_numpy(Y, csr, exaggeration=1.0):
    """(KL error, gradient [n][2]) at Y in float64: the contract's formulas, the all-pairs part in chunks of rows"""
    Y = np.asarray(Y, np.float64)
    indptr, indices, P = csr
    n = Y.shape[0]
    rep = np.zeros((n, 2))
    Z = 0.0
    ch = max(1, (1 << 21) // n)
    for s in range(0, n, ch):
        e = min(n, s + ch)
        D = Y[s:e, None, :] - Y[None, :, :]
        w = 1.0 / (1.0 + np.sum(D * D, axis=2))
        w[np.arange(e - s), np.arange(s, e)] = 0.0
        Z += float(np.sum(w))
        rep[s:e] = np.einsum("ij,ijk->ik", w * w, D)
    Z = max(Z, MACHINE_EPSILON)
    rows = _graph.row_ids_numpy(indptr)
    D = Y[rows] - Y[indices]
    w = 1.0 / (1.0 + np.sum(D * D, axis=1))
    pe = exaggeration * np.asarray(P, np.float64)
    f = (pe * w)[:, None] * D
    attr = np.stack([np.bincount(rows, f[:, 0], n), np.bincount(rows, f[:, 1], n)], axis=1)
    err = float(np.sum(pe * np.log(np.maximum(pe, FLOAT32_TINY) / np.maximum(w / Z, FLOAT32_TINY))))
    return err, 4.0 * (attr - rep / Z)


class _NumpyState:
    """float64 state of the optimiser"""

    def __init__(self, Y, csr):
        self.y = np.array(Y, np.float64)
        self.csr = csr

    def reset(self):
        self.update = np.zeros_like(self.y)
        self.gains = np.ones_like(self.y)

    def step(self, exaggeration, momentum, learning_rate, want):
        err, grad = gradient_numpy(self.y, self.csr, exaggeration)
        inc = self.update * grad < 0.0
        self.gains[inc] += 0.2
        self.gains[~inc] *= 0.8
        np.clip(self.gains, 0.01, np.inf, out=self.gains)
        grad *= self.gains
        self.update = momentum * self.update - learning_rate * grad
        self.y += self.update
        return (err, float(np.sum(grad * grad))) if want else None

    def embedding(self):
        return self.y.astype(np.float32)


# ---- device

class _Device(Launcher):
    """thin launcher of the ra_tsne_* entries on the current stream of a device; the lists come from _graph.knn / knn_query"""

    def affinity(self, d2, perplexity):
        n, k = (int(s) for s in d2.shape)
        pc = self.torch.empty((n, k), dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_affinity", ptr(d2), n, k, float(perplexity), ptr(pc))
        return pc

    def symmetrize(self, idx, pc):
        """CSR of (P_c + P_c^T) / max(sum, eps) on the device"""
        torch = self.torch
        indptr, indices, a, b = _graph.symmetrize_torch(idx, pc)
        v = a + b
        v = v / torch.clamp(v.sum(), min=MACHINE_EPSILON)
        return indptr.to(torch.int32), indices.to(torch.int32), v

    def gradient(self, y, indptr, indices, p32, exaggeration):
        n = int(y.shape[0])
        g = self.torch.empty((n, 2), dtype=self.torch.float32, device=self.dev)
        st = self.torch.empty(2, dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_error", ptr(y), n, ptr(indptr), ptr(indices), ptr(p32), int(p32.numel()), float(exaggeration), ptr(g), ptr(st))
        return float(st[0].item()), g

    def affinity_rows(self, d2, perplexity):
        rows, k = (int(s) for s in d2.shape)
        pc = self.torch.empty((rows, k), dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_affinity_rows", ptr(d2), rows, k, float(perplexity), ptr(pc))
        return pc

    def place_gradient(self, y, yfit, idx, p32, exaggeration=1.0):
        """(grad [n][2] float32, KL_i [n] float64, Z_i [n] float64) at y, as device tensors"""
        n, k = (int(s) for s in idx.shape)
        g = self.torch.empty((n, 2), dtype=self.torch.float32, device=self.dev)
        kl = self.torch.empty(n, dtype=self.torch.float64, device=self.dev)
        z = self.torch.empty(n, dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_place_gradient", ptr(y), n, ptr(yfit), int(yfit.shape[0]), ptr(idx), ptr(p32), k, float(exaggeration),
                  ptr(g), ptr(kl), ptr(z))
        return g, kl, z

    def place(self, y, yfit, idx, p32, exaggeration, momentum, learning_rate, n_iter):
        """n_iter iterations in place on y; returns KL_i [n] at the final y"""
        n, k = (int(s) for s in idx.shape)
        kl = self.torch.empty(n, dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_place", ptr(y), n, ptr(yfit), int(yfit.shape[0]), ptr(idx), ptr(p32), k, float(exaggeration),
                  float(momentum), float(learning_rate), int(n_iter), ptr(kl))
        return kl


class _DeviceState:
    """float32 state of the optimiser on the device: two embedding buffers (a step reads every y_j while it writes)"""

    def __init__(self, D, Y, indptr, indices, p32):
        torch = D.torch
        self.D, self.n = D, int(Y.shape[0])
        self.y = Y.contiguous().clone()
        self.y2 = torch.empty_like(self.y)
        self.update = torch.zeros_like(self.y)
        self.gains = torch.ones_like(self.y)
        self.indptr, self.indices, self.p = indptr, indices, p32
        self.stats = torch.empty(2, dtype=torch.float64, device=D.dev)

    def reset(self):
        self.update.zero_()
        self.gains.fill_(1.0)

    def step(self, exaggeration, momentum, learning_rate, want):
        self.D.call("ra_tsne_step", ptr(self.y), ptr(self.y2), ptr(self.update), ptr(self.gains), self.n, ptr(self.indptr),
                    ptr(self.indices), ptr(self.p), int(self.p.numel()), float(exaggeration), float(momentum), float(learning_rate),
                    ptr(self.stats) if want else None)
        self.y, self.y2 = self.y2, self.y
        if not want:
            return None
        s = self.stats.cpu().numpy()
        return float(s[0]), float(s[1])

    def embedding(self):
        return self.y.cpu().numpy()


# ---- the loop (sklearn _tsne / _gradient_descent)

def _optimise(state, max_iter, early_exaggeration, learning_rate, n_iter_without_progress, min_grad_norm):
    errors = []

    def descend(it, stop, momentum, exaggeration, without_progress):
        state.reset()
        error = best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, stop):
            check = (i + 1) % N_ITER_CHECK == 0
            st = state.step(exaggeration, momentum, learning_rate, check or i == stop - 1)
            if st is not None:
                error = st[0]
            if check:
                errors.append(error)
                grad_norm = math.sqrt(st[1])
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > without_progress:
                    break
                if grad_norm <= min_grad_norm:
                    break
        return error, i

    error, it = descend(0, EXPLORATION_ITER, 0.5, early_exaggeration, EXPLORATION_ITER)
    if it < EXPLORATION_ITER or max_iter - EXPLORATION_ITER > 0:
        error, it = descend(it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    return float(error), int(it), np.asarray(errors, np.float64)


def affinities(X, perplexity=30.0, backend="device"):
    """(indptr [n + 1], indices, P float64) of the symmetric joint probabilities, as numpy arrays"""
    X = _common.as_input(X, backend, TsneError, numpy_on_device=False)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, perplexity)
    _common.check_finite(X, backend, TsneError)
    k = n_neighbors(n, perplexity)
    if backend == "numpy":
        idx, d2 = knn_numpy(X, k)
        return _symmetrize_numpy(idx, binary_search_perplexity(d2, perplexity))
    import torch
    with torch.cuda.device(X.device):
        D = _Device(X.device)
        idx, d2 = _graph.knn(D, X, k)
        indptr, indices, P = D.symmetrize(idx, D.affinity(d2, perplexity))
        return indptr.cpu().numpy().astype(np.int64), indices.cpu().numpy().astype(np.int64), P.cpu().numpy()


def knn(X, k, backend="device"):
    """(idx [n][k], dist2 [n][k] float64) of the k nearest neighbours of every row, as numpy arrays"""
    X = _common.as_input(X, backend, TsneError, numpy_on_device=False)
    n, d = (int(s) for s in X.shape)
    if not (2 <= n <= MAX_N and 1 <= d <= MAX_D and 1 <= k <= min(n - 1, 301)):
        raise TsneError("need 2 <= n <= %d, 1 <= d <= %d and 1 <= k <= min(n - 1, 301)" % (MAX_N, MAX_D))
    if backend == "numpy":
        return knn_numpy(X, k)
    import torch
    with torch.cuda.device(X.device):
        idx, d2 = _graph.knn(Launcher(X), X, k)
        return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()


def _pca_init_numpy(X):
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = fix_signs(V[:, np.argsort(w, kind="stable")[::-1][:2]])
    return _scale_pca(Xc @ V)


def _pca_init_device(X, D):
    """top two principal axes from ra_sdr_mean / ra_sdr_gram (form 0, p = 1) and a float64 eigh, projected by ra_sdr_factors"""
    from . import sdr
    torch = D.torch
    n, d = (int(s) for s in X.shape)
    mean = torch.empty(d, dtype=torch.float32, device=D.dev)
    D.call("ra_sdr_mean", ptr(X), n, 1, d, ptr(mean))
    g = torch.empty((d, d), dtype=torch.float64, device=D.dev)
    D.call("ra_sdr_gram", ptr(X), n, 1, d, ptr(mean), 0, None, 0, ptr(g))
    _, V = sdr.top_eig(g.cpu().numpy(), 2)
    Vd = torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(D.dev)
    F = torch.empty((n, 2), dtype=torch.float32, device=D.dev)
    D.call("ra_sdr_factors", ptr(X), n, d, ptr(Vd), 2, ptr(F))
    shift = mean.cpu().numpy().astype(np.float64) @ V            # (x - mean) V = x V - mean V
    return _scale_pca(F.cpu().numpy().astype(np.float64) - shift)


def initial_embedding(X, init="pca", random_state=None, backend="device"):
    """the [n][2] float32 start of the optimisation (sklearn's init)"""
    X = _common.as_input(X, backend, TsneError, numpy_on_device=False)
    n, d = (int(s) for s in X.shape)
    if isinstance(init, str):
        if init == "random":
            return random_init(n, random_state)
        if init != "pca":
            raise TsneError("init is 'pca', 'random' or an [n][2] array, got %r" % (init,))
        if d < 2:
            raise TsneError("init 'pca' needs d >= 2 features (two principal axes), got d = %d" % d)
        if backend == "numpy":
            return _pca_init_numpy(X)
        import torch
        with torch.cuda.device(X.device):
            return _pca_init_device(X, _Device(X.device))
    Y = np.asarray(init.detach().cpu().numpy() if hasattr(init, "detach") else init, np.float32)
    if Y.shape != (n, 2):
        raise TsneError("an init array is [n][2] = [%d][2], got %s" % (n, Y.shape))
    if not np.all(np.isfinite(Y)):
        raise TsneError("the init array holds NaN or infinite values")
    return Y


def tsne(X, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300,
         min_grad_norm=1e-7, init="pca", random_state=None, n_components=2, backend="device"):
    """t-SNE of X [n][d]: TsneResult(embedding [n][2] float32, kl_divergence, n_iter, errors)"""
    X = _common.as_input(X, backend, TsneError, numpy_on_device=False)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, perplexity, max_iter, n_components, early_exaggeration, learning_rate)
    _common.check_finite(X, backend, TsneError)
    lr = resolve_learning_rate(learning_rate, n, early_exaggeration)
    Y0 = initial_embedding(X, init, random_state, backend)
    k = n_neighbors(n, perplexity)
    if backend == "numpy":
        idx, d2 = knn_numpy(X, k)
        csr = _symmetrize_numpy(idx, binary_search_perplexity(d2, perplexity))
        state = _NumpyState(Y0, csr)
        err, it, errors = _optimise(state, max_iter, early_exaggeration, lr, n_iter_without_progress, min_grad_norm)
        return TsneResult(state.embedding(), err, it, errors)
    import torch
    with torch.cuda.device(X.device):
        D = _Device(X.device)
        idx, d2 = _graph.knn(D, X, k)
        indptr, indices, P = D.symmetrize(idx, D.affinity(d2, perplexity))
        state = _DeviceState(D, torch.from_numpy(Y0).to(X.device), indptr, indices, P.to(torch.float32))
        err, it, errors = _optimise(state, max_iter, early_exaggeration, lr, n_iter_without_progress, min_grad_norm)
        return TsneResult(state.embedding(), err, it, errors)


def step(Y, csr, update, gains, exaggeration, momentum, learning_rate, backend="device"):
    """one iteration of the optimiser from the given state: (Y', update', gains', KL error at Y, squared norm of the gained
    gradient), as numpy arrays; csr = (indptr, indices, P) as affinities() returns it"""
    if backend == "numpy":
        st = _NumpyState(Y, csr)
        st.update, st.gains = np.array(update, np.float64), np.array(gains, np.float64)
        err, gn = st.step(exaggeration, momentum, learning_rate, True)
        return st.y, st.update, st.gains, err, gn
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    D = _Device(dev)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    st = _DeviceState(D, f32(Y), i32(csr[0]), i32(csr[1]), f32(csr[2]))
    st.update, st.gains = f32(update), f32(gains)
    err, gn = st.step(exaggeration, momentum, learning_rate, True)
    return st.embedding(), st.update.cpu().numpy(), st.gains.cpu().numpy(), err, gn


def gradient(Y, csr, exaggeration=1.0, backend="device"):
    """(KL error, gradient [n][2]) at Y: ra_tsne_error on the device, gradient_numpy on the CPU"""
    if backend == "numpy":
        return gradient_numpy(Y, csr, exaggeration)
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    D = _Device(dev)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    err, g = D.gradient(f32(Y), i32(csr[0]), i32(csr[1]), f32(csr[2]), exaggeration)
    return err, g.cpu().numpy()


def trustworthiness(X, Y, n_neighbors=10):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors) (euclidean), restated in numpy"""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    n = X.shape[0]
    if n_neighbors >= n / 2:
        raise TsneError("n_neighbors (%d) should be less than n_samples / 2 (%g)" % (n_neighbors, n / 2))

    def dists(A):
        nrm = np.einsum("ij,ij->i", A, A)
        D = np.sqrt(np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * (A @ A.T), 0.0))
        np.fill_diagonal(D, np.inf)
        return D
    ind_X = np.argsort(dists(X), axis=1)
    ind_Y = np.argsort(dists(Y), axis=1, kind="stable")[:, :n_neighbors]
    inverted = np.zeros((n, n), dtype=np.int64)
    ordered = np.arange(n + 1)
    inverted[ordered[:-1, None], ind_X] = ordered[1:]
    ranks = inverted[ordered[:-1, None], ind_Y] - n_neighbors
    t = np.sum(ranks[ranks > 0])
    return float(1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0))))


# ---- out-of-sample placement (rules 1 - 8 of the module's text)

MAX_NEW, MAX_BATCH = 4194304, 262144
TransformDetails = collections.namedtuple("TransformDetails", "embedding kl kl_init idx p")
LargeResult = collections.namedtuple("LargeResult", "embedding fit_indices kl_point fit")


def n_neighbors_query(m, perplexity):
    """rule 1's neighbour count for m fitted points"""
    return min(m, int(3.0 * perplexity + 1))


def check_transform_domain(n, m, d, perplexity=30.0, learning_rate=0.1, momentum=0.8, exaggeration=1.0, n_iter=250, batch=65536):
    """raise TsneError unless the shapes and parameters of a placement are inside the supported domain"""
    def need(ok, msg):
        if not ok:
            raise TsneError(msg)
    for name, v in (("n", n), ("m", m), ("d", d), ("n_iter", n_iter), ("batch", batch)):
        need(_common.is_int(v), "%s must be an integer, got %r" % (name, v))
    need(n >= 0, "need n >= 0 new points, got %d" % n)
    need(2 <= m <= MAX_N, "need 2 <= m <= %d fitted points, got %d" % (MAX_N, m))
    need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    need(_common.is_real(perplexity) and 0 < perplexity <= 100, "need 0 < perplexity <= 100, got %r" % (perplexity,))
    need(perplexity < m, "perplexity (%g) must be less than the number of fitted points (%d)" % (perplexity, m))
    need(_common.is_real(learning_rate) and learning_rate > 0, "need a finite learning_rate > 0, got %r" % (learning_rate,))
    need(_common.is_real(momentum) and 0 <= momentum < 1, "need 0 <= momentum < 1, got %r" % (momentum,))
    need(_common.is_real(exaggeration) and exaggeration >= 1, "need a finite exaggeration >= 1, got %r" % (exaggeration,))
    need(n_iter >= 0, "need n_iter >= 0, got %d" % n_iter)
    need(1 <= batch <= MAX_BATCH, "need 1 <= batch <= %d, got %d" % (MAX_BATCH, batch))


def knn_query_numpy(Q, X, k):
    """rule 1 in float64: (idx [nq][k] int64, dist2 [nq][k]) of the k rows of X nearest each row of Q, by (distance, index).
    Difference chains, nothing left out: apart from quality.knn_numpy, which leaves the row itself out and returns no distances."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    nq, m = Q.shape[0], X.shape[0]
    idx = np.empty((nq, k), np.int64)
    d2 = np.empty((nq, k), np.float64)
    ch = max(1, (1 << 22) // m)
    for s in range(0, nq, ch):
        e = min(nq, s + ch)
        D = np.zeros((e - s, m))
        for t in range(X.shape[1]):
            df = Q[s:e, t, None] - X[None, :, t]
            D += df * df
        o = np.argsort(D, axis=1, kind="stable")[:, :k]
        idx[s:e], d2[s:e] = o, np.take_along_axis(D, o, axis=1)
    return idx, d2


def place_gradient_numpy(y, Y_fit, idx, p, exaggeration=1.0, dtype=np.float64, want_kl=True):
    """rules 3 and 4 at y: (gradient [n][2], KL_i [n] or None, Z_i [n]) in `dtype`, the all-pairs part in chunks of rows; list
    entries outside 0 .. m - 1 are skipped"""
    y, Y_fit, p = np.asarray(y, dtype), np.asarray(Y_fit, dtype), np.asarray(p, dtype)
    idx = np.asarray(idx, np.int64)
    n, m = y.shape[0], Y_fit.shape[0]
    Z = np.empty(n, dtype)
    rep = np.empty((n, 2), dtype)
    ch = max(1, (1 << 21) // m)
    for s in range(0, n, ch):
        e = min(n, s + ch)
        dx, dy = y[s:e, 0, None] - Y_fit[None, :, 0], y[s:e, 1, None] - Y_fit[None, :, 1]
        w = 1 / (1 + (dx * dx + dy * dy))
        Z[s:e] = w.sum(axis=1)
        w *= w
        rep[s:e, 0], rep[s:e, 1] = (w * dx).sum(axis=1), (w * dy).sum(axis=1)
    ok = (idx >= 0) & (idx < m)
    j = np.where(ok, idx, 0)
    pv = np.where(ok, p, 0).astype(dtype)
    dx, dy = y[:, 0, None] - Y_fit[j, 0], y[:, 1, None] - Y_fit[j, 1]
    w = 1 / (1 + (dx * dx + dy * dy))
    f = pv * w
    attr = np.stack([(f * dx).sum(axis=1), (f * dy).sum(axis=1)], axis=1)
    kl = None
    if want_kl:
        tiny = dtype(FLOAT32_TINY)
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = (pv * np.log(np.maximum(pv, tiny) / np.maximum(w / Z[:, None], tiny))).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = 4 * (dtype(exaggeration) * attr - rep / Z[:, None])
    return grad, kl, Z


def place_numpy(y0, Y_fit, idx, p, exaggeration=1.0, momentum=0.8, learning_rate=0.1, n_iter=250, dtype=np.float64):
    """rule 6 in `dtype` numpy: (y [n][2], KL_i [n] at the final y)"""
    y = np.array(y0, dtype)
    update, gains = np.zeros_like(y), np.ones_like(y)
    for _ in range(n_iter):
        g = place_gradient_numpy(y, Y_fit, idx, p, exaggeration, dtype, want_kl=False)[0]
        gains = np.maximum(np.where(update * g < 0, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
        update = dtype(momentum) * update - dtype(learning_rate) * (gains * g)
        y = y + update
    return y, place_gradient_numpy(y, Y_fit, idx, p, 1.0, dtype)[1]


def _check_init(init, n):
    if isinstance(init, str):
        if init not in ("weighted", "nearest"):
            raise TsneError("init is 'weighted', 'nearest' or an [n][2] array, got %r" % (init,))
        return init
    Y = np.asarray(init.detach().cpu().numpy() if hasattr(init, "detach") else init, np.float32)
    if Y.shape != (n, 2):
        raise TsneError("an init array is [n][2] = [%d][2], got %s" % (n, Y.shape))
    if not np.all(np.isfinite(Y)):
        raise TsneError("the init array holds NaN or infinite values")
    return Y


def initial_placement_numpy(init, Y_fit, idx, p):
    """rule 5: the [n][2] float32 start; init is "weighted", "nearest" or the rows of an init array"""
    if not isinstance(init, str):
        return np.asarray(init, np.float32)
    Y = np.asarray(Y_fit, np.float64)
    if init == "nearest":
        return Y[idx[:, 0]].astype(np.float32)
    acc = np.zeros((idx.shape[0], 2))
    for j in range(idx.shape[1]):
        acc = acc + np.asarray(p[:, j, None], np.float64) * Y[idx[:, j]]
    return acc.astype(np.float32)


def _initial_placement_device(torch, init, Y_fit, idx, p32):
    """rule 5 on the device: the same sum, one list column at a time in float64 (a product and an addition, nothing fused)"""
    if not isinstance(init, str):
        return torch.from_numpy(np.ascontiguousarray(init, np.float32)).to(Y_fit.device)
    if init == "nearest":
        return Y_fit[idx[:, 0].long()].contiguous()
    Y = Y_fit.double()
    acc = torch.zeros((idx.shape[0], 2), dtype=torch.float64, device=Y_fit.device)
    for j in range(int(idx.shape[1])):
        acc = acc + p32[:, j, None].double() * Y[idx[:, j].long()]
    return acc.float().contiguous()


def knn_query(Q, X, k, backend="device"):
    """rule 1: (idx [nq][k], dist2 [nq][k] float64) of the k rows of X [m][d] nearest every row of Q [nq][d], as numpy arrays"""
    Q = _common.as_input(Q, backend, TsneError)
    X = _common.as_input(X, backend, TsneError)
    (nq, d), (m, dx) = (int(s) for s in Q.shape), (int(s) for s in X.shape)
    if not (_common.is_int(k) and 1 <= nq <= MAX_NEW and 1 <= m <= MAX_N and 1 <= d <= MAX_D and d == dx and 1 <= k <= min(m, 301)):
        raise TsneError("need 1 <= nq <= %d, 1 <= m <= %d, Q and X of the same 1 <= d <= %d and 1 <= k <= min(m, 301)"
                        % (MAX_NEW, MAX_N, MAX_D))
    if backend == "numpy":
        return knn_query_numpy(np.asarray(Q, np.float32), np.asarray(X, np.float32), k)
    import torch
    with torch.cuda.device(X.device):
        idx, d2 = _graph.knn_query(Launcher(X), Q, X, k)
        return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()


def transform(X_new, X_fit, Y_fit, perplexity=30.0, learning_rate=0.1, momentum=0.8, exaggeration=1.0, n_iter=250, init="weighted",
              batch=65536, backend="device", details=False):
    """Place X_new [n][d] into the embedding Y_fit [m][2] of X_fit [m][d] (rules 1 - 7): the embedding [n][2] float32, or with
    details TransformDetails(embedding, kl [n] (KL_i at the end), kl_init [n] (at the start), idx [n][k], p [n][k]), as numpy
    arrays.  backend="device": X_fit and Y_fit are contiguous float32 CUDA tensors (numpy arrays are copied to the current
    device) and the work runs on the current stream; X_new is such a tensor too, or a numpy array of any size, which is copied one
    batch at a time so that only a batch's lists live on the device."""
    if backend not in ("device", "numpy"):
        raise TsneError("backend is 'device' or 'numpy', got %r" % (backend,))
    host_new = backend == "numpy" or isinstance(X_new, np.ndarray)
    Xn = _common.as_input(X_new, "numpy" if host_new else "device", TsneError, numpy_on_device=False)
    Xf, Yf = _common.as_input(X_fit, backend, TsneError), _common.as_input(Y_fit, backend, TsneError)
    if backend == "numpy":
        Xf, Yf = np.ascontiguousarray(Xf, np.float32), np.ascontiguousarray(Yf, np.float32)
    elif Yf.device != Xf.device or not (host_new or Xn.device == Xf.device):
        raise TsneError("X_new, X_fit and Y_fit are on different devices")
    (n, d), m = (int(s) for s in Xn.shape), int(Xf.shape[0])
    if tuple(Yf.shape) != (m, 2):
        raise TsneError("Y_fit is [m][2] = [%d][2], got %s" % (m, tuple(Yf.shape)))
    if int(Xf.shape[1]) != d:
        raise TsneError("X_new has %d features, X_fit %d" % (d, int(Xf.shape[1])))
    check_transform_domain(n, m, d, perplexity, learning_rate, momentum, exaggeration, n_iter, batch)
    init = _check_init(init, n)
    _common.check_finite(Xf, backend, TsneError)
    _common.check_finite(Yf, backend, TsneError)
    if not (_common.host_finite(Xn) if host_new else bool(Xn.isfinite().all().item())):
        raise TsneError("X holds NaN or infinite values")
    k = n_neighbors_query(m, perplexity)
    emb, kl = np.empty((n, 2), np.float32), np.empty(n, np.float64)
    if details:
        kl0, idx_all, p_all = np.empty(n, np.float64), np.empty((n, k), np.int64), np.empty((n, k), np.float64)

    def run(torch=None, D=None):
        for s in range(0, n, batch):
            e = min(n, s + batch)
            y0 = init if isinstance(init, str) else init[s:e]
            if D is None:
                idx, d2 = knn_query_numpy(np.asarray(Xn[s:e], np.float32), Xf, k)
                p = binary_search_perplexity(d2, perplexity)
                y0 = initial_placement_numpy(y0, Yf, idx, p)
                if details:
                    kl0[s:e] = place_gradient_numpy(y0, Yf, idx, p)[1]
                y, kl[s:e] = place_numpy(y0, Yf, idx, p, exaggeration, momentum, learning_rate, n_iter)
                emb[s:e] = y.astype(np.float32)
            else:
                xb = torch.from_numpy(np.ascontiguousarray(Xn[s:e], np.float32)).to(D.dev) if host_new else Xn[s:e]
                idx, d2 = _graph.knn_query(D, xb, Xf, k)
                p = D.affinity_rows(d2, perplexity).to(torch.float32)
                y = _initial_placement_device(torch, y0, Yf, idx, p)
                if details:
                    kl0[s:e] = D.place_gradient(y, Yf, idx, p)[1].cpu().numpy()
                kl[s:e] = D.place(y, Yf, idx, p, exaggeration, momentum, learning_rate, n_iter).cpu().numpy()
                emb[s:e] = y.cpu().numpy()
            if details:
                idx_all[s:e] = idx if D is None else idx.cpu().numpy()
                p_all[s:e] = p if D is None else p.cpu().numpy()

    if backend == "numpy":
        run()
    elif n:
        import torch
        with torch.cuda.device(Xf.device):
            run(torch, _Device(Xf.device))
    return TransformDetails(emb, kl, kl0, idx_all, p_all) if details else emb


def affinities_query(X_new, X_fit, perplexity=30.0, batch=65536, backend="device"):
    """rules 1 and 2 alone: (idx [n][k] int64, p [n][k] float64; on the device p holds float32 values) of the rows of X_new (a
    numpy array, copied a batch at a time) against X_fit, as numpy arrays: what vote_labels needs for rows that were not placed"""
    X_new = np.asarray(X_new)
    Xf = _common.as_input(X_fit, backend, TsneError)
    (n, d), m = X_new.shape, int(Xf.shape[0])
    check_transform_domain(n, m, d, perplexity, batch=batch)
    k = n_neighbors_query(m, perplexity)
    idx_all, p_all = np.empty((n, k), np.int64), np.empty((n, k), np.float64)
    if backend == "device" and n:
        import torch
        D = _Device(Xf.device)
    for s in range(0, n, batch):
        xb = np.ascontiguousarray(X_new[s:s + batch], np.float32)
        if backend == "numpy":
            idx_all[s:s + batch], d2 = knn_query_numpy(xb, Xf, k)
            p_all[s:s + batch] = binary_search_perplexity(d2, perplexity)
        else:
            with torch.cuda.device(Xf.device):
                idx, d2 = _graph.knn_query(D, torch.from_numpy(xb).to(D.dev), Xf, k)
                idx_all[s:s + batch] = idx.cpu().numpy()
                p_all[s:s + batch] = D.affinity_rows(d2, perplexity).to(torch.float32).cpu().numpy()
    return idx_all, p_all


def vote_labels(idx, p, labels_fit):
    """rule 8: (labels [n] int32, confidence [n] float64) of the new points from their neighbour lists idx [n][k], p [n][k] and the
    fitted points' integer labels [m]; list entries outside 0 .. m - 1 are skipped"""
    idx, p, labels_fit = np.asarray(idx), np.asarray(p, np.float64), np.asarray(labels_fit)
    if labels_fit.ndim != 1 or labels_fit.size < 1 or not np.issubdtype(labels_fit.dtype, np.integer):
        raise TsneError("labels_fit is [m] integers, got %s %s" % (labels_fit.dtype, labels_fit.shape))
    if idx.ndim != 2 or idx.shape != p.shape or not np.issubdtype(idx.dtype, np.integer):
        raise TsneError("idx [n][k] (integers) and p [n][k] must agree, got %s %s and %s" % (idx.dtype, idx.shape, p.shape))
    classes, inv = np.unique(labels_fit, return_inverse=True)
    n, m = idx.shape[0], labels_fit.shape[0]
    score = np.zeros((n, classes.size))
    rows = np.arange(n)
    for j in range(idx.shape[1]):
        ok = (idx[:, j] >= 0) & (idx[:, j] < m)
        score[rows[ok], inv[idx[ok, j]]] += p[ok, j]
    best = np.argmax(score, axis=1)                         # the first maximum: the lowest label on ties
    return classes[best].astype(np.int32), score[rows, best]


def draw_fit_rows(n, fit_size, random_state=None):
    """the sorted fit rows of tsne_large: check_random_state(random_state).permutation(n)[:fit_size]"""
    return np.sort(check_random_state(random_state).permutation(n)[:fit_size])


def check_large_domain(n, fit_size):
    if not (_common.is_int(n) and _common.is_int(fit_size) and 2 <= fit_size <= min(n, MAX_N) and n <= MAX_NEW):
        raise TsneError("need 2 <= fit_size <= min(n, %d) and n <= %d, got fit_size = %r, n = %r" % (MAX_N, MAX_NEW, fit_size, n))


def tsne_large(X, fit_size, random_state=None, transform_kwargs=None, **tsne_kwargs):
    """t-SNE of any n <= 4194304 rows: tsne() on fit_size drawn rows (draw_fit_rows; random_state also seeds the fit), transform()
    for the rest; fitted rows keep their fitted positions.  LargeResult(embedding [n][2] float32, fit_indices, kl_point [n] (KL_i
    of the placed rows, nan on fitted rows), fit (the TsneResult)).  The backend is tsne_kwargs' (default "device": X is a CUDA
    tensor, or a numpy array whose rows are copied as they are used)."""
    backend = tsne_kwargs.get("backend", "device")
    host = backend == "numpy" or isinstance(X, np.ndarray)
    X = _common.as_input(X, "numpy" if host else "device", TsneError, numpy_on_device=False)
    n = int(X.shape[0])
    check_large_domain(n, fit_size)
    fit_idx = draw_fit_rows(n, fit_size, random_state)
    rest = np.setdiff1d(np.arange(n), fit_idx)
    if host:
        Xf, Xr = np.ascontiguousarray(X[fit_idx], np.float32), X[rest]
        if backend == "device":
            import torch
            Xf = torch.from_numpy(Xf).to(torch.device("cuda", torch.cuda.current_device()))
    else:
        import torch
        Xf, Xr = X[torch.from_numpy(fit_idx).to(X.device)].contiguous(), X[torch.from_numpy(rest).to(X.device)].contiguous()
    fit = tsne(Xf, random_state=random_state, **tsne_kwargs)
    if backend == "device":
        with torch.cuda.device(Xf.device):                 # the fitted embedding is copied to the device of the rows
            placed = transform(Xr, Xf, fit.embedding, details=True, **(transform_kwargs or {}))
    else:
        placed = transform(Xr, Xf, fit.embedding, backend=backend, details=True, **(transform_kwargs or {}))
    emb, kl = np.empty((n, 2), np.float32), np.full(n, np.nan)
    emb[fit_idx], emb[rest], kl[rest] = fit.embedding, placed.embedding, placed.kl
    return LargeResult(emb, fit_idx, kl, fit)


# ---- command line

def read_input(path, key="factors"):
    """[n][d] float32 from an .npz (key) or an .npy"""
    return _common.read_input(path, key, TsneError)


def read_fit_labels(path):
    """[m] integer labels from an int .npy, or the `labels` of an .npz of the dbscan, hdbscan, kmeans or gmm tool"""
    try:
        if path.endswith(".npz"):
            with np.load(path) as z:
                if "labels" not in z.files:
                    raise TsneError("%s has no array 'labels' (it holds %s)" % (path, ", ".join(z.files)))
                y = z["labels"]
        else:
            y = np.load(path)
    except (OSError, ValueError) as e:
        raise TsneError("%s: %s" % (path, e))
    if y.ndim != 1 or not np.issubdtype(y.dtype, np.integer):
        raise TsneError("%s: need [m] integers, got %s %s" % (path, y.dtype, y.shape))
    return y


def _check_quality(ap, args, n):
    """--quality's usage errors (status 2, before the device is touched)"""
    if args.quality is not None:
        from . import quality
        quality.check_tool_arguments(ap, n, n, args.quality, args.quality_sample)


def _add_quality(out, args, X, backend):
    """--quality: the four scores of out["embedding"] against the rows X into out; returns their part of the summary line"""
    if args.quality is None:
        return ""
    from . import quality
    try:
        q = quality.embedding_quality(X, out["embedding"], args.quality, args.quality_sample, args.seed, backend)
    except quality.QualityError as e:
        raise TsneError("--quality: %s" % e)
    out.update(trustworthiness=np.float64(q.trustworthiness), continuity=np.float64(q.continuity), trust_point=q.trust_point,
               cont_point=q.cont_point)
    if q.sample_indices is not None:
        out["quality_sample_indices"] = q.sample_indices
    return ", trustworthiness %.6f, continuity %.6f (k = %d)" % (q.trustworthiness, q.continuity, args.quality)


def _main_place(ap, args):
    """the tool's --fit_size and --place_into modes.  Usage errors leave through ap.error (status 2) before the device is touched"""
    if args.fit_size is not None and args.place_into is not None:
        ap.error("--fit_size and --place_into are two modes: give one of them")
    if args.place_into is not None and args.fit_input is None:
        ap.error("--place_into needs --fit_input (the rows its embedding was fitted on)")
    if args.fit_size is not None and args.fit_input is not None:
        ap.error("--fit_input goes with --place_into")
    try:
        X = read_input(args.input, args.key)
        labels_fit = read_fit_labels(args.fit_labels) if args.fit_labels else None
        lr = args.learning_rate if args.learning_rate == "auto" else float(args.learning_rate)
        init = args.init if args.init in ("pca", "random") else np.load(args.init)
        perplexity = args.perplexity
        if args.place_into is not None:
            Xf = read_input(args.fit_input, args.fit_key)
            with np.load(args.place_into) as z:
                if "embedding" not in z.files:
                    raise TsneError("%s has no array 'embedding' (it holds %s)" % (args.place_into, ", ".join(z.files)))
                Yf = np.ascontiguousarray(z["embedding"], np.float32)
                perplexity = float(z["perplexity"]) if "perplexity" in z.files else perplexity
    except (TsneError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    n, d = X.shape
    _check_quality(ap, args, n)
    if args.place_into is not None:
        m = Xf.shape[0]
        if Yf.shape != (m, 2):
            ap.error("%s holds an embedding %s, %s has %d rows" % (args.place_into, Yf.shape, args.fit_input, m))
        if Xf.shape[1] != d:
            ap.error("%s has %d features, %s %d" % (args.input, d, args.fit_input, Xf.shape[1]))
    else:
        m = args.fit_size
        try:
            check_large_domain(n, m)
        except TsneError as e:
            ap.error("--fit_size: %s" % e)
    if labels_fit is not None and labels_fit.shape[0] != m:
        ap.error("%s holds %d labels for %d fitted rows" % (args.fit_labels, labels_fit.shape[0], m))
    kw = dict(perplexity=perplexity if args.place_perplexity is None else args.place_perplexity,
              learning_rate=0.1 if args.place_lr is None else args.place_lr,
              exaggeration=1.0 if args.place_exaggeration is None else args.place_exaggeration,
              n_iter=250 if args.place_iter is None else args.place_iter, batch=65536 if args.batch is None else args.batch)
    try:
        check_transform_domain(n, m, d, kw["perplexity"], kw["learning_rate"], 0.8, kw["exaggeration"], kw["n_iter"], kw["batch"])
        if args.fit_size is not None:
            check_domain(m, d, args.perplexity, args.max_iter, 2, args.early_exaggeration, lr)
    except TsneError as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device":
        _common.require_gpu("no GPU visible: use --backend numpy for the CPU checker")

    def run():
        out = {}
        if args.fit_size is not None:
            res = tsne_large(X, m, random_state=args.seed, transform_kwargs=kw, perplexity=args.perplexity,
                             early_exaggeration=args.early_exaggeration, learning_rate=lr, max_iter=args.max_iter, init=init,
                             backend=args.backend)
            fit, fit_rows = res.fit, X[res.fit_indices]
            out.update(embedding=res.embedding, kl_divergence=np.float64(fit.kl_divergence), n_iter=np.int64(fit.n_iter),
                       errors=fit.errors, perplexity=np.float64(args.perplexity),
                       early_exaggeration=np.float64(args.early_exaggeration),
                       learning_rate=np.float64(resolve_learning_rate(lr, m, args.early_exaggeration)),
                       max_iter=np.int64(args.max_iter), init=np.str_(args.init),
                       seed=np.int64(-1 if args.seed is None else args.seed), backend=np.str_(args.backend),
                       fit_indices=res.fit_indices, kl_point=res.kl_point)
        else:
            placed = transform(X, Xf, Yf, backend=args.backend, details=True, **kw)
            out.update(embedding=placed.embedding, kl_point=placed.kl)
        if labels_fit is not None:
            # every row votes, the fitted ones too (each lists itself first at distance 0)
            idx, p = ((placed.idx, placed.p) if args.fit_size is None else
                      affinities_query(X, fit_rows, kw["perplexity"], kw["batch"], args.backend))
            out["labels"], out["label_confidence"] = vote_labels(idx, p, labels_fit)
        out["_quality"] = _add_quality(out, args, X, args.backend)
        return out
    try:
        if args.backend == "device":
            import torch
            with torch.cuda.device(args.device):
                out = run()
        else:
            out = run()
    except TsneError as e:
        raise SystemExit("error: %s" % e)
    tail = out.pop("_quality")
    np.savez(args.output, **out)
    kl = out["kl_point"][np.isfinite(out["kl_point"])]
    print("%s: %d points x %d placed against %d fitted, mean KL_i %.6f%s" % (args.output, kl.size, d, m,
                                                                          float(kl.mean()) if kl.size else float("nan"), tail))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.tsne")
    ap.add_argument("input", help="OUT.npz of python -m cryo_ralib_amd.sdr, or an [n][d] .npy")
    ap.add_argument("output", help="OUT.npz")
    ap.add_argument("--key", default="factors", help="array of an .npz input (default factors)")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--early_exaggeration", type=float, default=12.0)
    ap.add_argument("--learning_rate", default="auto", help="'auto' or a number")
    ap.add_argument("--max_iter", type=int, default=1000)
    ap.add_argument("--init", default="pca", help="pca, random or an [n][2] .npy")
    ap.add_argument("--seed", type=int, default=None, help="random_state of init random")
    ap.add_argument("--backend", default="device", choices=("device", "numpy"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fit_size", type=int, default=None, help="fit this many drawn rows (--seed) and place the rest into their "
                    "embedding; the only mode that takes more than %d rows" % MAX_N)
    ap.add_argument("--place_into", default=None, help="OUT.npz of an earlier run: place the input's rows into its embedding")
    ap.add_argument("--fit_input", default=None, help="the rows the embedding of --place_into was fitted on (.npz or .npy)")
    ap.add_argument("--fit_key", default="factors", help="array of an .npz --fit_input (default factors)")
    ap.add_argument("--place_iter", type=int, default=None, help="iterations of the placement (default 250)")
    ap.add_argument("--place_lr", type=float, default=None, help="learning rate of the placement (default 0.1)")
    ap.add_argument("--place_exaggeration", type=float, default=None, help="exaggeration of the placement (default 1)")
    ap.add_argument("--place_perplexity", type=float, default=None, help="perplexity of the placement (default: the fit's)")
    ap.add_argument("--batch", type=int, default=None, help="new rows on the device at a time (default 65536)")
    ap.add_argument("--fit_labels", default=None, help="int .npy, or OUT.npz of the dbscan, hdbscan, kmeans or gmm tool (its labels), "
                    "one label per fitted row: adds labels and label_confidence of every row by the neighbour vote")
    ap.add_argument("--quality", type=int, nargs="?", const=10, default=None, metavar="K",
                    help="add trustworthiness, continuity, trust_point and cont_point at K neighbours (default 10) to OUT.npz")
    ap.add_argument("--quality_sample", type=int, default=None, metavar="N",
                    help="evaluate --quality on N drawn rows (--seed); needed above %d rows" % MAX_N)
    args = ap.parse_args(argv)
    if args.quality_sample is not None and args.quality is None:
        ap.error("--quality_sample needs --quality")
    if args.fit_size is not None or args.place_into is not None:
        return _main_place(ap, args)
    given = [o for o in ("fit_input", "place_iter", "place_lr", "place_exaggeration", "place_perplexity", "batch", "fit_labels")
             if getattr(args, o) is not None]
    if given:
        ap.error("--%s needs --fit_size or --place_into" % given[0])
    try:
        X = read_input(args.input, args.key)
        lr = args.learning_rate if args.learning_rate == "auto" else float(args.learning_rate)
        init = args.init if args.init in ("pca", "random") else np.load(args.init)
        check_domain(X.shape[0], X.shape[1], args.perplexity, args.max_iter, 2, args.early_exaggeration, lr)
    except (TsneError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    _check_quality(ap, args, X.shape[0])
    if args.backend == "device":
        _common.require_gpu("no GPU visible: use --backend numpy for the CPU checker")
    x = _common.to_device(X, args.device) if args.backend == "device" else X

    def run():
        res = tsne(x, args.perplexity, args.early_exaggeration, lr, args.max_iter, init=init, random_state=args.seed,
                   backend=args.backend)
        out = dict(embedding=res.embedding, kl_divergence=np.float64(res.kl_divergence), n_iter=np.int64(res.n_iter),
                   errors=res.errors, perplexity=np.float64(args.perplexity), early_exaggeration=np.float64(args.early_exaggeration),
                   learning_rate=np.float64(resolve_learning_rate(lr, X.shape[0], args.early_exaggeration)),
                   max_iter=np.int64(args.max_iter), init=np.str_(args.init), seed=np.int64(-1 if args.seed is None else args.seed),
                   backend=np.str_(args.backend))
        return res, out, _add_quality(out, args, x, args.backend)
    try:
        if args.backend == "device":
            import torch
            with torch.cuda.device(x.device):
                res, out, tail = run()
        else:
            res, out, tail = run()
    except TsneError as e:
        raise SystemExit("error: %s" % e)
    np.savez(args.output, **out)
    print("%s: %d points x %d, %d iterations, KL %.6f%s" % (args.output, X.shape[0], X.shape[1], res.n_iter, res.kl_divergence, tail))
    return 0


if __name__ == "__main__":
    sys.exit(main())
