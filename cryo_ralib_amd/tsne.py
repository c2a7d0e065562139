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
"""
import argparse
import math
import sys

import numpy as np

from . import _common
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
    """(idx [n][k] int64, dist2 [n][k] float64): float64 brute force, itself excluded, ordered by (squared distance, index)"""
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


def _symmetrize_numpy(idx, pcond, n):
    k = idx.shape[1]
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1).astype(np.int64)
    keys = np.concatenate([rows * n + cols, cols * n + rows])
    vals = np.concatenate([pcond.reshape(-1), pcond.reshape(-1)])
    o = np.argsort(keys, kind="stable")
    keys, vals = keys[o], vals[o]
    uk, start, counts = np.unique(keys, return_index=True, return_counts=True)
    v = vals[start] + np.where(counts == 2, vals[np.minimum(start + 1, len(vals) - 1)], 0.0)
    v = v / max(float(np.sum(v)), MACHINE_EPSILON)
    indptr = np.searchsorted(uk // n, np.arange(n + 1)).astype(np.int64)
    return indptr, (uk % n).astype(np.int64), v


def _csr_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


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
    rows = _csr_rows(indptr)
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

class _Device:
    """thin launcher of the ra_tsne_* entries on the current stream of X's device"""

    def __init__(self, dev):
        L = Launcher(dev)
        self.torch, self.api, self.lib, self.dev, self.stream, self.call = L.torch, L.api, L.lib, L.dev, L.stream, L.call

    def knn(self, X, k):
        n, d = (int(s) for s in X.shape)
        idx = self.torch.empty((n, k), dtype=self.torch.int32, device=self.dev)
        d2 = self.torch.empty((n, k), dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_knn", ptr(X), n, d, k, ptr(idx), ptr(d2))
        return idx, d2

    def affinity(self, d2, perplexity):
        n, k = (int(s) for s in d2.shape)
        pc = self.torch.empty((n, k), dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_affinity", ptr(d2), n, k, float(perplexity), ptr(pc))
        return pc

    def symmetrize(self, idx, pc):
        """CSR of (P_c + P_c^T) / max(sum, eps) on the device: a stable sort of the keys i n + j, then the (at most two) entries of
        each key added; deterministic (no scatter)"""
        torch = self.torch
        n, k = (int(s) for s in idx.shape)
        rows = torch.arange(n, device=self.dev, dtype=torch.int64).repeat_interleave(k)
        cols = idx.reshape(-1).to(torch.int64)
        keys = torch.cat([rows * n + cols, cols * n + rows])
        vals = torch.cat([pc.reshape(-1), pc.reshape(-1)])
        keys, order = torch.sort(keys, stable=True)
        vals = vals[order]
        uk, counts = torch.unique_consecutive(keys, return_counts=True)
        start = torch.cumsum(counts, 0) - counts
        second = vals[torch.clamp(start + 1, max=vals.numel() - 1)]
        v = vals[start] + torch.where(counts == 2, second, torch.zeros_like(second))
        v = v / torch.clamp(v.sum(), min=MACHINE_EPSILON)
        indptr = torch.searchsorted(uk // n, torch.arange(n + 1, device=self.dev, dtype=torch.int64))
        return indptr.to(torch.int32), (uk % n).to(torch.int32), v

    def gradient(self, y, indptr, indices, p32, exaggeration):
        n = int(y.shape[0])
        g = self.torch.empty((n, 2), dtype=self.torch.float32, device=self.dev)
        st = self.torch.empty(2, dtype=self.torch.float64, device=self.dev)
        self.call("ra_tsne_error", ptr(y), n, ptr(indptr), ptr(indices), ptr(p32), int(p32.numel()), float(exaggeration), ptr(g), ptr(st))
        return float(st[0].item()), g


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
        return _symmetrize_numpy(idx, binary_search_perplexity(d2, perplexity), n)
    import torch
    with torch.cuda.device(X.device):
        D = _Device(X.device)
        idx, d2 = D.knn(X, k)
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
        idx, d2 = _Device(X.device).knn(X, k)
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
        csr = _symmetrize_numpy(idx, binary_search_perplexity(d2, perplexity), n)
        state = _NumpyState(Y0, csr)
        err, it, errors = _optimise(state, max_iter, early_exaggeration, lr, n_iter_without_progress, min_grad_norm)
        return TsneResult(state.embedding(), err, it, errors)
    import torch
    with torch.cuda.device(X.device):
        D = _Device(X.device)
        idx, d2 = D.knn(X, k)
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


# ---- command line

def read_input(path, key="factors"):
    """[n][d] float32 from an .npz (key) or an .npy"""
    return _common.read_input(path, key, TsneError)


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
    args = ap.parse_args(argv)
    try:
        X = read_input(args.input, args.key)
        lr = args.learning_rate if args.learning_rate == "auto" else float(args.learning_rate)
        init = args.init if args.init in ("pca", "random") else np.load(args.init)
        check_domain(X.shape[0], X.shape[1], args.perplexity, args.max_iter, 2, args.early_exaggeration, lr)
    except (TsneError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device":
        _common.require_gpu("no GPU visible: use --backend numpy for the CPU checker")
    x = _common.to_device(X, args.device) if args.backend == "device" else X
    try:
        if args.backend == "device":
            import torch
            with torch.cuda.device(x.device):
                res = tsne(x, args.perplexity, args.early_exaggeration, lr, args.max_iter, init=init, random_state=args.seed)
        else:
            res = tsne(x, args.perplexity, args.early_exaggeration, lr, args.max_iter, init=init, random_state=args.seed,
                       backend="numpy")
    except TsneError as e:
        raise SystemExit("error: %s" % e)
    np.savez(args.output, embedding=res.embedding, kl_divergence=np.float64(res.kl_divergence), n_iter=np.int64(res.n_iter),
             errors=res.errors, perplexity=np.float64(args.perplexity), early_exaggeration=np.float64(args.early_exaggeration),
             learning_rate=np.float64(resolve_learning_rate(lr, X.shape[0], args.early_exaggeration)),
             max_iter=np.int64(args.max_iter), init=np.str_(args.init), seed=np.int64(-1 if args.seed is None else args.seed),
             backend=np.str_(args.backend))
    print("%s: %d points x %d, %d iterations, KL %.6f" % (args.output, X.shape[0], X.shape[1], res.n_iter, res.kl_divergence))
    return 0


if __name__ == "__main__":
    sys.exit(main())
