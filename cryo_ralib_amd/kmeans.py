"""k-means of factors X [n][d] on the GPU, with class averages (scikit-learn 1.7 KMeans(algorithm="lloyd"), uniform weights).

    python -m cryo_ralib_amd.kmeans IN OUT.npz --k K [--key factors] [--init k-means++|random|FILE.npy] [--n_init auto|N]
                                    [--max_iter 300] [--tol 1e-4] [--seed S] [--backend device|numpy] [--truth FILE]
                                    [--stack STACK --params PARAMS --ou R --averages REFS.{hdf,mrcs,npy}]
                                    [--scores] [--sweep K1,K2,...|LO:HI[:STEP]] [--sample_size N]

IN is the OUT.npz of the sdr tool (--key factors) or of the tsne tool (--key embedding), or an [n][d] .npy.  --truth takes an int
.npy or a params.txt (its class column); OUT.npz then also holds purity, c_purity and contingency.  --averages writes the k class
averages of the stack (rot_shift2D by PARAMS, then the multi-reference loop's reference update): a refstack for the
multi-reference command line.

The contract is sklearn's KMeans(algorithm="lloyd") with uniform sample weights:
  Seeding: init="k-means++" is _kmeans_plusplus with n_local_trials = 2 + int(log(k)): the first centre
  random_state.choice(n, p=ones/n); every later one draws random_state.uniform(size=n_local_trials) * current_pot, takes the
  candidates np.searchsorted(cumsum(closest_dist_sq), rand_vals) clipped to n - 1, and keeps the first one of least potential
  sum_i min(closest_i, d^2(x_i, cand)).  init="random" is random_state.choice(n, size=k, replace=False, p=ones/n); init may be a
  [k][d] array.  random_state as sklearn's check_random_state.  The draws happen on the host in sklearn's order; the potentials,
  the cumulative sum and the search run on the device.
  n_init: "auto" is 1 for k-means++ or an array, 10 for random; the runs draw from one RandomState in turn, and a run replaces
  the best only if inertia < best and the clustering differs (_is_same_clustering).
  Lloyd (_kmeans_single_lloyd): E-step label = argmin_c |x - c|^2 (first index on ties), M-step member means, empty clusters
  relocated as _relocate_empty_clusters_dense (farthest points in decreasing distance, ties by lower index; none when every
  point sits on its centre), a cluster still empty placed on the heaviest one as _average_centers does, stop on strict
  convergence (labels unchanged) or when sum_c |c_new - c_old|^2 <= mean(var(X, axis=0)) * tol; without strict convergence one
  more E-step.  inertia = sum_i |x_i - c_label|^2; n_iter is sklearn's n_iter_.
Not built: sample_weight, algorithm="elkan", sparse input; sklearn's internal mean-centring (it changes rounding only).

Every distance, sum and update runs in the HIP kernels behind ra_kmeans_* (csrc/ralign_kmeans.h); the host reads the changed-label
count and the centre shift once per iteration and the potential once per seeded centre.  backend="numpy" runs the same loop in
float64 numpy: it is the CPU checker.  contingency_matrix, purity_score and c_purity_score restate the reference's utils_ralib
(sklearn is not a run-time dependency).

Cluster validity without ground truth (sklearn.metrics with metric="euclidean"): silhouette_samples,
silhouette_score (with sklearn's sample_size / random_state subsample), calinski_harabasz_score, davies_bouldin_score, validity
(all of them and the per-class silhouette) and sweep (k-means and the scores for every k of a list; best_k is the largest
silhouette, the smaller k on ties).  Only clusters with members count; their number m must satisfy 2 <= m <= n - 1 (ValueError
with sklearn's message otherwise).  The silhouette's n^2 distances come from ra_kmeans_silhouette (f32 differences, double sums),
the centroids and dispersions from ra_kmeans_dispersion; the silhouette takes 3 <= n <= 262144 and 2 <= k <= 256, more points
only with sample_size <= 262144.  --scores adds silhouette, class_silhouette, silhouette_samples (nan outside the sample),
calinski_harabasz and davies_bouldin to OUT.npz and prints one line per class; --sweep makes --k optional, prints the table
k / inertia / silhouette / CH / DB, stores it as sweep (and best_k) and writes the result of best_k, or of --k if given.

Domain: 1 <= k <= min(256, n), 1 <= n <= 4194304, 1 <= d <= 2048, max_iter >= 1, tol >= 0, finite input.  Anything else raises
KMeansError before anything is launched.
"""
import argparse
import math
import numbers
import sys
import warnings

import numpy as np

from . import _common
from ._common import Launcher, is_int, ptr

MAX_N, MAX_D, MAX_K = 4194304, 2048, 256


class KMeansError(ValueError):
    """an input outside the supported domain"""


class ConvergenceWarning(UserWarning):
    """sklearn's warning class for fewer distinct clusters than asked for"""


class KMeansResult:
    """labels int32 [n], centers float64 [k][d], inertia, n_iter (sklearn's n_iter_), init_indices (the rows of X the kept run
    started from; None for an init array)"""

    def __init__(self, labels, centers, inertia, n_iter, init_indices):
        self.labels, self.centers, self.inertia, self.n_iter, self.init_indices = labels, centers, inertia, n_iter, init_indices


def check_domain(n, d, n_clusters, max_iter=300, tol=1e-4, n_init="auto"):
    """raise KMeansError unless the shape and parameters are inside the supported domain"""
    def need(ok, msg):
        if not ok:
            raise KMeansError(msg)
    for name, v in (("n", n), ("d", d), ("n_clusters", n_clusters), ("max_iter", max_iter)):
        need(is_int(v), "%s must be an integer, got %r" % (name, v))
    need(1 <= n <= MAX_N, "need 1 <= n <= %d points, got %d" % (MAX_N, n))
    need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    need(1 <= n_clusters <= min(MAX_K, n), "need 1 <= n_clusters <= min(%d, n = %d), got %d" % (MAX_K, n, n_clusters))
    need(max_iter >= 1, "need max_iter >= 1, got %d" % max_iter)
    need(isinstance(tol, (numbers.Real, np.number)) and not isinstance(tol, bool) and math.isfinite(tol) and tol >= 0,
         "need a finite tol >= 0, got %r" % (tol,))
    need(n_init == "auto" or (is_int(n_init) and n_init >= 1), "n_init is 'auto' or an integer >= 1, got %r" % (n_init,))


def check_random_state(seed):
    """sklearn.utils.check_random_state"""
    return _common.check_random_state(seed, KMeansError)


def n_local_trials(k):
    """sklearn's k-means++ candidates per centre"""
    return 2 + int(np.log(k))


def tolerance(X, tol):
    """sklearn's _tolerance: mean(var(X, axis=0)) * tol, in float64"""
    if tol == 0:
        return 0.0
    return float(np.mean(np.var(np.asarray(X, np.float64), axis=0)) * tol)


def is_same_clustering(labels1, labels2, k):
    """sklearn's _is_same_clustering: equal up to a permutation of the labels"""
    mapping = np.full(k, -1, np.int64)
    for a, b in zip(np.asarray(labels1).tolist(), np.asarray(labels2).tolist()):
        if mapping[a] == -1:
            mapping[a] = b
        elif mapping[a] != b:
            return False
    return True


# ---- CPU checker (float64 numpy)

class _Numpy:
    """the backend operations in float64 numpy"""

    def __init__(self, X):
        self.X = np.asarray(X, np.float64)
        self.n, self.d = self.X.shape
        self.reset_labels()

    def reset_labels(self):
        self.labels = np.full(self.n, -1, np.int64)

    def gather(self, idx):
        return self.X[np.asarray(idx, np.int64)].copy()

    def centers_from(self, C):
        return np.array(C, np.float64)

    def to_numpy(self, C):
        return np.array(C, np.float64)

    def _dist(self, x):
        return np.sum((self.X - x) ** 2, axis=1)

    def seed(self, cand, first):
        D = np.stack([self._dist(self.X[c]) for c in cand])
        if not first:
            D = np.minimum(self.closest[None, :], D)
        pots = D.sum(axis=1)
        best = int(np.argmin(pots))
        self.closest = D[best]
        return int(cand[best]), float(pots[best])

    def search(self, vals):
        idx = np.searchsorted(np.cumsum(self.closest, dtype=np.float64), vals)
        return np.minimum(idx, self.n - 1)

    def assign(self, C):
        k = C.shape[0]
        lab = np.empty(self.n, np.int64)
        dist = np.empty(self.n)
        ch = max(1, (1 << 22) // max(1, k * self.d))
        for s in range(0, self.n, ch):
            D = np.sum((self.X[s:s + ch, None, :] - C[None, :, :]) ** 2, axis=2)
            lab[s:s + ch] = np.argmin(D, axis=1)
            dist[s:s + ch] = D[np.arange(D.shape[0]), lab[s:s + ch]]
        return lab, dist

    def lloyd(self, C):
        k = C.shape[0]
        lab, dist = self.assign(C)
        changed = int(np.count_nonzero(lab != self.labels))
        self.labels = lab
        sums = np.zeros((k, self.d))
        np.add.at(sums, lab, self.X)
        wt = np.bincount(lab, minlength=k).astype(np.float64)
        empty = np.nonzero(wt == 0)[0]
        if len(empty) and dist.max() != 0:
            far = np.lexsort((np.arange(self.n), -dist))[:len(empty)]
            for nw, f in zip(empty, far):
                old = lab[f]
                sums[old] -= self.X[f]
                sums[nw] = self.X[f]
                wt[nw] = 1.0
                wt[old] -= 1.0
        Cn = sums.copy()
        heavy = int(np.argmax(wt))
        for j in range(k):          # sklearn's _average_centers, in its order
            if wt[j] > 0:
                Cn[j] *= 1.0 / wt[j]
            else:
                Cn[j] = Cn[heavy]
        return Cn, float(np.sum((Cn - C) ** 2)), changed

    def finish(self, C, assign):
        if assign:
            self.labels, dist = self.assign(C)
        else:
            dist = np.sum((self.X - C[self.labels]) ** 2, axis=1)
        return float(np.sum(dist))

    def labels_numpy(self):
        return self.labels.astype(np.int32)


# ---- device

class _Device:
    """thin launcher of the ra_kmeans_* entries on the current stream of X's device"""

    def __init__(self, X):
        L = Launcher(X)
        torch = L.torch
        self.torch, self.api, self.lib, self.dev, self.stream, self.call = torch, L.api, L.lib, L.dev, L.stream, L.call
        self.X = X
        self.n, self.d = (int(s) for s in X.shape)
        self.nrm = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        self.call("ra_kmeans_sqnorm", ptr(X), self.n, self.d, ptr(self.nrm))
        self.labels = torch.empty(self.n, dtype=torch.int32, device=self.dev)
        self.stats = torch.empty(3, dtype=torch.float64, device=self.dev)
        self.closest = None
        self.reset_labels()

    def reset_labels(self):
        self.labels.fill_(-1)

    def gather(self, idx):
        i = self.torch.as_tensor(np.asarray(idx, np.int64), device=self.dev)
        return self.X.index_select(0, i).to(self.torch.float64).contiguous()

    def centers_from(self, C):
        return self.torch.from_numpy(np.ascontiguousarray(C, np.float64)).to(self.dev)

    def to_numpy(self, C):
        return C.cpu().numpy()

    def seed(self, cand, first):
        torch = self.torch
        if not isinstance(cand, torch.Tensor):
            cand = torch.as_tensor(np.asarray(cand, np.int32), device=self.dev)
        m = int(cand.numel())
        if self.closest is None:
            self.closest = torch.empty(self.n, dtype=torch.float64, device=self.dev)
        out = torch.empty(m + 2, dtype=torch.float64, device=self.dev)
        self.call("ra_kmeans_seed", ptr(self.X), self.n, self.d, ptr(cand), m, ptr(self.closest), int(bool(first)), ptr(out))
        o = out[:2].cpu().numpy()
        return int(o[0]), float(o[1])

    def search(self, vals):
        torch = self.torch
        v = torch.from_numpy(np.ascontiguousarray(vals, np.float64)).to(self.dev)
        idx = torch.empty(int(v.numel()), dtype=torch.int32, device=self.dev)
        self.call("ra_kmeans_search", ptr(self.closest), self.n, ptr(v), int(v.numel()), ptr(idx))
        return idx

    def lloyd(self, C):
        k = int(C.shape[0])
        Cn = self.torch.empty_like(C)
        self.call("ra_kmeans_lloyd", ptr(self.X), self.n, self.d, ptr(self.nrm), ptr(C), k, ptr(Cn), ptr(self.labels), ptr(self.stats))
        s = self.stats.cpu().numpy()
        return Cn, float(s[0]), int(s[1])

    def finish(self, C, assign):
        out = self.torch.empty(1, dtype=self.torch.float64, device=self.dev)
        self.call("ra_kmeans_labels", ptr(self.X), self.n, self.d, ptr(self.nrm), ptr(C), int(C.shape[0]), ptr(self.labels),
                  int(bool(assign)), ptr(out))
        return float(out.item())

    def labels_numpy(self):
        return self.labels.cpu().numpy().astype(np.int32)

    def tolerance(self, tol):
        """mean(var(X, axis=0)) * tol in float64, two passes over row chunks (torch plumbing, once per fit)"""
        if tol == 0:
            return 0.0
        torch = self.torch
        ch = max(1, (1 << 24) // self.d)
        s = torch.zeros(self.d, dtype=torch.float64, device=self.dev)
        for i in range(0, self.n, ch):
            s += self.X[i:i + ch].to(torch.float64).sum(0)
        mean = s / self.n
        q = torch.zeros(self.d, dtype=torch.float64, device=self.dev)
        for i in range(0, self.n, ch):
            q += ((self.X[i:i + ch].to(torch.float64) - mean) ** 2).sum(0)
        return float((q / self.n).mean().item()) * tol


# ---- the loop (sklearn KMeans.fit / _kmeans_single_lloyd / _kmeans_plusplus)

def _plusplus(B, k, rs):
    n = B.n
    m = n_local_trials(k)
    c0 = int(rs.choice(n, p=np.ones(n) / n))
    idx = [c0]
    _, pot = B.seed([c0], True)
    for _ in range(1, k):
        vals = rs.uniform(size=m) * pot
        chosen, pot = B.seed(B.search(vals), False)
        idx.append(chosen)
    return np.asarray(idx, np.int64)


def _single(B, C, max_iter, tol_abs):
    B.reset_labels()
    strict = False
    i = 0
    for i in range(max_iter):
        C, shift, changed = B.lloyd(C)
        if changed == 0:
            strict = True
            break
        if shift <= tol_abs:
            break
    inertia = B.finish(C, not strict)
    return B.labels_numpy(), inertia, C, i + 1


def _fit(B, k, init, n_init, max_iter, tol_abs, random_state):
    rs = check_random_state(random_state)
    best = None
    for _ in range(n_init):
        if isinstance(init, str) and init == "k-means++":
            idx = _plusplus(B, k, rs)
            C = B.gather(idx)
        elif isinstance(init, str) and init == "random":
            idx = np.asarray(rs.choice(B.n, size=k, replace=False, p=np.ones(B.n) / B.n), np.int64)
            C = B.gather(idx)
        else:
            idx = None
            C = B.centers_from(init)
        labels, inertia, C, n_iter = _single(B, C, max_iter, tol_abs)
        if best is None or (inertia < best[1] and not is_same_clustering(labels, best[0], k)):
            best = (labels, inertia, C, n_iter, idx)
    labels, inertia, C, n_iter, idx = best
    distinct = len(np.unique(labels))
    if distinct < k:
        warnings.warn("Number of distinct clusters ({}) found smaller than n_clusters ({}). Possibly due to duplicate points "
                      "in X.".format(distinct, k), ConvergenceWarning, stacklevel=3)
    return KMeansResult(labels, B.to_numpy(C), float(inertia), int(n_iter), idx)


def _resolve_init(init, k, d):
    if isinstance(init, str):
        if init not in ("k-means++", "random"):
            raise KMeansError("init is 'k-means++', 'random' or a [k][d] array, got %r" % (init,))
        return init
    C = np.array(init.detach().cpu().numpy() if hasattr(init, "detach") else init, np.float64)
    if C.shape != (k, d):
        raise KMeansError("an init array is [n_clusters][d] = [%d][%d], got %s" % (k, d, C.shape))
    if not np.all(np.isfinite(C)):
        raise KMeansError("the init array holds NaN or infinite values")
    return C


def kmeans(X, n_clusters, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None, backend="device"):
    """k-means of X [n][d]: KMeansResult(labels int32 [n], centers float64 [k][d], inertia, n_iter, init_indices)"""
    X = _common.as_input(X, backend, KMeansError)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, n_clusters, max_iter, tol, n_init)
    init = _resolve_init(init, n_clusters, d)
    check_random_state(random_state)
    _common.check_finite(X, backend, KMeansError)
    if n_init == "auto":
        n_init = 10 if isinstance(init, str) and init == "random" else 1
    if not isinstance(init, str) and n_init != 1:
        warnings.warn("Explicit initial center position passed: performing only one init in KMeans instead of n_init=%d." % n_init,
                      RuntimeWarning, stacklevel=2)
        n_init = 1
    if backend == "numpy":
        return _fit(_Numpy(X), n_clusters, init, n_init, max_iter, tolerance(X, tol), random_state)
    import torch
    with torch.cuda.device(X.device):
        B = _Device(X)
        return _fit(B, n_clusters, init, n_init, max_iter, B.tolerance(tol), random_state)


def labels_for(X, centers, backend="device"):
    """(labels int32 [n], inertia) of the given centers [k][d]: the E-step alone"""
    X = _common.as_input(X, backend, KMeansError)
    n, d = (int(s) for s in X.shape)
    C = np.asarray(centers, np.float64)
    check_domain(n, d, int(C.shape[0]) if C.ndim == 2 else 0)
    C = _resolve_init(C, C.shape[0], d)
    _common.check_finite(X, backend, KMeansError)
    if backend == "numpy":
        B = _Numpy(X)
        inertia = B.finish(C, True)
        return B.labels_numpy(), inertia
    import torch
    with torch.cuda.device(X.device):
        B = _Device(X)
        inertia = B.finish(B.centers_from(C), True)
        return B.labels_numpy(), inertia


# ---- scores (utils_ralib.purity_score / c_purity_score over sklearn.metrics.cluster.contingency_matrix)

def contingency_matrix(y_true, y_pred):
    """[classes of y_true][classes of y_pred] counts, both in sorted order of their distinct values"""
    y_true, y_pred = np.asarray(y_true).ravel(), np.asarray(y_pred).ravel()
    if y_true.shape != y_pred.shape:
        raise KMeansError("y_true and y_pred differ in length: %d, %d" % (y_true.size, y_pred.size))
    classes, ci = np.unique(y_true, return_inverse=True)
    clusters, ki = np.unique(y_pred, return_inverse=True)
    M = np.zeros((classes.size, clusters.size), np.int64)
    np.add.at(M, (ci, ki), 1)
    return M


def purity_score(y_true, y_pred):
    """sum over clusters of the largest class count / n"""
    M = contingency_matrix(y_true, y_pred)
    return float(np.sum(np.amax(M, axis=0)) / np.sum(M))


def c_purity_score(y_true, y_pred):
    """sum over classes of the largest cluster count / n"""
    M = contingency_matrix(y_true, y_pred)
    return float(np.sum(np.amax(M, axis=1)) / np.sum(M))


# ---- cluster validity without ground truth (sklearn.metrics silhouette_*, calinski_harabasz_score, davies_bouldin_score)

SIL_MAX_N = 262144      # rows of one silhouette evaluation (n^2 pair distances); larger n needs sample_size


class ValidityResult:
    """silhouette (mean of the evaluated samples), class_silhouette float64 [k] (mean per cluster, nan for an id without evaluated
    members), calinski_harabasz, davies_bouldin, counts int64 [k] (of all n points), samples float64 [n] (s_i; nan for rows outside
    the sample) and sample_indices (None without sample_size)"""

    def __init__(self, silhouette, class_silhouette, calinski_harabasz, davies_bouldin, counts, samples, sample_indices):
        self.silhouette, self.class_silhouette, self.calinski_harabasz = silhouette, class_silhouette, calinski_harabasz
        self.davies_bouldin, self.counts, self.samples, self.sample_indices = davies_bouldin, counts, samples, sample_indices


class SweepRow:
    """one k of a sweep: k, inertia, n_iter, silhouette, calinski_harabasz, davies_bouldin, labels int32 [n], centers float64 [k][d]"""

    def __init__(self, k, fit, val):
        self.k, self.inertia, self.n_iter, self.labels, self.centers = int(k), fit.inertia, fit.n_iter, fit.labels, fit.centers
        self.fit, self.validity = fit, val
        self.silhouette, self.calinski_harabasz, self.davies_bouldin = val.silhouette, val.calinski_harabasz, val.davies_bouldin
        self.class_silhouette, self.counts = val.class_silhouette, val.counts


class SweepResult:
    """rows (one SweepRow per k, in the order of ks) and best_k: the k of the largest silhouette, the smaller k on ties"""

    def __init__(self, rows):
        self.rows = rows
        best = rows[0]
        for r in rows[1:]:
            if r.silhouette > best.silhouette or (r.silhouette == best.silhouette and r.k < best.k):
                best = r
        self.best_k = best.k

    def row(self, k):
        return next(r for r in self.rows if r.k == k)

    def table(self):
        """float64 [len(ks)][5]: k, inertia, silhouette, calinski_harabasz, davies_bouldin"""
        return np.array([[r.k, r.inertia, r.silhouette, r.calinski_harabasz, r.davies_bouldin] for r in self.rows], np.float64).reshape(-1, 5)


def check_number_of_labels(m, n):
    """sklearn's check: 2 <= m <= n - 1 clusters with members"""
    if not 1 < m < n:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % m)


def _as_labels(labels, n, k):
    """(int64 [n] labels on the host, k): values in 0 .. k - 1, k = max + 1 when not given"""
    lab = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
    if lab.shape != (n,) or not np.issubdtype(lab.dtype, np.integer):
        raise KMeansError("labels are [%d] integers, got %s %s" % (n, lab.dtype, lab.shape))
    lab = lab.astype(np.int64)
    if k is None:
        k = int(lab.max()) + 1
    if not (is_int(k) and 1 <= k <= MAX_K):
        raise KMeansError("need 1 <= k <= %d, got %r" % (MAX_K, k))
    if lab.min() < 0 or lab.max() >= k:
        raise KMeansError("labels are integers in 0 .. k - 1 = %d, got %d .. %d" % (k - 1, lab.min(), lab.max()))
    return lab, int(k)


def _validity_input(X, labels, k, backend):
    X = _common.as_input(X, backend, KMeansError)
    n, d = (int(s) for s in X.shape)
    if not (1 <= n <= MAX_N and 1 <= d <= MAX_D):
        raise KMeansError("need 1 <= n <= %d points of 1 <= d <= %d features, got %d x %d" % (MAX_N, MAX_D, n, d))
    lab, k = _as_labels(labels, n, k)
    return X, lab, k, n, d


def _sample(n, sample_size, random_state):
    """sklearn's silhouette_score subsample: check_random_state(rs).permutation(n)[:sample_size]; None without sample_size"""
    if sample_size is None:
        return None
    if not (is_int(sample_size) and 1 <= sample_size):
        raise KMeansError("sample_size is None or an integer >= 1, got %r" % (sample_size,))
    return check_random_state(random_state).permutation(n)[:sample_size]


def _check_silhouette_domain(n, d, k, lab):
    if not (3 <= n <= SIL_MAX_N):
        raise KMeansError("the silhouette takes 3 <= n <= %d points (pass sample_size <= %d for more), got %d" % (SIL_MAX_N, SIL_MAX_N, n))
    if not (2 <= k <= MAX_K):
        raise KMeansError("the silhouette takes 2 <= k <= %d, got %d" % (MAX_K, k))
    check_number_of_labels(int(np.count_nonzero(np.bincount(lab, minlength=k))), n)


def _silhouette_numpy(X, lab, k):
    """(s, a, b, nearest) in float64 from differences: the CPU checker"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    cnt = np.bincount(lab, minlength=k)
    H = np.zeros((n, k))
    H[np.arange(n), lab] = 1.0
    D = np.empty((n, k))
    ch = max(1, (1 << 22) // max(1, n * d))
    for s0 in range(0, n, ch):
        df = X[s0:s0 + ch, None, :] - X[None, :, :]
        D[s0:s0 + ch] = np.sqrt(np.sum(df * df, axis=2)) @ H
    rows = np.arange(n)
    no = cnt[lab]
    a = np.where(no > 1, D[rows, lab] / np.maximum(no - 1, 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        M = np.where(cnt[None, :] > 0, D / cnt[None, :], np.inf)
    M[rows, lab] = np.inf
    nearest = np.argmin(M, axis=1)
    b = M[rows, nearest]
    mx = np.maximum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        sv = np.where((no > 1) & (mx > 0), (b - a) / mx, 0.0)
    return sv, a, b, nearest.astype(np.int32)


def _device_labels(X, lab):
    import torch
    return torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(X.device)


def _silhouette_device(X, lab, k):
    L = Launcher(X)
    torch = L.torch
    n, d = (int(s) for s in X.shape)
    with torch.cuda.device(X.device):
        labels = _device_labels(X, lab)
        out = torch.empty((n, 3), dtype=torch.float64, device=X.device)
        near = torch.empty(n, dtype=torch.int32, device=X.device)
        L.call("ra_kmeans_silhouette", ptr(X), n, d, ptr(labels), k, ptr(out), ptr(near))
        o = out.cpu().numpy()
        return o[:, 0].copy(), o[:, 1].copy(), o[:, 2].copy(), near.cpu().numpy()


def _take(X, idx, backend):
    if backend == "device":
        import torch
        return X.index_select(0, torch.as_tensor(np.asarray(idx, np.int64), device=X.device)).contiguous()
    return X[idx]


def _silhouette(X, lab, k, backend):
    n, d = (int(s) for s in X.shape)
    _check_silhouette_domain(n, d, k, lab)
    _common.check_finite(X, backend, KMeansError)
    return _silhouette_device(X, lab, k) if backend == "device" else _silhouette_numpy(X, lab, k)


def silhouette_samples(X, labels, k=None, backend="device", details=False):
    """sklearn's silhouette_samples(metric="euclidean"): float64 [n]; details=True: (s, a, b, nearest) with a the mean distance to
    the own cluster's other members (0 for a singleton), b the least mean distance to another cluster and nearest its id"""
    X, lab, k, n, d = _validity_input(X, labels, k, backend)
    sv, a, b, near = _silhouette(X, lab, k, backend)
    return (sv, a, b, near) if details else sv


def _sampled_silhouette(X, lab, k, sample_size, random_state, backend):
    """(s of the evaluated rows, their indices or None)"""
    idx = _sample(int(X.shape[0]), sample_size, random_state)
    if idx is None:
        return _silhouette(X, lab, k, backend)[0], None
    return _silhouette(_take(X, idx, backend), lab[idx], k, backend)[0], idx


def silhouette_score(X, labels, k=None, sample_size=None, random_state=None, backend="device"):
    """sklearn's silhouette_score(metric="euclidean"): the mean of silhouette_samples, over sklearn's subsample when sample_size is
    given (the cluster-count check then runs on the sample)"""
    X, lab, k, n, d = _validity_input(X, labels, k, backend)
    return float(np.mean(_sampled_silhouette(X, lab, k, sample_size, random_state, backend)[0]))


def _dispersion(X, lab, k, backend):
    """(centroids [k][d], counts [k], sum |x - mu_c|^2 [k], sum |x - mu_c| [k]) from the labels, float64"""
    n, d = (int(s) for s in X.shape)
    check_number_of_labels(int(np.count_nonzero(np.bincount(lab, minlength=k))), n)
    _common.check_finite(X, backend, KMeansError)
    if backend == "numpy":
        Xd = np.asarray(X, np.float64)
        cnt = np.bincount(lab, minlength=k)
        sums = np.zeros((k, d))
        np.add.at(sums, lab, Xd)
        cen = sums / np.maximum(cnt, 1)[:, None]
        dist = np.sum((Xd - cen[lab]) ** 2, axis=1)
        return cen, cnt, np.bincount(lab, weights=dist, minlength=k), np.bincount(lab, weights=np.sqrt(dist), minlength=k)
    L = Launcher(X)
    torch = L.torch
    with torch.cuda.device(X.device):
        labels = _device_labels(X, lab)
        cen = torch.empty((k, d), dtype=torch.float64, device=X.device)
        cnt = torch.empty(k, dtype=torch.int32, device=X.device)
        sq = torch.empty(k, dtype=torch.float64, device=X.device)
        ab = torch.empty(k, dtype=torch.float64, device=X.device)
        L.call("ra_kmeans_dispersion", ptr(X), n, d, ptr(labels), k, ptr(cen), ptr(cnt), ptr(sq), ptr(ab))
        return cen.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), sq.cpu().numpy(), ab.cpu().numpy()


def _ch_db(cen, cnt, sq, ab, n):
    """(Calinski-Harabasz, Davies-Bouldin) in float64 from the dispersion pass, as sklearn forms them"""
    nz = cnt > 0
    m = int(np.count_nonzero(nz))
    cen, cnt, sq, ab = cen[nz], cnt[nz].astype(np.float64), sq[nz], ab[nz]
    mu = np.sum(cen * cnt[:, None], axis=0) / n
    extra, intra = float(np.sum(cnt * np.sum((cen - mu) ** 2, axis=1))), float(np.sum(sq))
    ch = 1.0 if intra == 0.0 else extra * (n - m) / (intra * (m - 1.0))
    S = ab / cnt
    df = cen[:, None, :] - cen[None, :, :]
    cd = np.sqrt(np.sum(df * df, axis=2))
    if np.allclose(S, 0) or np.allclose(cd, 0):
        return ch, 0.0
    cd[cd == 0] = np.inf
    return ch, float(np.mean(np.max((S[:, None] + S[None, :]) / cd, axis=1)))


def calinski_harabasz_score(X, labels, k=None, backend="device"):
    """sklearn's calinski_harabasz_score: between- over within-cluster dispersion of the label-derived centroids"""
    X, lab, k, n, d = _validity_input(X, labels, k, backend)
    return _ch_db(*_dispersion(X, lab, k, backend), n)[0]


def davies_bouldin_score(X, labels, k=None, backend="device"):
    """sklearn's davies_bouldin_score: mean over the clusters of the worst (S_c + S_c') / |mu_c - mu_c'|"""
    X, lab, k, n, d = _validity_input(X, labels, k, backend)
    return _ch_db(*_dispersion(X, lab, k, backend), n)[1]


def validity(X, labels, k=None, sample_size=None, random_state=None, backend="device"):
    """ValidityResult of the labels: the silhouette (over sklearn's subsample when sample_size is given), its mean per cluster,
    the Calinski-Harabasz and Davies-Bouldin indices (always of all n points) and the cluster sizes"""
    X, lab, k, n, d = _validity_input(X, labels, k, backend)
    sv, idx = _sampled_silhouette(X, lab, k, sample_size, random_state, backend)
    ch, db = _ch_db(*_dispersion(X, lab, k, backend), n)
    sl = lab if idx is None else lab[idx]
    ne = np.bincount(sl, minlength=k)
    with np.errstate(divide="ignore", invalid="ignore"):
        cls = np.bincount(sl, weights=sv, minlength=k) / ne
    cls[ne == 0] = np.nan
    samples = sv
    if idx is not None:
        samples = np.full(n, np.nan)
        samples[idx] = sv
    return ValidityResult(float(np.mean(sv)), cls, ch, db, np.bincount(lab, minlength=k), samples, idx)


def parse_sweep(text):
    """the ks of 'K1,K2,...' or 'LO:HI[:STEP]' (HI included): strictly increasing integers >= 2"""
    try:
        if ":" in text:
            p = [int(v) for v in text.split(":")]
            if len(p) not in (2, 3):
                raise ValueError(text)
            step = p[2] if len(p) == 3 else 1
            ks = list(range(p[0], p[1] + 1, step)) if step >= 1 else []
        else:
            ks = [int(v) for v in text.split(",")]
    except ValueError:
        raise KMeansError("a sweep is K1,K2,... or LO:HI[:STEP], got %r" % (text,))
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 2:
        raise KMeansError("a sweep needs increasing k >= 2, got %r" % (text,))
    return ks


def sweep(X, ks, sample_size=None, random_state=None, backend="device", **kmeans_kwargs):
    """kmeans(X, k, random_state=random_state, **kmeans_kwargs) and validity() for every k of ks on one device copy of X:
    SweepResult(rows, best_k)"""
    ks = [int(v) for v in ks]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 2:
        raise KMeansError("a sweep needs increasing k >= 2, got %r" % (ks,))
    X = _common.as_input(X, backend, KMeansError)
    n, d = (int(s) for s in X.shape)
    for k in ks:
        check_domain(n, d, k)
    if n > SIL_MAX_N and not (is_int(sample_size) and sample_size <= SIL_MAX_N):
        raise KMeansError("more than %d points need sample_size <= %d for the silhouette" % (SIL_MAX_N, SIL_MAX_N))
    rows = []
    for k in ks:
        fit = kmeans(X, k, random_state=random_state, backend=backend, **kmeans_kwargs)
        rows.append(SweepRow(k, fit, validity(X, fit.labels, k, sample_size, random_state, backend)))
    return SweepResult(rows)


# ---- class averages through the engine

def class_averages(images, params, labels, k, ou, min_count=1, preprocess=True, device=0):
    """[k][nx][nx] float32 averages of the stack's clusters, as the multi-reference loop updates its references: the particles
    preprocessed (masked mean subtracted) unless preprocess=False, rot_shift2D by params [n][4] (alpha, sx, sy, mirror) with the
    cluster as ref_id (Engine.transform_accumulate), then (even + odd) / count normalised under model_circle(ou)
    (Engine.update_references).  Clusters with fewer than min_count members stay zero."""
    import torch
    from . import api
    dev = torch.device("cuda", device)
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images, np.float32))
    x = images.to(dev, dtype=torch.float32).contiguous().clone()
    if x.ndim != 3 or x.shape[1] != x.shape[2]:
        raise KMeansError("images are [n][nx][nx], got %s" % (tuple(x.shape),))
    n, nx = int(x.shape[0]), int(x.shape[-1])
    prm = np.asarray(params.detach().cpu().numpy() if hasattr(params, "detach") else params, np.float64)
    lab = np.asarray(labels.detach().cpu().numpy() if hasattr(labels, "detach") else labels).astype(np.int64)
    if prm.shape != (n, 4):
        raise KMeansError("params is [%d][4] (alpha, sx, sy, mirror), got %s" % (n, prm.shape))
    if lab.shape != (n,) or not (is_int(k) and 1 <= k <= MAX_K) or lab.min() < 0 or lab.max() >= k:
        raise KMeansError("labels are [%d] integers in 0 .. k - 1 with 1 <= k <= %d" % (n, MAX_K))
    rec = np.zeros(n, api.RESULT_DTYPE)
    rec["alpha"], rec["sx"], rec["sy"] = prm[:, 0], prm[:, 1], prm[:, 2]
    rec["mirror"] = (prm[:, 3] != 0).astype(np.int32)
    rec["ref_id"] = lab.astype(np.int32)
    with torch.cuda.device(dev):
        eng = api.Engine(nx, int(ou), 0.0, 0.0, 1.0, int(k), api.RA_MODE_MREF, device=dev.index)
        try:
            eng.use_current_stream()
            if preprocess:
                eng.normalize_particles(x)
            res = torch.from_numpy(rec.view(np.int32).reshape(n, 8).copy()).to(dev)
            sums = torch.zeros((k, 2, nx, nx), dtype=torch.float32, device=dev)
            counts = torch.zeros(k, dtype=torch.int32, device=dev)
            eng.transform_accumulate(x, res, 0, None, sums, counts)
            refs = torch.zeros((k, nx, nx), dtype=torch.float32, device=dev)
            eng.update_references(sums, counts, refs, int(min_count))
            eng.sync()
            return refs.cpu().numpy()
        finally:
            eng.close()


# ---- command line

def read_input(path, key="factors"):
    """[n][d] float32 from an .npz (key) or an .npy"""
    return _common.read_input(path, key, KMeansError)


def read_truth(path, n):
    """[n] int classes from an int .npy or a params.txt (idx angle_psi shift_x shift_y mirror class, rows in any order)"""
    return _common.read_truth(path, n, KMeansError)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.kmeans")
    _common.add_cluster_arguments(ap, ("input", "output"), "factors", False)
    ap.add_argument("--k", type=int, default=None, help="number of clusters (optional with --sweep)")
    ap.add_argument("--scores", action="store_true", help="silhouette (overall, per class, per sample), Calinski-Harabasz and "
                    "Davies-Bouldin of the result in OUT.npz, and one line per class")
    ap.add_argument("--sweep", default=None, help="K1,K2,... or LO:HI[:STEP]: k-means and the three scores for every k; the "
                    "result written is that of --k if given, else of the largest silhouette")
    ap.add_argument("--sample_size", type=int, default=None, help="evaluate the silhouette on sklearn's random subsample of this size")
    _common.add_cluster_arguments(ap, ("--key",), "factors", False)
    ap.add_argument("--init", default="k-means++", help="k-means++, random or a [k][d] .npy")
    ap.add_argument("--n_init", default="auto", help="'auto' or an integer")
    ap.add_argument("--max_iter", type=int, default=300)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=None, help="random_state")
    _common.add_cluster_arguments(ap, ("--backend", "--truth", "--stack", "--params", "--ou", "--averages", "--device"), "factors", False)
    args = ap.parse_args(argv)
    ks = None
    if args.sample_size is not None and not (args.scores or args.sweep is not None):
        ap.error("--sample_size needs --scores or --sweep")
    if args.k is None and args.sweep is None:
        ap.error("one of --k and --sweep is needed")
    if args.sweep is not None:
        try:
            ks = parse_sweep(args.sweep)
        except KMeansError as e:
            ap.error(str(e))
    try:
        X = read_input(args.input, args.key)
        n, d = X.shape
        n_init = args.n_init if args.n_init == "auto" else int(args.n_init)
        init = args.init if args.init in ("k-means++", "random") else np.load(args.init)
        for kk in (ks or []) + ([args.k] if args.k is not None else []):
            check_domain(n, d, kk, args.max_iter, args.tol, n_init)
        if args.sample_size is not None and args.sample_size < 1:
            raise KMeansError("--sample_size is an integer >= 1")
        if (args.scores or ks) and n > SIL_MAX_N and not (args.sample_size and args.sample_size <= SIL_MAX_N):
            raise KMeansError("more than %d points need --sample_size <= %d for the silhouette" % (SIL_MAX_N, SIL_MAX_N))
        truth = read_truth(args.truth, n) if args.truth else None
    except (KMeansError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    _common.check_averages_arguments(ap, args, usage=False)
    if args.backend == "device" or args.averages:
        _common.require_gpu(_common.NO_GPU)
    swept = val = None
    try:
        Xb = _common.to_device(X, args.device) if args.backend == "device" else X
        if ks:
            swept = sweep(Xb, ks, args.sample_size, args.seed, args.backend, init=init, n_init=n_init, max_iter=args.max_iter, tol=args.tol)
            if args.k is None:
                args.k = swept.best_k
        if swept is not None and args.k in ks:
            res, val = swept.row(args.k).fit, swept.row(args.k).validity
        else:
            res = kmeans(Xb, args.k, init, n_init, args.max_iter, args.tol, args.seed, backend=args.backend)
        if args.scores and val is None:
            val = validity(Xb, res.labels, args.k, args.sample_size, args.seed, args.backend)
    except (KMeansError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    out = dict(labels=res.labels, centers=res.centers, inertia=np.float64(res.inertia), n_iter=np.int64(res.n_iter),
               init_indices=res.init_indices if res.init_indices is not None else np.zeros(0, np.int64), k=np.int64(args.k),
               init=np.str_(args.init), seed=np.int64(-1 if args.seed is None else args.seed), backend=np.str_(args.backend))
    msg = "%s: %d points x %d, k = %d, %d iterations, inertia %.6g" % (args.output, n, d, args.k, res.n_iter, res.inertia)
    if truth is not None:
        msg += _common.truth_scores(out, truth, res.labels)
    if args.averages:
        msg += _common.write_averages(args, n, res.labels, args.k, None, KMeansError)
    if swept is not None:
        out["sweep"], out["best_k"] = swept.table(), np.int64(swept.best_k)
        print("%5s %14s %11s %14s %11s" % ("k", "inertia", "silhouette", "CH", "DB"))
        for r in swept.rows:
            print("%5d %14.6g %11.6f %14.6g %11.6f%s" % (r.k, r.inertia, r.silhouette, r.calinski_harabasz, r.davies_bouldin,
                                                          "  <- best" if r.k == swept.best_k else ""))
    if args.scores:
        out["silhouette"], out["class_silhouette"], out["silhouette_samples"] = np.float64(val.silhouette), val.class_silhouette, val.samples
        out["calinski_harabasz"], out["davies_bouldin"] = np.float64(val.calinski_harabasz), np.float64(val.davies_bouldin)
        for c in range(args.k):
            print("class %3d: %7d members, silhouette %8.4f" % (c, val.counts[c], val.class_silhouette[c]))
        msg += ", silhouette %.4f, CH %.6g, DB %.4f" % (val.silhouette, val.calinski_harabasz, val.davies_bouldin)
    np.savez(args.output, **out)
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
