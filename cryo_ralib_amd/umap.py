"""UMAP embedding of factors X [n][d] on the GPU, with out-of-sample placement (after umap-learn 0.5: McInnes, Healy and Melville
2018; its smooth_knn_dist, fuzzy_simplicial_set, find_ab_params and optimize_layout_euclidean, restated so that the result is a pure
function of the arguments).

    python -m cryo_ralib_amd.umap IN OUT.npz [--key factors] [--n_neighbors 15] [--min_dist 0.1] [--spread 1] [--n_epochs N]
                                  [--learning_rate 1] [--negative_sample_rate 5] [--init spectral|pca|random|FILE.npy] [--seed 42]
                                  [--backend device|numpy] [--quality [K]]
                                  [--place_into FIT_OUT.npz --fit_input FILE [--fit_key factors] [--fit_labels FILE] [--batch B]]

IN is the OUT.npz of the sdr tool (--key factors, the default) or an [n][d] .npy.  OUT.npz holds embedding [n][2] float32, a, b,
n_epochs, init (the start that was used) and the options; with --quality also trustworthiness, continuity, trust_point and cont_point
(as the tsne tool adds them).  The kmeans, gmm, dbscan, hdbscan and ward tools read the file with --key embedding.  --place_into
places the input's rows into the embedding of an earlier run (its a, b, n_neighbors, negative_sample_rate and seed are taken from
that file unless given), whose rows are
--fit_input; --fit_labels (an int .npy or a clustering tool's OUT.npz, one label per fitted row) adds labels and label_confidence by
tsne.vote_labels.

umap-learn's optimiser is Hogwild SGD over the edges with a racing generator; here an epoch is a gather per vertex over the previous
epoch's positions with a counter-based generator, so the same call gives the same bits.

The contract, rule by rule.  Positions are float32; everything else is float64.
  Inputs.  X [n][d] float32.  n_neighbors = 15, min_dist = 0.1, spread = 1.0, n_epochs = None (500 if n <= 10000, else 200),
     learning_rate = 1.0, negative_sample_rate = 5, repulsion_strength gamma = 1.0, init = "spectral", random_state = 42 (an integer
     in 0 .. 2^32 - 1; it feeds rules 6 and 7 only).  Two output dimensions.
  1. Neighbours.  N(i) is the K = n_neighbors - 1 nearest OTHER rows: ra_tsne_knn's rule (D2, j), D2 in double from the differences of
     the float32 values.  d_ij = sqrt(D2).
  2. Smooth-kNN calibration (smooth_knn_dist with local_connectivity = 1, bandwidth = 1).  rho_i is the least non-zero d_ij of the
     row, 0 if all are zero.  target = log2(n_neighbors).  psum(sigma) = sum_j (x_j > 0 ? exp(-x_j / sigma) : 1), x_j = d_ij - rho_i,
     in list order.  The search starts with lo = 0, hi = inf, mid = 1 and runs at most 64 trips; a trip stops the search when
     |psum(mid) - target| < 1e-5; else if psum > target: hi = mid, mid = (lo + hi) / 2; otherwise lo = mid and mid = 2 mid while hi
     is inf, else (lo + hi) / 2.  sigma_i = max(mid, 1e-3 mean_j d_ij), the row's own mean (umap-learn takes the global mean when
     rho_i = 0; a global mean has no fixed summation order).  w_ij = 1 when x_j <= 0 or sigma_i = 0, else exp(-x_j / sigma_i).
     (The device adds psum's terms lane by lane and then across the lanes, ralign_umap.h: psum may differ from list order by the
     roundings of k additions; the mean is added in list order there too.)
  3. Fuzzy union.  s_ij = w_ij + w_ji - w_ij w_ji, a missing direction counting 0: a CSR with the columns of a row ascending, built
     by _graph.py's stable sort.  Both operations commute, so s_ij == s_ji bit for bit.
  4. Curve.  (a, b) = scipy.optimize.curve_fit of 1 / (1 + a x^(2b)) to x = linspace(0, 3 spread, 300), y = 1 for x < min_dist, else
     exp(-(x - min_dist) / spread) (find_ab_params), on the host.  The defaults give a = 1.5769434603, b = 0.8950608779.  a and b may
     be passed instead.
  5. Schedule.  r_e = s_e / max s.  Entry e fires in epoch t = 1 .. n_epochs iff floor(t r_e) > floor((t - 1) r_e): one multiply and
     one floor each, so device and checker decide alike.  An entry with r_e < 1 / n_epochs never fires (umap-learn's pruning).
     alpha_t = learning_rate (1 - (t - 1) / n_epochs).
  6. One epoch, per vertex i, from the float32 positions of the previous epoch converted to double.  For a firing entry at CSR position
     p with column j: attraction, delta = y_i - y_j, q = delta . delta = dx dx + dy dy, qb = q^b, c = ((-2 a b) qb / q) / (1 + a qb)
     when q > 0, else no move; the move is 2 clip(c delta, -4, 4) per coordinate (the 2 stands in for umap-learn's move_other: entry
     (j, i) fires in the same epochs and pushes i by the same term).  Then repulsion for s = 0 .. negative_sample_rate - 1:
     k = ((z >> 32) n) >> 32, z = splitmix64(seed 0xD1342543DE82EF95 + t 0xA0761D6478BD642F + 16 p + s) mod 2^64 (the finaliser: add
     0x9E3779B97F4A7C15; xor-shift 30, times 0xBF58476D1CE4E5B9; xor-shift 27, times 0x94D049BB133111EB; xor-shift 31); k == i
     contributes nothing; otherwise delta = y_i - y_k, the move is +4 per coordinate when q = 0, else
     clip((2 gamma b) / ((0.001 + q) (1 + a qb)) delta, -4, 4).  Summation order: 16 lanes share a row; lane l walks the entries
     p0 + l, p0 + l + 16, ... and adds an entry's attraction and then its negatives, in that order, to its own sum; the 16 sums
     combine in the xor tree 8, 4, 2, 1 (v_l += v_{l xor m}).  y_i <- float32(y_i + alpha_t sum), rounded once.  No vertex reads a
     position written in the same epoch (two buffers).
  7. Start.  "spectral": spectral.embedding_from_graph on the fuzzy graph (2 components, its defaults); a disconnected graph gives one
     UmapWarning naming the number of components and the "pca" start (so does a graph the solver refuses).  "pca": the first two
     principal axes of X from a float64 eigh on the host.  "random": RandomState(random_state).uniform(-10, 10).  An [n][2] array is
     taken as given.  "spectral" and "pca" are rescaled per coordinate to [0, 10] in double (a coordinate of zero range maps to 5)
     and rounded to float32.  umap-learn's 1e-4 noise is left out.
  8. transform(X_new [n_new][d], X_fit [m][d], Y_fit [m][2]).  The k = min(m, n_neighbors) nearest fitted rows by ra_tsne_knn_query's
     rule, none excluded (k <= 301).  Rule 2 on them with target log2(n_neighbors).  Start: sum_j w_ij Y_j / sum_j w_ij in list
     order.  r = w / max w over the ROW.  Rule 6 with attraction factor 1, lanes over the list slots, the negatives drawn from the m
     fitted rows (none skipped) with p = (row0 + i) k + slot, row0 the global index of the batch's first row; Y_fit is fixed;
     n_epochs = 100.  A point's result is a function of that point, X_fit, Y_fit and the parameters: the same bits whatever the
     batch or the stream.
  9. Domain.  4 <= n <= 262144, 1 <= d <= 2048, 2 <= n_neighbors <= min(302, n), 0 <= min_dist <= spread, 1 <= n_epochs <= 10000,
     0 <= negative_sample_rate <= 16, learning_rate > 0, gamma >= 0, finite X, init="pca" needs d >= 2; transform: m >= 2,
     0 <= n_new <= 2^48 (0 returns empty without a launch; the samples' key index is formed in 64 bits), 1 <= batch <= 262144.  Anything else raises UmapError (a ValueError) before a
     launch.  The kNN's float32 screen has its documented limit on uncentred data.
 10. Reproducibility.  The same call gives the same bits, call to call and stream to stream; the epochs as one call or as several
     calls of fewer (layout's epoch0 and count) give the same bits.
Not built: more than two output dimensions, other metrics, supervised or densmap variants, set_op_mix_ratio != 1,
local_connectivity != 1, the 1e-4 start noise, multi-component spectral layout, a umap_large wrapper, multi-GPU.

On the device the lists come from ra_tsne_knn / ra_tsne_knn_query, rule 2 is ra_umap_smooth_knn, the union is torch plumbing (one
stable sort), rule 6 is ra_umap_epochs (one launch per epoch, no host synchronisation between them) and rule 8 ra_umap_place (one
launch).  backend="numpy" is the float64 checker: the same schedule and generator decisions, no [n][n] array, no GPU.
"""
import argparse
import sys
import warnings

import numpy as np

from . import _common, _graph
from ._common import Launcher, is_int, is_real, ptr

MAX_N, MAX_D = 262144, 2048
MAX_NEIGHBORS = 302
MAX_K = 301                     # list entries of ra_tsne_knn / ra_tsne_knn_query
MAX_EPOCHS = 10000
MAX_NEG = 16
MAX_BATCH = 262144
MAX_NEW = 1 << 48               # rows of one transform: 16 ((row0 + i) k + slot) + s stays below 2^62
TRIPS = 64
STOP = 1e-5
LANES = 16
KEY_SEED, KEY_EPOCH = 0xD1342543DE82EF95, 0xA0761D6478BD642F
MASK = (1 << 64) - 1


class UmapError(ValueError):
    """an input outside the supported domain"""


class UmapWarning(UserWarning):
    """a disconnected graph: the spectral start was replaced by the PCA start"""


def _need(ok, msg):
    if not ok:
        raise UmapError(msg)


def check_options(n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, learning_rate=1.0, negative_sample_rate=5,
                  repulsion_strength=1.0, random_state=42, a=None, b=None):
    """raise UmapError unless the options are inside the supported domain (rule 9)"""
    _need(is_int(n_neighbors) and 2 <= n_neighbors <= MAX_NEIGHBORS,
          "need an integer 2 <= n_neighbors <= %d, got %r" % (MAX_NEIGHBORS, n_neighbors))
    _need(is_real(min_dist) and is_real(spread) and 0 <= min_dist <= spread and spread > 0,
          "need 0 <= min_dist <= spread and spread > 0, got %r and %r" % (min_dist, spread))
    _need(n_epochs is None or (is_int(n_epochs) and 1 <= n_epochs <= MAX_EPOCHS),
          "need an integer 1 <= n_epochs <= %d, got %r" % (MAX_EPOCHS, n_epochs))
    _need(is_real(learning_rate) and learning_rate > 0, "need a finite learning_rate > 0, got %r" % (learning_rate,))
    _need(is_int(negative_sample_rate) and 0 <= negative_sample_rate <= MAX_NEG,
          "need an integer 0 <= negative_sample_rate <= %d, got %r" % (MAX_NEG, negative_sample_rate))
    _need(is_real(repulsion_strength) and repulsion_strength >= 0, "need a finite repulsion_strength >= 0, got %r" % (repulsion_strength,))
    _need(is_int(random_state) and 0 <= random_state < 2 ** 32, "random_state is an integer in 0 .. 2^32 - 1, got %r" % (random_state,))
    for name, v in (("a", a), ("b", b)):
        _need(v is None or (is_real(v) and v > 0), "need a finite %s > 0, got %r" % (name, v))
    _need((a is None) == (b is None), "give both a and b, or neither")


def check_domain(n, d, n_neighbors=15, init="spectral"):
    """raise UmapError unless the shape is inside the supported domain (rule 9)"""
    _need(4 <= n <= MAX_N, "need 4 <= n <= %d points, got %d" % (MAX_N, n))
    _need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    _need(is_int(n_neighbors) and 2 <= n_neighbors <= min(MAX_NEIGHBORS, n),
          "need an integer 2 <= n_neighbors <= min(%d, n = %d), got %r" % (MAX_NEIGHBORS, n, n_neighbors))
    if isinstance(init, str):
        _need(init in ("spectral", "pca", "random"), "init is 'spectral', 'pca', 'random' or an [n][2] array, got %r" % (init,))
        _need(init != "pca" or d >= 2, "init 'pca' needs d >= 2 features (two principal axes), got d = %d" % d)


def default_epochs(n):
    return 500 if n <= 10000 else 200


class UmapResult:
    """embedding float32 [n][2]; graph (indptr int32 [n + 1], indices int32 [nnz], s float64 [nnz]); rho, sigma float64 [n]; a, b;
    n_epochs; init (the start that was used: "spectral", "pca", "random" or "array")"""

    def __init__(self, embedding, graph, rho, sigma, a, b, n_epochs, init):
        self.embedding, self.graph, self.rho, self.sigma = embedding, graph, rho, sigma
        self.a, self.b, self.n_epochs, self.init = float(a), float(b), int(n_epochs), init


class TransformDetails:
    """embedding float32 [n][2], start float32 [n][2] (rule 8's weighted mean), idx int64 [n][k], w float64 [n][k]"""

    def __init__(self, embedding, start, idx, w):
        self.embedding, self.start, self.idx, self.w = embedding, start, idx, w


class SmoothKnn:
    """rule 2 of the checker: rho, sigma [rows], w [rows][k]; margin [rows] = the least |psum - target -+ 1e-5| over the row's trips
    (how close the row came to taking another branch); stopped [rows]: the search met its stop condition; floored [rows]: sigma is
    the floor 1e-3 mean d, not the search's mid"""

    def __init__(self, rho, sigma, w, margin, stopped, floored):
        self.rho, self.sigma, self.w, self.margin, self.stopped, self.floored = rho, sigma, w, margin, stopped, floored


# ---- rule 4

def find_ab(spread=1.0, min_dist=0.1):
    """umap-learn's find_ab_params: (a, b) of the curve 1 / (1 + a x^(2b)) fitted to the membership of (spread, min_dist)"""
    from scipy.optimize import curve_fit
    _need(is_real(min_dist) and is_real(spread) and 0 <= min_dist <= spread and spread > 0,
          "need 0 <= min_dist <= spread and spread > 0, got %r and %r" % (min_dist, spread))

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


# ---- rules 2 and 3 in numpy: the checker

def _list_sum(T):
    """the row sums of T [rows][k], the columns added in list order"""
    s = np.zeros(T.shape[0])
    for j in range(T.shape[1]):
        s = s + T[:, j]
    return s


def psum_numpy(x, sigma):
    """rule 2's psum of the rows x [rows][k] = d - rho at sigma [rows], in list order"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return _list_sum(np.where(x > 0, np.exp(-x / sigma[:, None]), 1.0))


def smooth_knn_numpy(dist2, n_neighbors):
    """rule 2 on squared distances [rows][k]: a SmoothKnn"""
    d = np.sqrt(np.asarray(dist2, np.float64))
    rows, k = d.shape
    pos = d > 0
    rho = np.where(pos.any(axis=1), np.where(pos, d, np.inf).min(axis=1), 0.0)
    x = d - rho[:, None]
    target = float(np.log2(float(n_neighbors)))
    lo, hi, mid = np.zeros(rows), np.full(rows, np.inf), np.ones(rows)
    margin, live = np.full(rows, np.inf), np.ones(rows, bool)
    for _ in range(TRIPS):
        r = np.nonzero(live)[0]
        if r.size == 0:
            break
        ps = psum_numpy(x[r], mid[r])
        diff = ps - target
        margin[r] = np.minimum(margin[r], np.minimum(np.abs(diff - STOP), np.abs(diff + STOP)))
        done = np.abs(diff) < STOP
        up, dn = ~done & (ps > target), ~done & ~(ps > target)
        ru, rd = r[up], r[dn]
        hi[ru] = mid[ru]
        mid[ru] = (lo[ru] + hi[ru]) / 2.0
        lo[rd] = mid[rd]
        mid[rd] = np.where(hi[rd] == np.inf, mid[rd] * 2.0, (lo[rd] + hi[rd]) / 2.0)
        live[r[done]] = False
    floor = 1e-3 * (_list_sum(d) / k)
    sigma = np.maximum(mid, floor)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        w = np.where((x <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-x / sigma[:, None]))
    return SmoothKnn(rho, sigma, w, margin, ~live, floor > mid)


def _union_numpy(idx, w):
    indptr, indices, first, second = _graph.symmetrize_numpy(idx, w)
    return indptr.astype(np.int32), indices.astype(np.int32), first + second - first * second


# ---- rules 5 and 6 in numpy: the checker

def rates(s):
    """rule 5: r = s / max s"""
    s = np.asarray(s, np.float64)
    return s / s.max() if s.size else s.copy()


def fires(rate, t):
    """rule 5: the entries that fire in epoch t"""
    return np.floor(t * rate) > np.floor((t - 1) * rate)


def alpha_at(learning_rate, t, n_epochs):
    return float(learning_rate) * (1.0 - (t - 1) / n_epochs)


def epoch_key(seed, t):
    return (int(seed) * KEY_SEED + int(t) * KEY_EPOCH) & MASK


def _mix(z):
    """splitmix64's finaliser on uint64 arrays (arithmetic mod 2^64)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(seed, t, p, s, count):
    """rule 6's sample s of the entries p (array) in epoch t: indices in 0 .. count - 1, int64"""
    p = np.asarray(p).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = _mix(np.uint64(epoch_key(seed, t)) + np.uint64(16) * p + np.uint64(s))
        return (((z >> np.uint64(32)) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def _sq(dlt):
    return dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]


def _attract(yi, yj, a, b, factor):
    dlt = yi - yj
    q = _sq(dlt)
    ok = q > 0
    qs = np.where(ok, q, 1.0)
    qb = qs ** b
    c = np.where(ok, (((-2.0 * a) * b) * qb / qs) / (1.0 + a * qb), 0.0)
    return np.where(ok[:, None], factor * np.clip(c[:, None] * dlt, -4.0, 4.0), 0.0)


def _repel(yi, yk, a, b, gamma):
    dlt = yi - yk
    q = _sq(dlt)
    ok = q > 0
    qs = np.where(ok, q, 1.0)
    qb = qs ** b
    c = ((2.0 * gamma) * b) / ((0.001 + qs) * (1.0 + a * qb))
    return np.where(ok[:, None], np.clip(c[:, None] * dlt, -4.0, 4.0), 4.0)


def _combine(terms, group, lane, n_groups):
    """terms [e][1 + neg][2] of the firing entries (ascending in walk order within a group and lane) -> sums [n_groups][2]: each
    (group, lane) adds its terms in order, then the 16 lanes combine in the xor tree 8, 4, 2, 1"""
    e, m = terms.shape[0], terms.shape[1]
    key = np.repeat(group * LANES + lane, m)
    out = np.empty((n_groups, 2))
    lanes = np.arange(LANES)
    for c in range(2):
        acc = np.bincount(key, weights=terms[:, :, c].reshape(-1), minlength=n_groups * LANES).reshape(n_groups, LANES)
        for msk in (8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ msk]
        out[:, c] = acc[:, 0]
    return out


def epoch_numpy(Y, indptr, indices, rate, a, b, t, n_epochs, gamma=1.0, negative_sample_rate=5, learning_rate=1.0, random_state=42):
    """rule 6: the float32 positions after epoch t from the float32 positions Y before it"""
    Y32 = np.asarray(Y, np.float32)
    Y64 = Y32.astype(np.float64)
    n = Y64.shape[0]
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    p = np.nonzero(fires(np.asarray(rate, np.float64), t))[0]
    i = _graph.row_ids_numpy(indptr)[p]
    j = indices[p]
    terms = np.empty((len(p), 1 + negative_sample_rate, 2))
    terms[:, 0] = _attract(Y64[i], Y64[j], a, b, 2.0)
    for s in range(negative_sample_rate):
        k = draw(random_state, t, p, s, n)
        terms[:, 1 + s] = np.where((k == i)[:, None], 0.0, _repel(Y64[i], Y64[k], a, b, gamma))
    S = _combine(terms, i, (p - indptr[i]) % LANES, n)
    return (Y64 + alpha_at(learning_rate, t, n_epochs) * S).astype(np.float32)


def place_numpy(y0, Y_fit, idx, rate, a, b, n_epochs=100, gamma=1.0, negative_sample_rate=5, learning_rate=1.0, random_state=42, row0=0):
    """rule 8's optimisation: the float32 positions of the new rows after n_epochs epochs from the start y0"""
    y = np.asarray(y0, np.float32).copy()
    F64 = np.asarray(Y_fit, np.float32).astype(np.float64)
    idx, rate = np.asarray(idx, np.int64), np.asarray(rate, np.float64)
    n, k = idx.shape
    m = F64.shape[0]
    for t in range(1, n_epochs + 1):
        i, slot = np.nonzero(fires(rate, t))
        y64 = y.astype(np.float64)
        terms = np.empty((len(i), 1 + negative_sample_rate, 2))
        terms[:, 0] = _attract(y64[i], F64[idx[i, slot]], a, b, 1.0)
        p = (row0 + i) * k + slot
        for s in range(negative_sample_rate):
            terms[:, 1 + s] = _repel(y64[i], F64[draw(random_state, t, p, s, m)], a, b, gamma)
        y = (y64 + alpha_at(learning_rate, t, n_epochs) * _combine(terms, i, slot % LANES, n)).astype(np.float32)
    return y


def start_numpy(Y_fit, idx, w):
    """rule 8's start: sum_j w_ij Y_j / sum_j w_ij in list order, rounded to float32"""
    F64 = np.asarray(Y_fit, np.float32).astype(np.float64)
    num, den = np.zeros((idx.shape[0], 2)), np.zeros(idx.shape[0])
    for j in range(idx.shape[1]):
        num = num + w[:, j, None] * F64[idx[:, j]]
        den = den + w[:, j]
    return (num / den[:, None]).astype(np.float32)


# ---- the same on the device

class _Device(Launcher):
    """rules 2, 3, 6 and 8 on the current stream of X's device (rule 1's lists are _graph.knn's and knn_query's)"""

    def smooth_knn(self, d2, n_neighbors):
        torch = self.torch
        rows, k = (int(s) for s in d2.shape)
        rho = torch.empty(rows, dtype=torch.float64, device=self.dev)
        sigma = torch.empty(rows, dtype=torch.float64, device=self.dev)
        w = torch.empty((rows, k), dtype=torch.float64, device=self.dev)
        self.call("ra_umap_smooth_knn", ptr(d2), rows, k, int(n_neighbors), ptr(rho), ptr(sigma), ptr(w))
        return rho, sigma, w

    def union(self, idx, w):
        indptr, indices, first, second = _graph.symmetrize_torch(idx, w)
        return indptr.to(self.torch.int32), indices.to(self.torch.int32), first + second - first * second

    def epochs(self, y, indptr, indices, rate, a, b, gamma, neg, lr, n_epochs, epoch0, count, seed):
        """`count` epochs from epoch0 on the float32 tensor y [n][2]; returns the tensor that holds the result"""
        alt = self.torch.empty_like(y)
        self.call("ra_umap_epochs", ptr(y), ptr(alt), int(y.shape[0]), ptr(indptr), ptr(indices), ptr(rate), int(indices.numel()),
                  float(a), float(b), float(gamma), int(neg), float(lr), int(n_epochs), int(epoch0), int(count), int(seed))
        return alt if count % 2 else y

    def place(self, y, row0, yfit, idx, rate, a, b, gamma, neg, lr, n_epochs, seed):
        n, k = (int(s) for s in idx.shape)
        self.call("ra_umap_place", ptr(y), n, int(row0), ptr(yfit), int(yfit.shape[0]), ptr(idx), ptr(rate), k, float(a), float(b),
                  float(gamma), int(neg), float(lr), int(n_epochs), int(seed))
        return y

    def start(self, yfit, idx, w):
        """rule 8's start, the list slots added one after another (elementwise kernels: a fixed order, no fused multiply-add)"""
        torch = self.torch
        F = yfit.to(torch.float64)
        num = torch.zeros((idx.shape[0], 2), dtype=torch.float64, device=self.dev)
        den = torch.zeros(idx.shape[0], dtype=torch.float64, device=self.dev)
        for j in range(int(idx.shape[1])):
            num = num + w[:, j, None] * F[idx[:, j].long()]
            den = den + w[:, j]
        return (num / den[:, None]).to(torch.float32).contiguous()


def _graph_device(X, n_neighbors):
    D = _Device(X)
    with D.torch.cuda.device(D.dev):
        idx, d2 = _graph.knn(D, X, n_neighbors - 1)
        rho, sigma, w = D.smooth_knn(d2, n_neighbors)
        indptr, indices, s = D.union(idx, w)
    return D, indptr, indices, s, rho, sigma


def _graph_numpy(X, n_neighbors):
    from . import tsne
    idx, d2 = tsne.knn_numpy(X, n_neighbors - 1)
    sk = smooth_knn_numpy(d2, n_neighbors)
    return _union_numpy(idx, sk.w) + (sk.rho, sk.sigma)


def _input(X, n_neighbors, init, backend):
    X = _common.as_input(X, backend, UmapError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, n_neighbors, init)
    _common.check_finite(X, backend, UmapError)
    return X


def fuzzy_graph(X, n_neighbors=15, backend="device"):
    """rules 1 - 3 of X [n][d]: (indptr int32 [n + 1], indices int32 [nnz], s float64 [nnz], rho [n], sigma [n]) as numpy arrays"""
    X = _input(X, n_neighbors, None, backend)
    if backend == "numpy":
        return _graph_numpy(X, n_neighbors)
    _, indptr, indices, s, rho, sigma = _graph_device(X, n_neighbors)
    return tuple(v.cpu().numpy() for v in (indptr, indices, s, rho, sigma))


# ---- rule 7

def rescale(F):
    """rule 7: every coordinate to [0, 10] in double (zero range: 5), rounded to float32"""
    F = np.asarray(F, np.float64)
    lo, hi = F.min(axis=0), F.max(axis=0)
    rng = hi - lo
    out = np.where(rng > 0, 10.0 * (F - lo) / np.where(rng > 0, rng, 1.0), 5.0)
    return np.ascontiguousarray(out, np.float32)


def pca_start(X):
    """the first two principal axes of X (float64 eigh on the host), rescaled"""
    from .sdr import fix_signs
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = fix_signs(V[:, np.argsort(w, kind="stable")[::-1][:2]])
    return rescale(Xc @ V)


def n_components(indptr, indices):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(indptr) - 1
    return int(connected_components(csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n)), directed=False)[0])


def _host(X):
    return X.detach().cpu().numpy() if hasattr(X, "detach") else np.asarray(X)


def initial_embedding(X, graph, init="spectral", random_state=42, backend="device"):
    """rule 7: (Y0 float32 [n][2], the name of the start that was used)"""
    n, d = (int(s) for s in X.shape)
    if not isinstance(init, str):
        Y = np.ascontiguousarray(_host(init), np.float32)
        _need(Y.shape == (n, 2), "an init array is [n][2] = [%d][2], got %s" % (n, Y.shape))
        _need(bool(np.all(np.isfinite(Y))), "the init array holds NaN or infinite values")
        return Y, "array"
    if init == "random":
        return np.ascontiguousarray(np.random.RandomState(random_state).uniform(-10.0, 10.0, (n, 2)), np.float32), "random"
    if init == "spectral":
        from . import spectral
        indptr, indices, s = graph
        nc = n_components(indptr, indices)
        why = "the fuzzy graph has %d connected components" % nc if nc > 1 else None
        if why is None:
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", spectral.SpectralWarning)
                    E = spectral.embedding_from_graph(indptr, indices, s, n_components=2, backend=backend).embedding
                if np.all(np.isfinite(E)):
                    return rescale(E), "spectral"
                why = "the spectral start is not finite"
            except spectral.SpectralError as e:
                why = "the spectral start failed (%s)" % e
        _need(d >= 2, "%s and the 'pca' start needs d >= 2 features: use init='random'" % why)
        warnings.warn("%s: the 'pca' start is used instead of the spectral one" % why, UmapWarning, stacklevel=3)
    return pca_start(_host(X)), "pca"


# ---- rules 5 and 6: the layout

def _check_csr(indptr, indices, s, n_min=4):
    indptr, indices, s = np.asarray(indptr), np.asarray(indices), np.asarray(s, np.float64)
    _need(indptr.ndim == 1 and indices.ndim == 1 and s.ndim == 1 and len(indptr) >= 2, "indptr [n + 1], indices [nnz] and s [nnz] are 1-D")
    _need(np.issubdtype(indptr.dtype, np.integer) and np.issubdtype(indices.dtype, np.integer), "indptr and indices hold integers")
    n = len(indptr) - 1
    _need(n_min <= n <= MAX_N, "need %d <= n <= %d rows, got %d" % (n_min, MAX_N, n))
    _need(indptr[0] == 0 and bool(np.all(np.diff(indptr) >= 0)) and indptr[-1] == len(indices) == len(s) and len(s) <= 2 * n * MAX_K,
          "indptr ascends from 0 to nnz = len(indices) = len(s) <= 2 n %d" % MAX_K)
    _need(len(indices) == 0 or (indices.min() >= 0 and indices.max() < n), "a column index is outside 0 .. n - 1")
    _need(bool(np.all(np.isfinite(s))) and bool(np.all(s >= 0)), "the weights are finite and >= 0")
    return indptr.astype(np.int32), indices.astype(np.int32), s


def layout(indptr, indices, s, Y0, a, b, n_epochs=None, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0, random_state=42,
           epoch0=1, count=None, backend="device"):
    """rules 5 and 6 on a symmetric CSR graph from anywhere (numpy arrays) from the start Y0 [n][2]: the float32 positions after the
    epochs epoch0 .. epoch0 + count - 1 (default: all of them up to n_epochs) of a schedule of n_epochs"""
    _need(backend in ("device", "numpy"), "backend is 'device' or 'numpy', got %r" % (backend,))
    indptr, indices, s = _check_csr(indptr, indices, s)
    n = len(indptr) - 1
    n_epochs = default_epochs(n) if n_epochs is None else n_epochs
    check_options(2, 0.0, 1.0, n_epochs, learning_rate, negative_sample_rate, repulsion_strength, random_state, a, b)
    _need(a is not None, "layout needs a and b")
    count = n_epochs - epoch0 + 1 if count is None else count
    _need(is_int(epoch0) and is_int(count) and epoch0 >= 1 and count >= 1 and epoch0 + count - 1 <= n_epochs,
          "need epoch0 >= 1, count >= 1 and epoch0 + count - 1 <= n_epochs, got %r and %r" % (epoch0, count))
    Y = np.ascontiguousarray(_host(Y0), np.float32)
    _need(Y.shape == (n, 2) and bool(np.all(np.isfinite(Y))), "Y0 is a finite [n][2] = [%d][2] array" % n)
    rate = rates(s)
    if backend == "numpy":
        for t in range(epoch0, epoch0 + count):
            Y = epoch_numpy(Y, indptr, indices, rate, a, b, t, n_epochs, repulsion_strength, negative_sample_rate, learning_rate,
                            random_state)
        return Y
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    D = _Device(dev)
    with torch.cuda.device(dev):
        ip, ix, rt, y = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (indptr, indices, rate, Y))
        return D.epochs(y, ip, ix, rt, a, b, repulsion_strength, negative_sample_rate, learning_rate, n_epochs, epoch0, count,
                        random_state).cpu().numpy()


def umap(X, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0,
         init="spectral", random_state=42, a=None, b=None, backend="device"):
    """UMAP of X [n][d] by the rules at the top of this module: a UmapResult.  backend="device" takes a contiguous float32 CUDA tensor
    (a numpy array is copied) and works on the current stream."""
    check_options(n_neighbors, min_dist, spread, n_epochs, learning_rate, negative_sample_rate, repulsion_strength, random_state, a, b)
    X = _input(X, n_neighbors, init, backend)
    n = int(X.shape[0])
    n_epochs = default_epochs(n) if n_epochs is None else n_epochs
    if a is None:
        a, b = find_ab(spread, min_dist)
    if backend == "numpy":
        indptr, indices, s, rho, sigma = _graph_numpy(X, n_neighbors)
        Y, used = initial_embedding(X, (indptr, indices, s), init, random_state, backend)
        rate = rates(s)
        for t in range(1, n_epochs + 1):
            Y = epoch_numpy(Y, indptr, indices, rate, a, b, t, n_epochs, repulsion_strength, negative_sample_rate, learning_rate,
                            random_state)
        return UmapResult(Y, (indptr, indices, s), rho, sigma, a, b, n_epochs, used)
    D, ip, ix, sv, rho, sigma = _graph_device(X, n_neighbors)
    torch = D.torch
    with torch.cuda.device(D.dev):
        graph = (ip.cpu().numpy(), ix.cpu().numpy(), sv.cpu().numpy())
        Y0, used = initial_embedding(X, graph, init, random_state, backend)
        y = torch.from_numpy(Y0).to(D.dev)
        y = D.epochs(y, ip, ix, (sv / sv.max()).contiguous(), a, b, repulsion_strength, negative_sample_rate, learning_rate, n_epochs, 1,
                     n_epochs, random_state)
        return UmapResult(y.cpu().numpy(), graph, rho.cpu().numpy(), sigma.cpu().numpy(), a, b, n_epochs, used)


# ---- rule 8

def check_transform_domain(n, m, d, n_neighbors=15, batch=65536):
    for name, v in (("n", n), ("m", m), ("d", d), ("batch", batch)):
        _need(is_int(v), "%s must be an integer, got %r" % (name, v))
    _need(0 <= n <= MAX_NEW, "need 0 <= n <= 2^48 new points, got %d" % n)
    _need(2 <= m <= MAX_N, "need 2 <= m <= %d fitted points, got %d" % (MAX_N, m))
    _need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    _need(min(m, n_neighbors) <= MAX_K, "the placement lists min(m, n_neighbors) <= %d fitted rows, got %d" % (MAX_K, min(m, n_neighbors)))
    _need(1 <= batch <= MAX_BATCH, "need 1 <= batch <= %d, got %d" % (MAX_BATCH, batch))


def transform(X_new, X_fit, Y_fit, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=100, learning_rate=1.0, negative_sample_rate=5,
              repulsion_strength=1.0, random_state=42, a=None, b=None, batch=65536, backend="device", details=False):
    """Place X_new [n][d] into the embedding Y_fit [m][2] of X_fit [m][d] (rule 8): the embedding [n][2] float32, or with details
    TransformDetails(embedding, start, idx [n][k], w [n][k]), as numpy arrays; tsne.vote_labels takes idx and w as they are.
    backend="device": X_fit and Y_fit are contiguous float32 CUDA tensors (numpy arrays are copied to the current device); X_new is
    such a tensor too, or a numpy array of any size, copied one batch at a time."""
    _need(backend in ("device", "numpy"), "backend is 'device' or 'numpy', got %r" % (backend,))
    check_options(n_neighbors, min_dist, spread, n_epochs, learning_rate, negative_sample_rate, repulsion_strength, random_state, a, b)
    host_new = backend == "numpy" or isinstance(X_new, np.ndarray)
    Xn = _common.as_input(X_new, "numpy" if host_new else "device", UmapError, numpy_on_device=False)
    Xf, Yf = _common.as_input(X_fit, backend, UmapError), _common.as_input(Y_fit, backend, UmapError)
    if backend == "numpy":
        Xf, Yf = np.ascontiguousarray(Xf, np.float32), np.ascontiguousarray(Yf, np.float32)
    else:
        _need(Yf.device == Xf.device and (host_new or Xn.device == Xf.device), "X_new, X_fit and Y_fit are on different devices")
    (n, d), m = (int(s) for s in Xn.shape), int(Xf.shape[0])
    _need(tuple(Yf.shape) == (m, 2), "Y_fit is [m][2] = [%d][2], got %s" % (m, tuple(Yf.shape)))
    _need(int(Xf.shape[1]) == d, "X_new has %d features, X_fit %d" % (d, int(Xf.shape[1])))
    check_transform_domain(n, m, d, n_neighbors, batch)
    _common.check_finite(Xf, backend, UmapError)
    _common.check_finite(Yf, backend, UmapError)
    _need(_common.host_finite(Xn) if host_new else bool(Xn.isfinite().all().item()), "X holds NaN or infinite values")
    if a is None:
        a, b = find_ab(spread, min_dist)
    k = min(m, n_neighbors)
    emb, start = np.empty((n, 2), np.float32), np.empty((n, 2), np.float32)
    if details:
        idx_all, w_all = np.empty((n, k), np.int64), np.empty((n, k), np.float64)

    def run(torch=None, D=None):
        from . import tsne
        for s in range(0, n, batch):
            e = min(n, s + batch)
            if D is None:
                idx, d2 = tsne.knn_query_numpy(np.asarray(Xn[s:e], np.float32), Xf, k)
                w = smooth_knn_numpy(d2, n_neighbors).w
                y0 = start_numpy(Yf, idx, w)
                emb[s:e] = place_numpy(y0, Yf, idx, w / w.max(axis=1)[:, None], a, b, n_epochs, repulsion_strength, negative_sample_rate,
                                       learning_rate, random_state, s)
                start[s:e] = y0
            else:
                xb = torch.from_numpy(np.ascontiguousarray(Xn[s:e], np.float32)).to(D.dev) if host_new else Xn[s:e]
                idx, d2 = _graph.knn_query(D, xb, Xf, k)
                w = D.smooth_knn(d2, n_neighbors)[2]
                y = D.start(Yf, idx, w)
                start[s:e] = y.cpu().numpy()
                rate = (w / w.max(dim=1).values[:, None]).contiguous()
                emb[s:e] = D.place(y, s, Yf, idx, rate, a, b, repulsion_strength, negative_sample_rate, learning_rate, n_epochs,
                                   random_state).cpu().numpy()
            if details:
                idx_all[s:e] = idx if D is None else idx.cpu().numpy()
                w_all[s:e] = w if D is None else w.cpu().numpy()

    if backend == "numpy":
        run()
    elif n:
        import torch
        with torch.cuda.device(Xf.device):
            run(torch, _Device(Xf.device))
    return TransformDetails(emb, start, idx_all, w_all) if details else emb


# ---- command line

def _fit_options(path):
    """(embedding, the options a placement takes from the fit's OUT.npz)"""
    with np.load(path) as z:
        _need("embedding" in z.files, "%s has no array 'embedding' (it holds %s)" % (path, ", ".join(z.files)))
        opts = {k: z[k].item() for k in ("a", "b", "n_neighbors", "seed", "negative_sample_rate") if k in z.files}
        return np.ascontiguousarray(z["embedding"], np.float32), opts


def _add_quality(out, X, k, backend):
    """--quality: the scores of out["embedding"] against the rows X into out; returns their part of the summary line"""
    from . import quality
    q = quality.embedding_quality(X, out["embedding"], k, backend=backend)
    out.update(trustworthiness=np.float64(q.trustworthiness), continuity=np.float64(q.continuity), trust_point=q.trust_point,
               cont_point=q.cont_point)
    return ", trustworthiness %.6f, continuity %.6f (k = %d)" % (q.trustworthiness, q.continuity, k)


def main(argv=None):
    from . import tsne
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.umap")
    _common.add_cluster_arguments(ap, ("input", "output", "--key"), "factors", False)
    ap.add_argument("--n_neighbors", type=int, default=None, help="the row itself and n_neighbors - 1 others (default 15; with "
                    "--place_into the fit's)")
    ap.add_argument("--min_dist", type=float, default=0.1)
    ap.add_argument("--spread", type=float, default=1.0)
    ap.add_argument("--n_epochs", type=int, default=None, help="default 500 up to 10000 rows, else 200; 100 with --place_into")
    ap.add_argument("--learning_rate", type=float, default=1.0)
    ap.add_argument("--negative_sample_rate", type=int, default=None, help="default 5; with --place_into the fit's")
    ap.add_argument("--init", default="spectral", help="spectral, pca, random or an [n][2] .npy")
    ap.add_argument("--seed", type=int, default=None, help="random_state (default 42; with --place_into the fit's)")
    _common.add_cluster_arguments(ap, ("--backend", "--device"), "factors", False)
    ap.add_argument("--quality", type=int, nargs="?", const=10, default=None, metavar="K",
                    help="add trustworthiness, continuity, trust_point and cont_point at K neighbours (default 10) to OUT.npz")
    ap.add_argument("--place_into", default=None, help="OUT.npz of an earlier run: place the input's rows into its embedding")
    ap.add_argument("--fit_input", default=None, help="the rows the embedding of --place_into was fitted on (.npz or .npy)")
    ap.add_argument("--fit_key", default="factors", help="array of an .npz --fit_input (default factors)")
    ap.add_argument("--fit_labels", default=None, help="int .npy, or OUT.npz of a clustering tool (its labels), one label per fitted "
                    "row: adds labels and label_confidence by the neighbour vote")
    ap.add_argument("--batch", type=int, default=None, help="new rows on the device at a time (default 65536)")
    args = ap.parse_args(argv)
    if args.place_into is not None and args.fit_input is None:
        ap.error("--place_into needs --fit_input (the rows its embedding was fitted on)")
    if args.place_into is None:
        given = [o for o in ("fit_input", "fit_labels", "batch") if getattr(args, o) is not None]
        if given:
            ap.error("--%s needs --place_into" % given[0])
    place = args.place_into is not None
    try:
        X = _common.read_input(args.input, args.key, UmapError)
        n, d = X.shape
        opts, Xf, Yf, labels_fit = {}, None, None, None
        if place:
            Xf = _common.read_input(args.fit_input, args.fit_key, UmapError)
            Yf, opts = _fit_options(args.place_into)
            labels_fit = tsne.read_fit_labels(args.fit_labels) if args.fit_labels else None
        init = args.init if args.init in ("spectral", "pca", "random") else np.load(args.init)
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    n_neighbors = args.n_neighbors if args.n_neighbors is not None else int(opts.get("n_neighbors", 15))
    seed = args.seed if args.seed is not None else int(opts.get("seed", 42))
    neg = args.negative_sample_rate if args.negative_sample_rate is not None else int(opts.get("negative_sample_rate", 5))
    kw = dict(n_neighbors=n_neighbors, learning_rate=args.learning_rate, negative_sample_rate=neg, random_state=seed, backend=args.backend)
    try:
        check_options(n_neighbors, args.min_dist, args.spread, args.n_epochs, args.learning_rate, neg, 1.0, seed)
        if place:
            m = Xf.shape[0]
            if Yf.shape != (m, 2):
                ap.error("%s holds an embedding %s, %s has %d rows" % (args.place_into, Yf.shape, args.fit_input, m))
            if Xf.shape[1] != d:
                ap.error("%s has %d features, %s %d" % (args.input, d, args.fit_input, Xf.shape[1]))
            if labels_fit is not None and labels_fit.shape[0] != m:
                ap.error("%s holds %d labels for %d fitted rows" % (args.fit_labels, labels_fit.shape[0], m))
            check_transform_domain(n, m, d, n_neighbors, 65536 if args.batch is None else args.batch)
        else:
            check_domain(n, d, n_neighbors, init)
            if not isinstance(init, str):
                _need(init.shape == (n, 2), "%s holds %s, the input has %d rows" % (args.init, init.shape, n))
    except UmapError as e:
        ap.error(str(e))
    if args.quality is not None:
        from . import quality
        quality.check_tool_arguments(ap, n, n, args.quality, None)
    if args.backend == "device":
        _common.require_gpu("no GPU visible: use --backend numpy for the CPU checker")

    def run():
        on_device = args.backend == "device" and (not place or args.quality is not None)
        x = _common.to_device(X, args.device) if on_device else X
        if place:
            if "a" in opts and "b" in opts:
                kw.update(a=float(opts["a"]), b=float(opts["b"]))
            else:
                kw.update(min_dist=args.min_dist, spread=args.spread)
            res = transform(X, Xf, Yf, n_epochs=100 if args.n_epochs is None else args.n_epochs,
                            batch=65536 if args.batch is None else args.batch, details=True, **kw)
            a, b = (kw["a"], kw["b"]) if "a" in kw else find_ab(args.spread, args.min_dist)
            out = dict(embedding=res.embedding, a=np.float64(a), b=np.float64(b),
                       n_epochs=np.int64(100 if args.n_epochs is None else args.n_epochs), init=np.str_("weighted"))
            if labels_fit is not None:
                out["labels"], out["label_confidence"] = tsne.vote_labels(res.idx, res.w, labels_fit)
            head = "%d points x %d placed against %d fitted" % (n, d, Xf.shape[0])
        else:
            res = umap(x, min_dist=args.min_dist, spread=args.spread, n_epochs=args.n_epochs, init=init, **kw)
            out = dict(embedding=res.embedding, a=np.float64(res.a), b=np.float64(res.b), n_epochs=np.int64(res.n_epochs),
                       init=np.str_(res.init))
            head = "%d points x %d, %d epochs from the %s start, a %.6f, b %.6f" % (n, d, res.n_epochs, res.init, res.a, res.b)
        out.update(n_neighbors=np.int64(n_neighbors), min_dist=np.float64(args.min_dist), spread=np.float64(args.spread),
                   learning_rate=np.float64(args.learning_rate), negative_sample_rate=np.int64(neg),
                   repulsion_strength=np.float64(1.0), seed=np.int64(seed), key=np.str_(args.key), backend=np.str_(args.backend))
        return out, head + (_add_quality(out, x, args.quality, args.backend) if args.quality is not None else "")
    try:
        if args.backend == "device":
            import torch
            with torch.cuda.device(args.device), warnings.catch_warnings():
                warnings.simplefilter("always", UmapWarning)
                out, msg = run()
        else:
            out, msg = run()
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    np.savez(args.output, **out)
    print("%s: %s" % (args.output, msg))
    return 0


if __name__ == "__main__":
    sys.exit(main())
