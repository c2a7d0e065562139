"""Ward (minimum-variance) hierarchical clustering of factors or embeddings X [n][d] on the GPU (after scipy 1.15
scipy.cluster.hierarchy.ward and scikit-learn 1.7 AgglomerativeClustering(linkage="ward")).

    python -m cryo_ralib_amd.ward IN OUT.npz (--k K | --distance_threshold T | --sweep K1,K2,...|LO:HI[:STEP])
                                  [--key factors] [--backend device|numpy] [--scores] [--sample_size N] [--seed S] [--truth FILE]
                                  [--stack STACK --params PARAMS --ou R --averages REFS.{hdf,mrcs,npy}]

IN is the OUT.npz of the sdr tool (--key factors, the default) or of the tsne tool (--key embedding), or an [n][d] .npy.  OUT.npz
holds labels, linkage (scipy's Z), n_clusters, counts, inertia (the within-class sum of squares of the cut), n_rounds,
rows_evaluated and the options used.  --scores adds what the kmeans tool adds (silhouette, class_silhouette, silhouette_samples,
calinski_harabasz, davies_bouldin).  --sweep builds ONE tree and adds the table `sweep` (k, inertia, silhouette, CH, DB) and
best_k; the labels written are those of --k if given, else of best_k.  --truth adds purity, c_purity and contingency; --averages
writes the class averages of the stack (kmeans.class_averages): a refstack for the multi-reference command line, at most 256
classes.  OUT.npz has a `labels` key, so the tsne tool's --fit_labels takes it as it is.

One tree gives every k: a merge's W2 is the increase of the within-class sum of squares, so inertia(k) is a prefix sum of the
sorted W2, and the classes at a smaller k are unions of those at a larger k.

The contract, rule by rule:
  1. Input.  X [n][d] float32 converts to double exactly.  A cluster is (centroid c in double, size s) and lives in a slot
     0 .. n - 1.  Point i starts as the cluster (x_i, 1) in slot i.
  2. Distance.  D2(a, b) is dbscan.py's rule 2 on the centroids: differences in double, the features in order, one chain per pair.
     W2(a, b) = f D2 with f = (s_a s_b) / (s_a + s_b); the sizes go to double first and s_a s_b is exact.  W2 is the increase of
     the within-class sum of squares if a and b merge; the scipy / sklearn height is sqrt(2 W2).  Every comparison is on W2; the
     square root is taken once per merge, on the host.
  3. Nearest neighbour.  nn(a) is the live slot b != a that minimises (W2(a, b), b): ties go to the lower slot.
  4. Rounds.  Every live cluster keeps a record (nn, w).  A round re-evaluates the records of the stale rows (all rows in round
     0), then merges every reciprocal pair nn(a) = b, nn(b) = a, a < b; at least one member of such a pair is stale, so only stale
     rows are examined.  A merge writes c_a <- (s_a c_a + s_b c_b) / (s_a + s_b), s_a <- s_a + s_b, and slot b dies, so a slot
     always equals its cluster's lowest member index.  The merged clusters are stale in the next round, and so are the live
     clusters whose recorded nn was consumed (was a member of a merged pair).  Other records stay valid: Ward's criterion is
     reducible, W2(a u b, c) >= min(W2(a, c), W2(b, c)).  If a round finds no reciprocal pair the next round re-evaluates every
     live row (in exact arithmetic on tie-free data this cannot happen; after a full re-evaluation a pair exists, because the
     lowest slot among the clusters at the least W2 is reciprocal with its nn); a second empty round in a row raises.  The loop
     ends after exactly n - 1 merges.
  5. Tree.  Merges are sorted by (W2, round, a); a parent is always in a later round than its children, so it follows them even
     at equal height.  Merge r creates node n + r; Z[r] = (min(id), max(id), sqrt(2 W2), size) is scipy's linkage layout and
     children = Z[:, :2] is sklearn's children_.  inertia(k) = the sum of the first n - k sorted W2, in double, in that order.
  6. Cuts.  n_clusters = k undoes the last k - 1 merges; distance_threshold = t applies exactly the merges with height < t
     (sklearn's rule: n_clusters_ = count(height >= t) + 1).  Labels are numbered 0 .. k - 1 by lowest member index, as in
     dbscan.py and hdbscan.py; sklearn numbers them by heap order, so compare up to a renaming.
  7. Function of the data.  The result is a pure function of X, bitwise reproducible call to call and stream to stream.  On
     tie-free data it is the greedy Ward dendrogram, equal to scipy's up to rounding of the heights, and permuting the rows
     permutes the labels.  With ties it is defined by rules 3 - 5 and may differ from scipy.  Exact duplicates stay exact:
     (s_a c + s_b c) / (s_a + s_b) = c bit for bit, because c has 24 significant bits and the sizes stay below 2^29.
  8. Device versus checker.  The device fuses each multiply-add of the D2 chain and of the centroid update; the numpy checker does
     not.  Decisions can therefore differ only where two candidates' W2 agree to rounding.  The checker reports margin, the least
     (second - least) / second over every evaluated row with two candidates, and height_gap, the least relative gap of
     consecutive sorted heights.
Domain: 2 <= n <= 262144, 1 <= d <= 2048, finite X; 1 <= n_clusters <= n; distance_threshold > 0; exactly one of the two is given.
Anything else raises WardError (a ValueError) before anything is launched.
Not built: other linkages (average and complete linkage need the n^2 matrix), connectivity constraints, other metrics,
compute_full_tree=False, more than 262144 points, multi-GPU.

On the device the cluster table is X.double() and an int32 size per slot.  Per round the host uploads the stale list, calls
ra_ward_nearest (csrc/ralign_ward.h: 64 listed rows per workgroup against the padded list of the live columns in 64 x 64 double
tiles; nothing of size n^2 is stored), reads back 12 bytes per stale row in one copy, finds the reciprocal pairs among the stale
rows with numpy, uploads them and calls ra_ward_merge: one synchronisation per round.  At most n - 1 rounds; data whose nearest
neighbours form one long chain (points on a line with growing gaps) costs one launch and one synchronisation per merge.
backend="numpy" is the float64 checker: the same rounds with unfused arithmetic, the rows in chunks (_common.row_chunks) so that
no [n][n] array is built; it needs no GPU.  greedy_numpy is a second, independent checker for tests: the literal definition.
"""
import argparse
import sys

import numpy as np

from . import _common, _graph
from ._common import Launcher, is_int, is_real, ptr, row_chunks

MAX_N, MAX_D = 262144, 2048
MAX_AVERAGES = 256          # kmeans.class_averages' limit on the number of classes
MAX_GREEDY_N = 200


class WardError(ValueError):
    """an input outside the supported domain"""


def check_domain(n, d):
    """raise WardError unless the shape is inside the supported domain"""
    if not 2 <= n <= MAX_N:
        raise WardError("need 2 <= n <= %d points, got %d" % (MAX_N, n))
    if not 1 <= d <= MAX_D:
        raise WardError("need 1 <= d <= %d features, got %d" % (MAX_D, d))


def check_cut(n, n_clusters=None, distance_threshold=None):
    """raise WardError unless exactly one of n_clusters (an integer in 1 .. n) and distance_threshold (a finite real > 0) is given"""
    if (n_clusters is None) == (distance_threshold is None):
        raise WardError("exactly one of n_clusters and distance_threshold is needed")
    if n_clusters is not None and not (is_int(n_clusters) and 1 <= n_clusters <= n):
        raise WardError("need an integer 1 <= n_clusters <= n = %d, got %r" % (n, n_clusters))
    if distance_threshold is not None and not (is_real(distance_threshold) and distance_threshold > 0):
        raise WardError("need a finite distance_threshold > 0, got %r" % (distance_threshold,))


class WardTree:
    """n, d; Z float64 [n - 1][4] (scipy's linkage: the two node ids, the height sqrt(2 W2), the size); children int64 [n - 1][2]
    (sklearn's children_); heights and w2 float64 [n - 1], ascending; merges int64 [n - 1][2] (the slots a < b of every merge, in
    the tree's order) and merge_round int64 [n - 1]; n_rounds; rows_evaluated (the rows re-evaluated over all rounds); with
    details (numpy backend) margin and height_gap of rule 8, else None"""

    def __init__(self, n, d, merges, w2, merge_round, children, sizes, n_rounds, rows_evaluated, margin=None):
        self.n, self.d, self.merges, self.w2, self.merge_round = int(n), int(d), merges, w2, merge_round
        self.heights = np.sqrt(2.0 * w2)
        self.children = children
        self.Z = np.column_stack([children.astype(np.float64), self.heights, sizes.astype(np.float64)])
        self.n_rounds, self.rows_evaluated = int(n_rounds), int(rows_evaluated)
        self.margin = self.height_gap = None
        if margin is not None:
            self.margin = float(margin)
            h0, h1 = self.heights[:-1], self.heights[1:]
            gap = np.where(h1 > 0, (h1 - h0) / np.where(h1 > 0, h1, 1.0), 0.0)
            self.height_gap = float(gap.min()) if gap.size else float("inf")
        self._prefix = np.concatenate([[0.0], np.cumsum(w2)])           # a sequential sum in the tree's order

    def inertia(self, k):
        """the within-class sum of squares of cut(n_clusters=k): the sum of the first n - k sorted W2 (rule 5)"""
        if not (is_int(k) and 1 <= k <= self.n):
            raise WardError("need an integer 1 <= k <= n = %d, got %r" % (self.n, k))
        return float(self._prefix[self.n - int(k)])


class WardResult:
    """labels int32 [n], n_clusters, counts int64 [k], centers float64 [k][d] (the class centroids), inertia and the WardTree"""

    def __init__(self, labels, centers, tree):
        self.labels, self.centers, self.tree = labels, centers, tree
        self.n_clusters = int(labels.max()) + 1
        self.counts = np.bincount(labels, minlength=self.n_clusters).astype(np.int64)
        self.inertia = tree.inertia(self.n_clusters)


# ---- rule 2 - 3 on the host: the checker's row function

def rows_numpy(C, size, rows, details=False):
    """(nn int64, w float64[, margin]) of the listed slots against the live slots of the state (C float64 [n][d], size [n]):
    rule 2 unfused, rule 3's ties to the lower slot.  A listed slot that is dead or outside 0 .. n - 1, or the only live one,
    gives (-1, +inf).  margin: the least (second - least) / second over the rows with two candidates (inf without any)."""
    C, size, rows = np.asarray(C, np.float64), np.asarray(size), np.asarray(rows, np.int64)
    n, d = C.shape
    live = np.nonzero(size > 0)[0]
    nn, w, margin = np.full(len(rows), -1, np.int64), np.full(len(rows), np.inf), np.inf
    inside = (rows >= 0) & (rows < n)
    ok = np.nonzero(inside & (size[np.where(inside, rows, 0)] > 0))[0]
    if len(live) < 2 or not len(ok):
        return (nn, w, margin) if details else (nn, w)
    sb, Cb = size[live].astype(np.float64), C[live]
    ch = max(1, (1 << 22) // len(live))
    for s0 in range(0, len(ok), ch):
        pos = ok[s0:s0 + ch]
        a = rows[pos]
        D = np.zeros((len(a), len(live)))
        for t in range(d):
            df = C[a, t, None] - Cb[None, :, t]
            D += df * df
        sa = size[a].astype(np.float64)[:, None]
        W = (sa * sb[None, :]) / (sa + sb[None, :]) * D
        W[np.arange(len(a)), np.searchsorted(live, a)] = np.inf             # b != a
        j = np.argmin(W, axis=1)                                            # the first least: the lowest slot
        nn[pos], w[pos] = live[j], W[np.arange(len(a)), j]
        if details and len(live) >= 3:
            two = np.partition(W, 1, axis=1)[:, :2]
            with np.errstate(invalid="ignore", divide="ignore"):
                m = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
            margin = min(margin, float(m.min()))
    return (nn, w, margin) if details else (nn, w)


class _NumpyState:
    """the checker's cluster table: rule 4's update unfused, in the order written"""

    def __init__(self, X, details):
        self.C, self.size = np.array(X, np.float64), np.ones(X.shape[0], np.int64)
        self.details, self.margin = details, np.inf

    def nearest(self, rows):
        out = rows_numpy(self.C, self.size, rows, self.details)
        if self.details:
            self.margin = min(self.margin, out[2])
        return out[0], out[1]

    def merge(self, a, b):
        sa, sb = self.size[a].astype(np.float64)[:, None], self.size[b].astype(np.float64)[:, None]
        self.C[a] = (sa * self.C[a] + sb * self.C[b]) / (sa + sb)
        self.size[a] += self.size[b]
        self.size[b] = 0


class _DeviceState:
    """the cluster table in device memory: ra_ward_nearest and ra_ward_merge on the current stream, one read-back per round"""

    def __init__(self, X):
        self.L = L = Launcher(X)
        torch = L.torch
        self.n, self.d = (int(s) for s in X.shape)
        with torch.cuda.device(L.dev):
            self.C = X.double().contiguous()
            self.size = torch.ones(self.n, dtype=torch.int32, device=L.dev)
            self.out = torch.empty(12 * self.n, dtype=torch.uint8, device=L.dev)         # w2 [m] double, then nn [m] int

    def nearest(self, rows):
        torch, m = self.L.torch, len(rows)
        with torch.cuda.device(self.L.dev):
            rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(self.L.dev)
            w_d, nn_d = self.out[:8 * m], self.out[8 * m:12 * m]
            self.L.call("ra_ward_nearest", ptr(self.C), ptr(self.size), self.n, self.d, ptr(rows_d), m, ptr(nn_d), ptr(w_d))
            host = self.out[:12 * m].cpu().numpy()                                        # the round's one synchronisation
        return host[8 * m:].view(np.int32).astype(np.int64), host[:8 * m].view(np.float64).copy()

    def merge(self, a, b):
        torch = self.L.torch
        with torch.cuda.device(self.L.dev):
            ab = torch.from_numpy(np.ascontiguousarray(np.stack([a, b]), np.int32)).to(self.L.dev)
            self.L.call("ra_ward_merge", ptr(self.C), ptr(self.size), self.n, self.d, ptr(ab[0]), ptr(ab[1]), len(a))


# ---- rules 4 - 5

def _rounds(S, n):
    """rule 4 on a state S (nearest(rows) -> (nn, w); merge(a, b)): (a, b, w2, round, generation of a, generation of b) of the
    n - 1 merges in the order made, the number of rounds and of rows evaluated.  The generation of a slot counts the merges it
    has survived: (slot, generation) names one cluster."""
    nn, w = np.full(n, -1, np.int64), np.full(n, np.inf)
    live, gen, size = np.ones(n, bool), np.zeros(n, np.int64), np.ones(n, np.int64)
    stale = np.arange(n, dtype=np.int64)
    ma, mb, mw, mr, mga, mgb, ms = [], [], [], [], [], [], []
    done = rounds = evaluated = 0
    empty = False
    while done < n - 1:
        nn[stale], w[stale] = S.nearest(stale)
        evaluated += len(stale)
        b = nn[stale]
        has = b >= 0
        a, b = stale[has], b[has]
        rec = nn[b] == a
        lo = np.unique(np.minimum(a[rec], b[rec]))                          # every reciprocal pair once, by its lower slot
        if not len(lo):
            if empty:
                raise RuntimeError("ward: no reciprocal pair after a full re-evaluation in round %d, %d clusters left" % (rounds, n - done))
            empty = True
            stale = np.nonzero(live)[0]
            rounds += 1
            continue
        empty = False
        hi = nn[lo]
        S.merge(lo, hi)
        ma.append(lo); mb.append(hi); mw.append(w[lo].copy()); mr.append(np.full(len(lo), rounds, np.int64))
        mga.append(gen[lo].copy()); mgb.append(gen[hi].copy())
        gen[lo] += 1
        size[lo] += size[hi]
        ms.append(size[lo].copy())
        live[hi] = False
        consumed = np.zeros(n, bool)
        consumed[lo] = consumed[hi] = True
        nn[hi], w[hi] = -1, np.inf
        stale = np.nonzero(live & (consumed | ((nn >= 0) & consumed[np.maximum(nn, 0)])))[0]
        done += len(lo)
        rounds += 1
    return tuple(np.concatenate(v) for v in (ma, mb, mw, mr, mga, mgb, ms)), rounds, evaluated


def _tree(n, d, merges, rounds, evaluated, margin=None):
    """rule 5: sort, number the nodes, lay out scipy's Z"""
    a, b, w2, rnd, ga, gb, size = merges
    if len(a) != n - 1:
        raise RuntimeError("ward: %d merges for %d points" % (len(a), n))
    order = np.lexsort((a, rnd, w2))
    a, b, w2, rnd, ga, gb, size = (v[order] for v in (a, b, w2, rnd, ga, gb, size))
    # merge r creates the cluster (a_r, ga_r + 1) as node n + r; the cluster (slot, 0) is the point itself
    made = a * n + ga + 1
    by = np.argsort(made)

    def node(slot, g):
        r = by[np.minimum(np.searchsorted(made[by], slot * n + g), n - 2)]
        return np.where(g == 0, slot, n + r)

    ia, ib = node(a, ga), node(b, gb)
    if np.any(np.maximum(ia, ib) >= n + np.arange(n - 1)):
        raise RuntimeError("ward: a merge sorts before one of its children (heights that fall by rounding)")
    children = np.stack([np.minimum(ia, ib), np.maximum(ia, ib)], axis=1)
    return WardTree(n, d, np.stack([a, b], axis=1), w2, rnd, children, size, rounds, evaluated, margin)


def linkage(X, backend="device", details=False):
    """the Ward dendrogram of X [n][d] by the rules at the top of this module: a WardTree.  details (numpy backend only) adds
    margin and height_gap of rule 8."""
    X = _common.as_input(X, backend, WardError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d)
    if details and backend != "numpy":
        raise WardError("details are the numpy backend's")
    _common.check_finite(X, backend, WardError)
    S = _NumpyState(X, details) if backend == "numpy" else _DeviceState(X)
    merges, rounds, evaluated = _rounds(S, n)
    return _tree(n, d, merges, rounds, evaluated, S.margin if details else None)


def greedy_numpy(X):
    """the literal definition, for tests: at every step the globally least (W2, a, b) pair of live slots merges, O(n^3), n <= 200.
    Returns (merges int64 [n - 1][2], w2 [n - 1]) in the order made."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    if X.ndim != 2 or not 2 <= n <= MAX_GREEDY_N:
        raise WardError("greedy_numpy takes [n][d] with 2 <= n <= %d" % MAX_GREEDY_N)
    C, size = X.astype(np.float64), np.ones(n, np.float64)
    merges, w2 = np.empty((n - 1, 2), np.int64), np.empty(n - 1)
    for r in range(n - 1):
        live = np.nonzero(size > 0)[0]
        D = np.zeros((len(live), len(live)))
        for t in range(X.shape[1]):
            df = C[live, t, None] - C[None, live, t]
            D += df * df
        s = size[live]
        W = (s[:, None] * s[None, :]) / (s[:, None] + s[None, :]) * D
        W[np.tril_indices(len(live))] = np.inf                              # a < b only
        i, j = np.unravel_index(np.argmin(W), W.shape)                      # row-major first least: the least (a, b)
        a, b = live[i], live[j]
        merges[r], w2[r] = (a, b), W[i, j]
        C[a] = (size[a] * C[a] + size[b] * C[b]) / (size[a] + size[b])
        size[a] += size[b]
        size[b] = 0
    return merges, w2


# ---- rule 6

def n_clusters_at(tree, distance_threshold):
    """sklearn's rule: the merges with height >= t are undone"""
    return int(np.count_nonzero(tree.heights >= distance_threshold)) + 1


def cut(tree, n_clusters=None, distance_threshold=None):
    """int32 [n] labels of the tree cut at n_clusters = k (the last k - 1 merges undone) or at distance_threshold = t (exactly the
    merges with height < t applied), numbered by lowest member index.  One union-find pass over the applied merges: slot b of a
    merge points at slot a < b, and pointer doubling takes every point to its cluster's slot, the lowest member index."""
    check_cut(tree.n, n_clusters, distance_threshold)
    k = int(n_clusters) if n_clusters is not None else n_clusters_at(tree, distance_threshold)
    m = tree.n - k
    up = np.arange(tree.n, dtype=np.int64)
    up[tree.merges[:m, 1]] = tree.merges[:m, 0]
    root = _graph.jump(up)
    return np.searchsorted(np.unique(root), root).astype(np.int32)


def _centers(X, labels, k):
    """float64 [k][d] class centroids: the rows summed in index order within each class"""
    X = np.asarray(X.detach().cpu().numpy() if hasattr(X, "detach") else X, np.float64)
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=k)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.add.reduceat(X[order], starts, axis=0) / counts[:, None]


def ward(X, n_clusters=None, distance_threshold=None, backend="device"):
    """Ward clustering of X [n][d]: WardResult(labels, n_clusters, counts, centers, inertia, tree) of the tree of linkage() cut at
    n_clusters or at distance_threshold"""
    Xb = _common.as_input(X, backend, WardError, numpy_dtype=np.float32)
    check_domain(*(int(s) for s in Xb.shape))
    check_cut(int(Xb.shape[0]), n_clusters, distance_threshold)
    tree = linkage(Xb, backend)
    labels = cut(tree, n_clusters, distance_threshold)
    return WardResult(labels, _centers(Xb, labels, int(labels.max()) + 1), tree)


class SweepRow:
    """one k of a sweep: k, inertia, silhouette, calinski_harabasz, davies_bouldin, class_silhouette, counts, labels int32 [n] and
    the ValidityResult"""

    def __init__(self, k, inertia, labels, val):
        self.k, self.inertia, self.labels, self.validity = int(k), float(inertia), labels, val
        self.silhouette, self.calinski_harabasz, self.davies_bouldin = val.silhouette, val.calinski_harabasz, val.davies_bouldin
        self.class_silhouette, self.counts = val.class_silhouette, val.counts


def check_sweep(ks, n):
    from . import kmeans
    ks = [int(v) for v in ks]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 2:
        raise WardError("a sweep needs increasing k >= 2, got %r" % (ks,))
    if ks[-1] > min(n - 1, kmeans.MAX_K):
        raise WardError("the scores of a sweep need k <= min(n - 1, %d), got %d" % (kmeans.MAX_K, ks[-1]))
    return ks


def sweep(X, ks, sample_size=None, random_state=None, backend="device"):
    """one tree, then for every k of ks its cut, inertia(k) and kmeans.validity on the same device copy of X: a kmeans.SweepResult
    (rows, best_k: the largest silhouette, the smaller k on ties) with the tree as .tree"""
    from . import kmeans
    X = _common.as_input(X, backend, WardError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d)
    ks = check_sweep(ks, n)
    tree = linkage(X, backend)
    rows = []
    for k in ks:
        labels = cut(tree, k)
        rows.append(SweepRow(k, tree.inertia(k), labels, kmeans.validity(X, labels, k, sample_size, random_state, backend)))
    res = kmeans.SweepResult(rows)
    res.tree = tree
    return res


# ---- command line

def main(argv=None):
    from . import kmeans
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.ward")
    _common.add_cluster_arguments(ap, ("input", "output"), "factors", False)
    ap.add_argument("--k", type=int, default=None, help="number of clusters")
    ap.add_argument("--distance_threshold", type=float, default=None, help="apply exactly the merges below this height (sklearn's rule)")
    ap.add_argument("--sweep", default=None, help="K1,K2,... or LO:HI[:STEP]: one tree, its cut and the three scores for every k; the "
                    "labels written are those of --k if given, else of the largest silhouette")
    ap.add_argument("--scores", action="store_true", help="silhouette (overall, per class, per sample), Calinski-Harabasz and "
                    "Davies-Bouldin of the result in OUT.npz, and one line per class")
    ap.add_argument("--sample_size", type=int, default=None, help="evaluate the silhouette on sklearn's random subsample of this size")
    ap.add_argument("--seed", type=int, default=None, help="random_state of the subsample")
    _common.add_cluster_arguments(ap, ("--key", "--backend", "--truth", "--stack", "--params", "--ou", "--averages", "--device"), "factors", False)
    args = ap.parse_args(argv)
    ks = None
    if args.sweep is None and (args.k is None) == (args.distance_threshold is None):
        ap.error("exactly one of --k and --distance_threshold is needed (or --sweep)")
    if args.sweep is not None:
        if args.distance_threshold is not None:
            ap.error("--sweep goes with --k, not with --distance_threshold")
        try:
            ks = kmeans.parse_sweep(args.sweep)
        except ValueError as e:
            ap.error(str(e))
    if args.sample_size is not None and not (args.scores or ks):
        ap.error("--sample_size needs --scores or --sweep")
    if args.sample_size is not None and args.sample_size < 1:
        ap.error("--sample_size is an integer >= 1")
    if args.k is not None and args.k < 1:
        ap.error("--k must be at least 1")
    if args.distance_threshold is not None and not (np.isfinite(args.distance_threshold) and args.distance_threshold > 0):
        ap.error("--distance_threshold must be a finite number > 0")
    _common.check_averages_arguments(ap, args)
    try:
        X = kmeans.read_input(args.input, args.key)
        n, d = X.shape
        check_domain(n, d)
        if ks:
            ks = check_sweep(ks, n)
        if args.k is not None:
            check_cut(n, n_clusters=args.k)
        truth = kmeans.read_truth(args.truth, n) if args.truth else None
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device" or args.averages:
        _common.require_gpu(_common.NO_GPU)
    swept = val = None
    try:
        Xb = _common.to_device(X, args.device) if args.backend == "device" else X
        if ks:
            swept = sweep(Xb, ks, args.sample_size, args.seed, args.backend)
            tree = swept.tree
            if args.k is None:
                args.k = swept.best_k
            if args.k in ks:
                val = swept.row(args.k).validity
        else:
            tree = linkage(Xb, args.backend)
        labels = cut(tree, args.k, None if args.k is not None else args.distance_threshold)
        k = int(labels.max()) + 1
        if args.scores and val is None:
            val = kmeans.validity(Xb, labels, k, args.sample_size, args.seed, args.backend)
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    out = dict(labels=labels, linkage=tree.Z, n_clusters=np.int64(k), counts=counts, inertia=np.float64(tree.inertia(k)),
               n_rounds=np.int64(tree.n_rounds), rows_evaluated=np.int64(tree.rows_evaluated), k=np.int64(args.k if args.k is not None else -1),
               distance_threshold=np.float64(args.distance_threshold if args.distance_threshold is not None else np.nan),
               key=np.str_(args.key), backend=np.str_(args.backend), seed=np.int64(-1 if args.seed is None else args.seed))
    msg = "%s: %d points x %d, %d clusters, inertia %.6g, %d rounds, %.2f n rows evaluated" % (
        args.output, n, d, k, tree.inertia(k), tree.n_rounds, tree.rows_evaluated / n)
    if truth is not None:
        msg += _common.truth_scores(out, truth, labels)
    if args.averages:
        msg += _common.write_averages(args, n, labels, k, None, WardError, MAX_AVERAGES)
    if swept is not None:
        out["sweep"], out["best_k"] = swept.table(), np.int64(swept.best_k)
        print("%5s %14s %11s %14s %11s" % ("k", "inertia", "silhouette", "CH", "DB"))
        for r in swept.rows:
            print("%5d %14.6g %11.6f %14.6g %11.6f%s" % (r.k, r.inertia, r.silhouette, r.calinski_harabasz, r.davies_bouldin,
                                                          "  <- best" if r.k == swept.best_k else ""))
    if args.scores:
        out["silhouette"], out["class_silhouette"], out["silhouette_samples"] = np.float64(val.silhouette), val.class_silhouette, val.samples
        out["calinski_harabasz"], out["davies_bouldin"] = np.float64(val.calinski_harabasz), np.float64(val.davies_bouldin)
        for c in range(k):
            print("class %3d: %7d members, silhouette %8.4f" % (c, val.counts[c], val.class_silhouette[c]))
        msg += ", silhouette %.4f, CH %.6g, DB %.4f" % (val.silhouette, val.calinski_harabasz, val.davies_bouldin)
    np.savez(args.output, **out)
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
