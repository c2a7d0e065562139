"""HDBSCAN of embeddings or factors X [n][d] on the GPU (after scikit-learn 1.7 HDBSCAN(min_cluster_size, min_samples,
cluster_selection_method, metric="euclidean", allow_single_cluster=False), with equal weights merged at once).

    python -m cryo_ralib_amd.hdbscan IN OUT.npz [--min_cluster_size 5] [--min_samples S] [--method eom|leaf] [--key embedding]
                                     [--backend device|numpy] [--truth FILE] [--min_proba P]
                                     [--stack STACK --params PARAMS --ou R --averages REFS.{hdf,mrcs,npy}]

IN is the OUT.npz of the tsne tool (--key embedding, the default) or of the sdr tool (--key factors), or an [n][d] .npy.  OUT.npz
holds labels, probabilities, tie_mask, n_clusters, n_noise, core_distances, the tree edges (mst_lo, mst_hi, mst_distance), the
condensed rows (condensed_parent, condensed_child, condensed_lambda, condensed_size), stabilities, n_rounds and the options used;
the tool prints one line per cluster (size, stability, median probability) and the noise count.  --min_proba P adds
keep = probabilities >= P (noise has probability 0).  --truth takes an int .npy or a params.txt (its class column) and adds
purity, c_purity and contingency over the non-noise points.  --averages writes the class averages of the non-noise particles of
the stack (kmeans.class_averages with k = n_clusters): a refstack for the multi-reference command line; more than 256 clusters is
an error there.

scikit-learn's labels are not a function of the data: a cluster splits at the weight w of one bridging edge (a, b), w is usually
a's core distance, so a's other edges weigh exactly w too, and in sklearn's binary dendrogram a lands on one side or the other by
the order an unstable argsort gives equal weights.  The rules below merge equal weights at once (Campello et al.'s definition):
a pure function of the data, invariant under row permutation, and different from sklearn only on the tie set of rule 9.

The contract, rule by rule:
  1. Input is X [n][d] float32, which converts to double exactly; min_cluster_size = 5 and min_samples = None are integers, None
     meaning min_cluster_size; cluster_selection_method is "eom" (the default) or "leaf".
  2. D2(i, j) is dbscan.py's rule 2: sum_t (x_it - x_jt)^2 in double from differences, the features in order, one chain per pair;
     exactly symmetric and 0 on the diagonal.  One device function chain (dbs_tile, and hdb_d2 for single pairs) forms every D2.
  3. core2_i is D2 to the (min_samples - 1)-th nearest other point, 0 for min_samples = 1 (sklearn counts the point itself among
     its min_samples neighbours): dbscan.kdistances squared.
  4. w2(i, j) = max(core2_i, core2_j, D2(i, j)).  All comparisons are on squared values; sqrt is taken once, on the n - 1 tree
     edges.
  5. Edges are totally ordered by (w2, min(i, j), max(i, j)); the MST is the unique minimum spanning tree under that order
     (Kruskal over it), so the edge list is a pure function of the data, whatever the Boruvka schedule.
  6. Level hierarchy: walk the distinct values of w2 upwards and unite all tree edges of one value at once; every component that
     results is one node whose children are the components it absorbed.  A node may have more than two children.
  7. Condensed tree, from the root down, with lambda = 1 / w and lambda = inf for w = 0.  When a cluster c reaches a node of
     height w, children smaller than min_cluster_size leave c: each of their points gets a row (c, point, lambda, 1).  If exactly
     one child has at least min_cluster_size points it continues as c; if two or more do, c ends and each is a new cluster born
     at lambda, with a row (c, child, lambda, size); if none does, c ends.  A node of height 0 has only single points as
     children, so no cluster is born at inf.
  8. Selection and labels follow sklearn's _tree.pyx.  stability_c = sum over the rows with parent c of (lambda_row - birth_c)
     size_row, birth_root = 0.  "eom": from the leaves up, never selecting the root (allow_single_cluster=False); if the
     children's stabilities sum to MORE than c's own, c is unselected and carries the sum, otherwise c is selected and all its
     descendants are unselected (a tie keeps the parent, as sklearn's strict > does).  "leaf": the leaves of the cluster tree;
     without any split nothing is selected.  A point's label is the selected cluster at or above the cluster it left, -1 if that
     is the root or no selected cluster lies above.  probability = min(lambda_point, L) / L with L the largest lambda among the
     rows whose parent is the selected cluster; 1 when L = 0 or lambda_point = inf, 0 for noise.  Clusters are numbered
     0 .. c - 1 by their lowest member index.
  9. The tie set T holds the points with a row (c, point, lambda) whose lambda equals the lambda at which c ends in a true split;
     it is returned as tie_mask.  sklearn may give these points to either child.  Outside T labels agree with sklearn up to a
     renaming of cluster ids, unless a piece below min_cluster_size plus a tie point reaches min_cluster_size in sklearn's binary
     tree (seen with min_cluster_size 8 on 2000 points; the pins exclude such cases by construction).
 10. The result is a pure function of (X, min_cluster_size, min_samples, method), bitwise reproducible call to call and stream to
     stream; permuting the rows permutes labels, probabilities and tie_mask (cluster ids renamed).  Sums of floating-point
     values on the host (stabilities) run over values sorted first, so they do not depend on the row order either.
Domain: 2 <= n <= 262144, 1 <= d <= 2048, 2 <= min_cluster_size <= n, 1 <= min_samples <= min(n, 302) (ra_tsne_knn's cap of 301
neighbours), finite X.  Anything else raises HdbscanError (a ValueError) before anything is launched.
Not built: allow_single_cluster=True, cluster_selection_epsilon, max_cluster_size, alpha != 1, other metrics, store_centers,
sparse or precomputed input, multi-GPU, GLOSH outlier scores.

On the device ra_hdbscan_core writes core2 and every Boruvka round is one ra_hdbscan_round (csrc/ralign_hdbscan.h): an all-pairs
pass in 64 x 64 tiles that keeps the least (w2, lo, hi) per row over the columns of other components, and the minimum per
component by integer atomicMin.  Nothing of size n^2 is stored.  The host reads the entries at the component roots, drops the
edge two components chose both, unites the components (label = lowest index) and writes comp back.  Every round at least halves
the number of components, so the loop is capped at ceil(log2 n) + 1 rounds and raises past the cap.  backend="numpy" is the
float64 checker: core2 from row chunks of the unfused D2 (no [n][n] array) and Prim's algorithm under rule 5's order, one D2 row
per step; it needs no GPU.  Rules 6 - 9 are one numpy implementation for both backends (tree_from_mst): the binary dendrogram by
one union-find pass over the sorted edges, everything after it by pointer jumping over arrays, O(n log n).
"""
import argparse
import math
import sys
import time

import numpy as np

from . import _common, _graph
from ._common import Launcher, d2_rows, is_int, ptr, row_chunks

MAX_N, MAX_D, MAX_MIN_SAMPLES = 262144, 2048, 302
MAX_AVERAGES = 256          # kmeans.class_averages' limit on the number of classes
METHODS = ("eom", "leaf")


class HdbscanError(ValueError):
    """an input outside the supported domain"""


class HdbscanResult:
    """labels int32 [n] (-1 for noise), probabilities float64 [n], tie_mask bool [n] (rule 9), n_clusters, core_distances float64 [n],
    mst = (lo int32, hi int32, distance float64), n - 1 edges in rule 5's order, condensed = (parent int64, child int64, lambda
    float64, size int64) with the root cluster numbered n, stabilities float64 [n_clusters] of the selected clusters in label order,
    n_rounds (Boruvka rounds; 0 for the numpy backend) and tree_seconds (host time of rules 6 - 9)"""

    def __init__(self, labels, probabilities, tie_mask, core_distances, mst, condensed, stabilities, n_rounds, tree_seconds):
        self.labels, self.probabilities, self.tie_mask, self.core_distances = labels, probabilities, tie_mask, core_distances
        self.mst, self.condensed, self.stabilities = mst, condensed, stabilities
        self.n_rounds, self.tree_seconds = int(n_rounds), float(tree_seconds)
        self.n_clusters = int(labels.max()) + 1 if labels.size and labels.max() >= 0 else 0

    @property
    def n_noise(self):
        return int(np.count_nonzero(self.labels < 0))


def check_domain(n, d, min_cluster_size=5, min_samples=None, method="eom", device=True):
    """raise HdbscanError unless the shape and parameters are inside the supported domain; returns min_samples with None resolved"""
    def need(ok, msg):
        if not ok:
            raise HdbscanError(msg)
    need(is_int(min_cluster_size), "min_cluster_size must be an integer, got %r" % (min_cluster_size,))
    need(min_samples is None or is_int(min_samples), "min_samples must be an integer or None, got %r" % (min_samples,))
    need(method in METHODS, "cluster_selection_method is 'eom' or 'leaf', got %r" % (method,))
    need(2 <= n <= MAX_N, "need 2 <= n <= %d points, got %d" % (MAX_N, n))
    need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    need(2 <= min_cluster_size <= n, "need 2 <= min_cluster_size <= n = %d, got %d" % (n, min_cluster_size))
    ms = int(min_cluster_size if min_samples is None else min_samples)
    need(1 <= ms <= min(n, MAX_MIN_SAMPLES), "need 1 <= min_samples <= min(n, %d) = %d, got %d" % (MAX_MIN_SAMPLES, min(n, MAX_MIN_SAMPLES), ms))
    return ms


def _sort_edges(lo, hi, w2):
    order = np.lexsort((hi, lo, w2))
    return lo[order].astype(np.int32), hi[order].astype(np.int32), w2[order]


# ---- CPU checker (float64 numpy): rules 2 - 5

def core2_numpy(X, min_samples):
    """core2 [n] of rule 3 from row chunks of the unfused D2"""
    X = np.asarray(X, np.float64)
    n, k = X.shape[0], int(min_samples) - 1
    if k == 0:
        return np.zeros(n)
    out = np.empty(n)
    for s0, s1 in row_chunks(n):
        out[s0:s1] = np.partition(d2_rows(X, s0, s1), k, axis=1)[:, k]             # the point itself is the 0-th
    return out


def mst_numpy(X, core2):
    """(lo, hi, w2) of rule 5 by Prim's algorithm from point 0: every comparison is on the triple (w2, lo, hi), a strict total order
    of the edges, under which the minimum spanning tree is unique, so the choice of algorithm and of the start cannot matter"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    idx = np.arange(n, dtype=np.int64)
    intree = np.zeros(n, bool)
    bw, blo, bhi = np.full(n, np.inf), np.full(n, n, np.int64), np.full(n, n, np.int64)
    lo, hi, w2 = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1)
    u = 0
    for e in range(n - 1):
        intree[u] = True
        w = np.maximum(np.maximum(d2_rows(X, u, u + 1)[0], core2[u]), core2)
        elo, ehi = np.minimum(idx, u), np.maximum(idx, u)
        less = (w < bw) | ((w == bw) & ((elo < blo) | ((elo == blo) & (ehi < bhi))))
        less &= ~intree
        bw[less], blo[less], bhi[less] = w[less], elo[less], ehi[less]
        bw[u] = np.inf
        cand = np.nonzero(bw == bw.min())[0]
        cand = cand[~intree[cand]]
        v = cand[np.lexsort((bhi[cand], blo[cand]))[0]]
        lo[e], hi[e], w2[e] = blo[v], bhi[v], bw[v]
        u = int(v)
    return _sort_edges(lo, hi, w2)


# ---- device: rules 2 - 5

def _unite(m, a, b):
    """label [m] = the lowest index of the connected component of 0 .. m - 1 under the edges (a, b): minimum, hook, compress"""
    lab = np.arange(m, dtype=np.int64)
    while True:
        mn = lab.copy()
        np.minimum.at(mn, a, lab[b])
        np.minimum.at(mn, b, lab[a])
        P = lab.copy()
        sel = mn < lab
        np.minimum.at(P, lab[sel], mn[sel])
        P = np.minimum(P, mn)
        while True:
            Q = P[P]
            if np.array_equal(Q, P):
                break
            P = Q
        if np.array_equal(P, lab):
            return lab
        lab = P


def boruvka_merge(comp, w2, lo, hi):
    """one round on the host: comp int [n] (lowest index of each component) and the round's outputs at the roots -> (new comp, lo,
    hi, w2 of the new tree edges, each once).  A component that holds every point has no edge (+inf, -1, -1)."""
    n = len(comp)
    roots = np.nonzero(comp == np.arange(n))[0]
    rw, rlo, rhi = w2[roots], lo[roots].astype(np.int64), hi[roots].astype(np.int64)
    ok = np.isfinite(rw)
    if not ok.all():
        if len(roots) == 1:
            return comp, rlo[:0], rhi[:0], rw[:0]
        raise RuntimeError("hdbscan: a component without an outgoing edge while %d components remain" % len(roots))
    if not (np.all(rlo >= 0) and np.all(rlo < rhi) and np.all(rhi < n)):
        raise RuntimeError("hdbscan: a round returned an edge outside 0 <= lo < hi < n")
    key, first = np.unique(rlo * n + rhi, return_index=True)            # two components may choose the same edge
    elo, ehi, ew = rlo[first], rhi[first], rw[first]
    ca, cb = np.searchsorted(roots, comp[elo]), np.searchsorted(roots, comp[ehi])
    lab = _unite(len(roots), ca, cb)
    return roots[lab][np.searchsorted(roots, comp)], elo, ehi, ew


def _mst_device(X, min_samples):
    L = Launcher(X)
    torch, dev = L.torch, L.dev
    n, d = (int(s) for s in X.shape)
    cap = max(1, math.ceil(math.log2(n))) + 1
    with torch.cuda.device(dev):
        core2 = torch.empty(n, dtype=torch.float64, device=dev)
        comp_d = torch.arange(n, dtype=torch.int32, device=dev)
        out_w = torch.empty(n, dtype=torch.float64, device=dev)
        out_lo = torch.empty(n, dtype=torch.int32, device=dev)
        out_hi = torch.empty(n, dtype=torch.int32, device=dev)
        L.call("ra_hdbscan_core", ptr(X), n, d, int(min_samples), ptr(core2))
        comp = np.arange(n, dtype=np.int64)
        lo, hi, w2, rounds, left = [], [], [], 0, n
        while left > 1:
            if rounds >= cap:
                raise RuntimeError("hdbscan: %d components left after %d rounds for %d points: every round at least halves them" % (
                    left, rounds, n))
            L.call("ra_hdbscan_round", ptr(X), n, d, ptr(core2), ptr(comp_d), ptr(out_w), ptr(out_lo), ptr(out_hi))
            rounds += 1
            comp, elo, ehi, ew = boruvka_merge(comp, out_w.cpu().numpy(), out_lo.cpu().numpy(), out_hi.cpu().numpy())
            lo.append(elo)
            hi.append(ehi)
            w2.append(ew)
            now = int(np.count_nonzero(comp == np.arange(n)))
            if 2 * now > left:
                raise RuntimeError("hdbscan: round %d left %d of %d components" % (rounds, now, left))
            left = now
            comp_d.copy_(torch.from_numpy(comp.astype(np.int32)))
        lo, hi, w2 = np.concatenate(lo), np.concatenate(hi), np.concatenate(w2)
        if len(lo) != n - 1:
            raise RuntimeError("hdbscan: %d tree edges for %d points" % (len(lo), n))
        return core2.cpu().numpy(), _sort_edges(lo, hi, w2), rounds


# ---- rules 6 - 9, shared by both backends

def _dendrogram(n, lo, hi):
    """the binary single-linkage dendrogram of the sorted tree edges: node n + e joins the two nodes that hold lo[e] and hi[e].
    Returns parent [2 n - 1] (the root its own parent) and size [2 n - 1].  The one pass that is a Python loop: a union-find
    over the points (union by size, path halving), with the dendrogram node of every component kept at its root."""
    uf, node, count = list(range(n)), list(range(n)), [1] * n
    parent, size = list(range(2 * n - 1)), [1] * n
    nxt = n
    for a, b in zip(lo.tolist(), hi.tolist()):
        while uf[a] != a:
            uf[a] = a = uf[uf[a]]
        while uf[b] != b:
            uf[b] = b = uf[uf[b]]
        if a == b:
            raise ValueError("the edges do not form a tree")
        parent[node[a]] = parent[node[b]] = nxt
        both = count[a] + count[b]
        if count[a] < count[b]:
            a, b = b, a
        uf[b] = a
        count[a] = both
        node[a] = nxt
        size.append(both)
        nxt += 1
    return np.array(parent, np.int64), np.array(size, np.int64)


def tree_from_mst(n, lo, hi, w2, min_cluster_size, method="eom"):
    """rules 6 - 9 from the n - 1 tree edges in rule 5's order: (labels, probabilities, tie_mask, condensed rows, stabilities)"""
    mcs = int(min_cluster_size)
    lo, hi, w2 = np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(w2, np.float64)
    if len(lo) != n - 1 or np.any(np.diff(w2) < 0):
        raise ValueError("tree_from_mst takes the n - 1 edges sorted by weight")
    N = 2 * n - 1
    parent, size = _dendrogram(n, lo, hi)
    height = np.concatenate([np.zeros(n), w2])                      # w2 of the edge that made the node; unused for points
    root = N - 1
    # rule 6: a node whose parent has the same height is part of its parent's level node; rep = the top of that chain
    ident = np.arange(N, dtype=np.int64)
    same = (ident >= n) & (parent != ident) & (height[parent] == height) & (parent >= n)
    rep = _graph.jump(np.where(same, parent, ident))
    is_level = rep == ident                                         # points, and the top binary node of every level node
    lp = rep[parent]                                                # level parent of a level node (the root: itself)
    big = is_level & (size >= mcs)
    # rule 7: the number of children of at least min_cluster_size of every level node
    kids = np.nonzero(is_level & (ident != root))[0]
    nbig = np.bincount(lp[kids], weights=big[kids].astype(np.float64), minlength=N).astype(np.int64)
    # a big level node heads a cluster if it is the root or one of two or more big children; otherwise it continues its parent's
    heads = big & ((ident == root) | (nbig[lp] >= 2))
    head = _graph.jump(np.where(big & ~heads, lp, ident))          # for a big level node: the node that heads its cluster
    head_nodes = np.nonzero(heads)[0][::-1]                         # the root first; a parent cluster before its children
    ncl = len(head_nodes)
    cid = np.full(N, -1, np.int64)
    cid[head_nodes] = np.arange(ncl)
    with np.errstate(divide="ignore"):
        lam_node = 1.0 / np.sqrt(height)                            # lambda of a level node; inf for height 0
    # cluster rows: every head but the root is born at its level parent's lambda, in the cluster that reached that parent
    ch = head_nodes[1:]
    c_parent, c_lambda, c_size = cid[head[lp[ch]]], lam_node[lp[ch]], size[ch]
    birth = np.zeros(ncl)
    birth[1:] = c_lambda
    cl_parent = np.full(ncl, -1, np.int64)
    cl_parent[1:] = c_parent
    # point rows: a point leaves with the topmost level ancestor-or-self below min_cluster_size, at that node's level parent
    top = _graph.jump(np.where(is_level & ~big[lp] & (ident != root), lp, ident))
    pts = np.arange(n, dtype=np.int64)
    leave = lp[top[pts]]
    p_parent, p_lambda = cid[head[leave]], lam_node[leave]
    # rule 9: the lambda at which a cluster ends in a true split
    split_lambda = np.full(ncl, np.nan)
    split_lambda[c_parent] = c_lambda
    tie_mask = p_lambda == split_lambda[p_parent]
    # rule 8: stabilities, each a sum over values sorted first
    rp = np.concatenate([p_parent, c_parent])
    rl = np.concatenate([p_lambda, c_lambda])
    rs = np.concatenate([np.ones(n, np.int64), c_size])
    order = np.lexsort((rs, rl, rp))
    stab = np.bincount(rp[order], weights=(rl[order] - birth[rp[order]]) * rs[order], minlength=ncl)
    maxlam = np.zeros(ncl)
    np.maximum.at(maxlam, rp, rl)
    has_child = np.zeros(ncl, bool)
    has_child[c_parent] = True
    selected = np.zeros(ncl, bool)
    if method == "leaf":
        selected = ~has_child
        selected[0] = False
    else:
        carried = [[] for _ in range(ncl)]
        for c in range(ncl - 1, 0, -1):
            below = float(np.sum(np.sort(np.array(carried[c])))) if carried[c] else 0.0
            if below > stab[c]:
                carry = below
            else:
                selected[c] = True
                carry = stab[c]
            carried[cl_parent[c]].append(carry)
        covered = np.zeros(ncl, bool)
        for c in range(1, ncl):
            q = cl_parent[c]
            covered[c] = covered[q] or selected[q]
        selected &= ~covered
    # the selected cluster at or above every cluster (-1: none)
    above = np.where(selected, np.arange(ncl), -1)
    for c in range(1, ncl):
        if above[c] < 0:
            above[c] = above[cl_parent[c]]
    psel = above[p_parent]
    labels = np.full(n, -1, np.int32)
    prob = np.zeros(n)
    member = psel >= 0
    if member.any():
        ids, first = np.unique(psel[member], return_index=True)    # first: the lowest member index of each selected cluster
        rank = np.empty(len(ids), np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(len(ids))
        labels[member] = rank[np.searchsorted(ids, psel[member])].astype(np.int32)
        L = maxlam[psel[member]]
        lam = p_lambda[member]
        with np.errstate(invalid="ignore", divide="ignore"):
            pr = np.minimum(lam, L) / L
        prob[member] = np.where((L == 0.0) | np.isinf(lam), 1.0, pr)
        stabilities = stab[ids[np.argsort(first, kind="stable")]]
    else:
        stabilities = np.zeros(0)
    condensed = (np.concatenate([p_parent, c_parent]) + n, np.concatenate([pts, cid[ch] + n]), rl, rs)
    return labels, prob, tie_mask, condensed, stabilities


# ---- the public call

def hdbscan(X, min_cluster_size=5, min_samples=None, cluster_selection_method="eom", backend="device"):
    """HDBSCAN of X [n][d] by the rules at the top of this module: HdbscanResult(labels int32 [n] with -1 for noise, probabilities,
    tie_mask, n_clusters, core_distances, mst, condensed, stabilities, n_rounds).  Euclidean metric, allow_single_cluster=False,
    no cluster_selection_epsilon, max_cluster_size, alpha, store_centers or outlier scores, no precomputed or sparse input, one
    GPU, at most 262144 points."""
    X = _common.as_input(X, backend, HdbscanError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    ms = check_domain(n, d, min_cluster_size, min_samples, cluster_selection_method)
    _common.check_finite(X, backend, HdbscanError)
    if backend == "numpy":
        core2 = core2_numpy(X, ms)
        (lo, hi, w2), rounds = mst_numpy(X, core2), 0
    else:
        core2, (lo, hi, w2), rounds = _mst_device(X, ms)
    t0 = time.perf_counter()
    labels, prob, tie_mask, condensed, stabilities = tree_from_mst(n, lo, hi, w2, int(min_cluster_size), cluster_selection_method)
    return HdbscanResult(labels, prob, tie_mask, np.sqrt(core2), (lo, hi, np.sqrt(w2)), condensed, stabilities, rounds,
                         time.perf_counter() - t0)


# ---- command line

def main(argv=None):
    from . import kmeans
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.hdbscan")
    _common.add_cluster_arguments(ap, ("input", "output"), "embedding", True)
    ap.add_argument("--min_cluster_size", type=int, default=5, help="the least number of points of a cluster")
    ap.add_argument("--min_samples", type=int, default=None, help="neighbours, itself included, of the core distance (default min_cluster_size)")
    ap.add_argument("--method", default="eom", choices=METHODS, help="cluster selection: excess of mass, or the leaves")
    _common.add_cluster_arguments(ap, ("--key", "--backend", "--truth"), "embedding", True)
    ap.add_argument("--min_proba", type=float, default=None, help="P in (0, 1]: store keep = probabilities >= P")
    _common.add_cluster_arguments(ap, ("--stack", "--params", "--ou", "--averages", "--device"), "embedding", True)
    args = ap.parse_args(argv)
    if args.min_proba is not None and not (0.0 < args.min_proba <= 1.0):
        ap.error("--min_proba must lie in (0, 1]")
    _common.check_averages_arguments(ap, args)
    if args.min_cluster_size < 2:
        ap.error("--min_cluster_size must be at least 2")
    if args.min_samples is not None and not 1 <= args.min_samples <= MAX_MIN_SAMPLES:
        ap.error("--min_samples must lie in 1 .. %d" % MAX_MIN_SAMPLES)
    try:
        X = kmeans.read_input(args.input, args.key)
        n, d = X.shape
        check_domain(n, d, args.min_cluster_size, args.min_samples, args.method)
    except HdbscanError as e:
        ap.error(str(e))
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    try:
        truth = kmeans.read_truth(args.truth, n) if args.truth else None
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device" or args.averages:
        _common.require_gpu(_common.NO_GPU)
    Xb = _common.to_device(X, args.device) if args.backend == "device" else X
    try:
        res = hdbscan(Xb, args.min_cluster_size, args.min_samples, args.method, backend=args.backend)
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    ms = args.min_cluster_size if args.min_samples is None else args.min_samples
    out = dict(min_cluster_size=np.int64(args.min_cluster_size), min_samples=np.int64(ms), method=np.str_(args.method),
               key=np.str_(args.key), backend=np.str_(args.backend), labels=res.labels, probabilities=res.probabilities,
               tie_mask=res.tie_mask, n_clusters=np.int64(res.n_clusters), n_noise=np.int64(res.n_noise),
               core_distances=res.core_distances, mst_lo=res.mst[0], mst_hi=res.mst[1], mst_distance=res.mst[2],
               condensed_parent=res.condensed[0], condensed_child=res.condensed[1], condensed_lambda=res.condensed[2],
               condensed_size=res.condensed[3], stabilities=res.stabilities, n_rounds=np.int64(res.n_rounds))
    size = np.bincount(res.labels[res.labels >= 0], minlength=res.n_clusters)
    for c in range(res.n_clusters):
        print("cluster %4d: %7d members, stability %.6g, median probability %.4f" % (
            c, size[c], res.stabilities[c], float(np.median(res.probabilities[res.labels == c]))))
    print("noise: %d points" % res.n_noise)
    msg = "%s: %d points x %d, min_cluster_size = %d, min_samples = %d, %s: %d clusters, %d noise, %d tie points, %d rounds" % (
        args.output, n, d, args.min_cluster_size, ms, args.method, res.n_clusters, res.n_noise, int(res.tie_mask.sum()), res.n_rounds)
    keep = res.labels >= 0
    if args.min_proba is not None:
        out["min_proba"] = np.float64(args.min_proba)
        out["keep"] = res.probabilities >= args.min_proba
        msg += ", %d kept at probability >= %g" % (int(out["keep"].sum()), args.min_proba)
    if truth is not None:
        msg += _common.truth_scores(out, truth, res.labels, keep)
    if args.averages:
        msg += _common.write_averages(args, n, res.labels, res.n_clusters, keep, HdbscanError, MAX_AVERAGES)
    np.savez(args.output, **out)
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
