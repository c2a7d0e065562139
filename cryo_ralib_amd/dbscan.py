"""DBSCAN of embeddings or factors X [n][d] on the GPU (scikit-learn 1.7 DBSCAN(eps, min_samples, metric="euclidean")).

    python -m cryo_ralib_amd.dbscan IN OUT.npz --eps E [--min_samples 5] [--key embedding] [--backend device|numpy] [--kdist]
                                    [--truth FILE] [--stack STACK --params PARAMS --ou R --averages REFS.{hdf,mrcs,npy}]

IN is the OUT.npz of the tsne tool (--key embedding, the default) or of the sdr tool (--key factors), or an [n][d] .npy.  OUT.npz
holds labels, core_mask, counts, n_clusters, n_noise, n_rounds and the options used; the tool prints one line per cluster (size,
core points) and the noise count.  --kdist works without --eps: it stores the sorted kdistances as kdist and prints their
50/75/90/95/99 % quantiles (the sorted curve is the standard way to pick eps).  --truth takes an int .npy or a params.txt (its class
column) and adds purity, c_purity and contingency over the non-noise points.  --averages writes the class averages of the non-noise
particles of the stack (kmeans.class_averages with k = n_clusters): a refstack for the multi-reference command line; more than 256
clusters is an error there.

The contract, rule by rule:
  1. Input is X [n][d] float32, eps a double and min_samples an integer.  X converts to double exactly.
  2. D2(i, j) = sum_t (x_it - x_jt)^2 is formed in double from differences with the features in order, never as a Gram expansion.
     D2(i, i) = 0 exactly and D2(i, j) = D2(j, i) bit for bit.
  3. j is a neighbour of i iff D2(i, j) <= eps * eps (the double product): the test is inclusive and i is its own neighbour.  The
     device fuses each multiply-add, the numpy checker does not: where every term is exactly representable the decisions are
     equal; elsewhere they may differ only for pairs with |D2 - eps^2| <= d 2^-50 eps^2.  There is no float32 screen.
  4. count_i is the number of neighbours, itself included; i is a core point iff count_i >= min_samples.
  5. Clusters are the connected components of the core points under the neighbour relation, numbered 0 .. c - 1 by their lowest
     core index (sklearn scans i upwards and opens a cluster at the first unlabelled core point).
  6. A non-core point with at least one core neighbour is a border point; its label is the least cluster id among its core
     neighbours (sklearn expands cluster 0 completely before cluster 1, and a point keeps the first label it gets).
  7. A non-core point without a core neighbour is noise, -1.
  8. The result is a pure function of (X, eps, min_samples), bitwise reproducible call to call and stream to stream.
Domain: 1 <= n <= 262144, 1 <= d <= 2048, finite eps > 0, integer min_samples >= 1, finite X.  Anything else raises DbscanError
(a ValueError) before anything is launched.
Not built: other metrics, sample_weight, precomputed or sparse input, OPTICS, multi-GPU, more than 262144 points (HDBSCAN is
hdbscan.py).

On the device every pass recomputes its n^2 distances in the HIP kernels behind ra_dbscan_count / ra_dbscan_step
(csrc/ralign_dbscan.h); nothing of size n^2 is stored.  The host reads one int per round (the number of core points whose label
moved) and stops at 0; the loop is capped at n_core + 1 rounds, which cannot be reached because every unfinished round lowers a
label.  The roots (lowest core index of a component) are then mapped to 0 .. c - 1 by unique.  backend="numpy" is the float64
checker: it runs chunked over rows, keeps the neighbour pairs that involve a core point as index lists (no [n][n] array), needs
no GPU and follows the rules above literally.

kdistances(X, min_samples) is, for each point, the least eps at which it is a core point: the distance to its
(min_samples - 1)-th nearest other point, 0 for min_samples = 1 and inf for min_samples > n.  The device reads the last column of
ra_tsne_knn, whose domain it has: n >= 2 and min_samples - 1 <= 301 (the numpy backend has no such cap).  core_mask ==
(kdistances <= eps) ties the two kernels together.
"""
import argparse
import math
import sys

import numpy as np

from . import _common, _graph
from ._common import Launcher, d2_rows, is_int, is_real, ptr, row_chunks

MAX_N, MAX_D, MAX_KNN = 262144, 2048, 301
MAX_AVERAGES = 256          # kmeans.class_averages' limit on the number of classes


class DbscanError(ValueError):
    """an input outside the supported domain"""


class DbscanResult:
    """labels int32 [n] (-1 for noise), core_mask bool [n], core_sample_indices int64 (sklearn's core_sample_indices_), n_clusters,
    counts int32 [n] (neighbours within eps, the point itself included) and n_rounds (merging rounds run)"""

    def __init__(self, labels, core_mask, counts, n_rounds):
        self.labels, self.core_mask, self.counts, self.n_rounds = labels, core_mask, counts, int(n_rounds)
        self.core_sample_indices = np.nonzero(core_mask)[0].astype(np.int64)
        self.n_clusters = int(labels.max()) + 1 if labels.size and labels.max() >= 0 else 0

    @property
    def n_noise(self):
        return int(np.count_nonzero(self.labels < 0))


def check_domain(n, d, eps, min_samples):
    """raise DbscanError unless the shape and parameters are inside the supported domain"""
    def need(ok, msg):
        if not ok:
            raise DbscanError(msg)
    need(is_int(min_samples), "min_samples must be an integer, got %r" % (min_samples,))
    need(1 <= n <= MAX_N, "need 1 <= n <= %d points, got %d" % (MAX_N, n))
    need(1 <= d <= MAX_D, "need 1 <= d <= %d features, got %d" % (MAX_D, d))
    need(is_real(eps) and eps > 0, "need a finite eps > 0, got %r" % (eps,))
    need(min_samples >= 1, "need min_samples >= 1, got %d" % min_samples)


# ---- CPU checker (float64 numpy)

def _components(n, ea, eb):
    """label [n] = the lowest index of the connected component under the edges (ea, eb): minimum, hook, compress, as the device.
    Apart from spectral.components_numpy: this one takes an edge list, hooks every point as well as its label, and counts rounds."""
    lab = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        m = lab.copy()
        np.minimum.at(m, ea, lab[eb])
        np.minimum.at(m, eb, lab[ea])
        P = lab.copy()
        sel = m < lab
        np.minimum.at(P, lab[sel], m[sel])
        P = _graph.jump(np.minimum(P, m))
        if np.array_equal(P, lab):
            return lab, rounds
        lab = P


def _dbscan_numpy(X, eps, min_samples):
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    eps2 = float(eps) * float(eps)
    chunks = row_chunks(n)
    counts = np.empty(n, np.int64)
    for s0, s1 in chunks:
        counts[s0:s1] = np.count_nonzero(d2_rows(X, s0, s1) <= eps2, axis=1)
    core = counts >= min_samples
    ea, eb = [], []                     # pairs (i, j) with j core: i < j for a core i, every j for a non-core i
    for s0, s1 in chunks:
        N = d2_rows(X, s0, s1) <= eps2
        N &= core[None, :]
        i, j = np.nonzero(N)
        i += s0
        keep = ~core[i] | (i < j)
        ea.append(i[keep])
        eb.append(j[keep])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    cc = core[ea]
    root, rounds = _components(n, ea[cc], eb[cc])
    least = np.full(n, n, np.int64)
    np.minimum.at(least, ea[~cc], root[eb[~cc]])
    root = np.where(core, root, least)
    ids = np.unique(root[core])
    labels = np.where(root < n, np.searchsorted(ids, np.minimum(root, n - 1)), -1).astype(np.int32)
    return DbscanResult(labels, core, counts.astype(np.int32), rounds)


# ---- device

def _dbscan_device(X, eps, min_samples, raw=False):
    L = Launcher(X)
    torch, dev = L.torch, L.dev
    n, d = (int(s) for s in X.shape)
    ms = int(min(min_samples, 2 ** 31 - 1))
    with torch.cuda.device(dev):
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        label = torch.empty(n, dtype=torch.int32, device=dev)
        other = torch.empty(n, dtype=torch.int32, device=dev)
        changed = torch.empty(1, dtype=torch.int32, device=dev)
        L.call("ra_dbscan_count", ptr(X), n, d, float(eps), ms, ptr(counts), ptr(label))
        core = counts >= ms
        cap = int(core.sum().item()) + 1
        rounds = 0
        while True:
            if rounds >= cap:
                raise RuntimeError("dbscan: %d merging rounds for %d core points: every unfinished round lowers a label" % (rounds, cap - 1))
            L.call("ra_dbscan_step", ptr(X), n, d, float(eps), ptr(counts), ms, ptr(label), ptr(other), ptr(changed))
            rounds += 1
            label, other = other, label
            if int(changed.item()) == 0:
                break
        ids = torch.unique(label[core].to(torch.int64))           # sorted: the components by their lowest core index
        lab64 = label.to(torch.int64)
        if ids.numel():
            mapped = torch.searchsorted(ids, lab64.clamp(min=0))
            labels = torch.where(lab64 >= 0, mapped, torch.full_like(lab64, -1)).to(torch.int32)
        else:
            labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
        res = DbscanResult(labels.cpu().numpy(), core.cpu().numpy(), counts.cpu().numpy(), rounds)
        if raw:
            return res, label.cpu().numpy(), int(changed.item())
        return res


def dbscan(X, eps, min_samples=5, backend="device"):
    """DBSCAN of X [n][d] by the rules at the top of this module: DbscanResult(labels int32 [n] with -1 for noise, core_mask,
    core_sample_indices, n_clusters, counts, n_rounds).  Euclidean metric only; no sample_weight, no precomputed or sparse input,
    one GPU, at most 262144 points."""
    X = _common.as_input(X, backend, DbscanError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, eps, min_samples)
    _common.check_finite(X, backend, DbscanError)
    if backend == "numpy":
        return _dbscan_numpy(X, eps, int(min_samples))
    return _dbscan_device(X, eps, int(min_samples))


def kdistances(X, min_samples, backend="device"):
    """float64 [n]: for each point the least eps at which it is a core point, i.e. the distance to its (min_samples - 1)-th nearest
    other point; 0 for min_samples = 1, inf for min_samples > n.  The device reads the last column of ra_tsne_knn and has its
    domain: n >= 2 and min_samples - 1 <= 301."""
    X = _common.as_input(X, backend, DbscanError, numpy_dtype=np.float32)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, 1.0, min_samples)
    _common.check_finite(X, backend, DbscanError)
    k = int(min_samples) - 1
    if k == 0:
        return np.zeros(n)
    if k > n - 1:
        return np.full(n, np.inf)
    if backend == "numpy":
        Xd = np.asarray(X, np.float64)
        out = np.empty(n)
        for s0, s1 in row_chunks(n):
            out[s0:s1] = np.partition(d2_rows(Xd, s0, s1), k, axis=1)[:, k]        # the point itself is the 0-th
        return np.sqrt(out)
    if k > MAX_KNN:
        raise DbscanError("the device takes min_samples - 1 <= %d, got min_samples = %d" % (MAX_KNN, min_samples))
    L = Launcher(X)
    torch = L.torch
    with torch.cuda.device(X.device):
        return torch.sqrt(_graph.knn(L, X, k)[1][:, k - 1]).cpu().numpy()


# ---- command line

def main(argv=None):
    from . import kmeans
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.dbscan")
    _common.add_cluster_arguments(ap, ("input", "output"), "embedding", True)
    ap.add_argument("--eps", type=float, default=None, help="neighbourhood radius (optional with --kdist)")
    ap.add_argument("--min_samples", type=int, default=5, help="neighbours, itself included, that make a core point")
    _common.add_cluster_arguments(ap, ("--key", "--backend"), "embedding", True)
    ap.add_argument("--kdist", action="store_true", help="store the sorted k-distances as kdist and print their quantiles")
    _common.add_cluster_arguments(ap, ("--truth", "--stack", "--params", "--ou", "--averages", "--device"), "embedding", True)
    args = ap.parse_args(argv)
    if args.eps is None and not args.kdist:
        ap.error("one of --eps and --kdist is needed")
    if args.eps is not None and not (math.isfinite(args.eps) and args.eps > 0):
        ap.error("--eps must be a finite number > 0")
    _common.check_averages_arguments(ap, args)
    if args.averages and args.eps is None:
        ap.error("--averages needs --eps")
    try:
        X = kmeans.read_input(args.input, args.key)
        n, d = X.shape
        check_domain(n, d, 1.0 if args.eps is None else args.eps, args.min_samples)
        truth = kmeans.read_truth(args.truth, n) if args.truth else None
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device" or args.averages:
        _common.require_gpu(_common.NO_GPU)
    Xb = _common.to_device(X, args.device) if args.backend == "device" else X
    out = dict(min_samples=np.int64(args.min_samples), key=np.str_(args.key), backend=np.str_(args.backend),
               eps=np.float64(np.nan if args.eps is None else args.eps))
    try:
        if args.kdist:
            kd = np.sort(kdistances(Xb, args.min_samples, backend=args.backend))
            out["kdist"] = kd
            print("k-distances (min_samples = %d): %s" % (args.min_samples, ", ".join(
                "%d %% %.6g" % (q, np.quantile(kd, q / 100.0)) for q in (50, 75, 90, 95, 99))))
        res = dbscan(Xb, args.eps, args.min_samples, backend=args.backend) if args.eps is not None else None
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    msg = "%s: %d points x %d" % (args.output, n, d)
    if res is not None:
        out.update(labels=res.labels, core_mask=res.core_mask, counts=res.counts, n_clusters=np.int64(res.n_clusters),
                   n_noise=np.int64(res.n_noise), n_rounds=np.int64(res.n_rounds))
        size = np.bincount(res.labels[res.labels >= 0], minlength=res.n_clusters)
        cores = np.bincount(res.labels[res.core_mask], minlength=res.n_clusters)
        for c in range(res.n_clusters):
            print("cluster %4d: %7d members, %7d core points" % (c, size[c], cores[c]))
        print("noise: %d points" % res.n_noise)
        msg += ", eps = %g, min_samples = %d: %d clusters, %d noise, %d rounds" % (args.eps, args.min_samples, res.n_clusters, res.n_noise,
                                                                               res.n_rounds)
        keep = res.labels >= 0
        if truth is not None:
            msg += _common.truth_scores(out, truth, res.labels, keep)
        if args.averages:
            msg += _common.write_averages(args, n, res.labels, res.n_clusters, keep, DbscanError, MAX_AVERAGES)
    np.savez(args.output, **out)
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
