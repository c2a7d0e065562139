"""Trustworthiness and continuity of an embedding Y [n][d_Y] of X [n][d_X] on the GPU (sklearn.manifold.trustworthiness 1.7,
metric="euclidean"), with the per-point scores and the co-ranking curve.

    python -m cryo_ralib_amd.quality HIGH LOW OUT.npz [--high_key factors] [--low_key embedding] [--k 10] [--sample_size N --seed S]
                                     [--backend device|numpy] [--worst M] [--device 0]

HIGH and LOW are the OUT.npz of the sdr and tsne tools (--high_key / --low_key name their arrays) or [n][d] .npy files with the same
rows.  OUT.npz holds trustworthiness, continuity, trust_point, cont_point, qnx, lcmc, k_best, sample_indices and the options used;
the tool prints T, C and k_best, and with --worst M the M rows of least trust_point (the particles most likely put in the wrong
island).  More than 262144 rows need --sample_size.

The contract, rule by rule:
  1. Distance.  D2(A; i, j) = sum_t (a_it - a_jt)^2 in double from the differences of the float32 values, the features in order
     (DBSCAN's rule 2): D2(i, i) = 0 exactly and D2(i, j) = D2(j, i) bit for bit.  The device fuses each multiply-add, the numpy
     checker (_common.d2_rows) does not: where every term is exactly representable the two agree in every bit; elsewhere a rank
     may differ only for an entry with a column whose |D2 - threshold| <= d 2^-50 threshold.
  2. Total order.  In the row of i, column l precedes column j iff (D2(i, l), l) < (D2(i, j), j) lexicographically.  Column i
     itself is never counted.  rank_A(i, j) = 1 + #{l != i : l precedes j}, so it lies in 1 .. n - 1.  It is a pure function of
     the data: ties go to the lower index (sklearn's unstable argsort leaves them undefined).
  3. Neighbours.  N_B(i) is the list of ra_tsne_knn on B: i excluded, ordered by (D2, index), length k.
  4. Trustworthiness.  pen_i = sum_{j in N_Y(i)} max(0, rank_X(i, j) - k); trust_i = 1 - 2 pen_i / (k (2 n - 3 k - 1));
     T = mean_i trust_i, formed as 1 - 2 sum_i pen_i / (n k (2 n - 3 k - 1)) with the penalties summed as integers (int64) and one
     division.  k < n / 2 is required, else a ValueError with sklearn's message.  Continuity is the same with X and Y swapped:
     neighbours in X, ranks in Y.
  5. Co-ranking curve, from trustworthiness' rank table.  Q_NX(K) = #{(i, t) : t < K and rank_X(i, N_Y(i)[t]) <= K} / (n K) for
     K = 1 .. k; LCMC(K) = Q_NX(K) - K / (n - 1); k_best = argmax LCMC, the smaller K on ties.
  6. Purity.  Everything returned is a pure function of (X, Y, k), bitwise the same call to call and stream to stream: no
     floating-point atomics, no floating-point sum across threads; the counts are integers.
Domain: 3 <= n <= 262144 rows on both sides, 1 <= d <= 2048 on both sides, 1 <= n_neighbors <= 301 and n_neighbors < n / 2, finite
input.  Anything else raises QualityError (a ValueError) before anything is launched.  embedding_quality's sample_size is the only
way past 262144 rows, up to 4194304.
Not built: other metrics, precomputed distances, stress and Shepard diagrams, multi-GPU.

On the device the neighbours are ra_tsne_knn's and the ranks ra_embed_ranks' (csrc/ralign_quality.h): one pass over the n^2
distances of the rank space per 24 list entries, each compared against the row's sorted thresholds in LDS; nothing of size n^2 is
stored.  The kNN's float32 screen keeps its documented limit on uncentred data (README, t-SNE): rows far from the origin compared
with their spread can lose true neighbours from the list; centre such data first.  backend="numpy" is the float64 checker: chunked
over rows (_common.row_chunks), neighbours and ranks from a stable sort of each row of D2, no [n][n] array, no GPU.
"""
import argparse
import collections
import sys

import numpy as np

from . import _common, _graph
from ._common import Launcher, d2_rows, is_int, ptr, row_chunks

MAX_N, MAX_D, MAX_K, MAX_ROWS = 262144, 2048, 301, 4194304

QualityDetails = collections.namedtuple("QualityDetails", "score point ranks neighbors")
QualityResult = collections.namedtuple("QualityResult",
                                       "trustworthiness continuity trust_point cont_point qnx lcmc k_best sample_indices")


class QualityError(ValueError):
    """an input outside the supported domain"""


def _need(ok, msg):
    if not ok:
        raise QualityError(msg)


def check_neighbors(n, n_neighbors):
    """rule 4's condition on k, for the n rows that are evaluated"""
    _need(is_int(n_neighbors), "n_neighbors must be an integer, got %r" % (n_neighbors,))
    _need(1 <= n_neighbors <= MAX_K, "need 1 <= n_neighbors <= %d, got %d" % (MAX_K, n_neighbors))
    _need(n_neighbors < n / 2, "n_neighbors (%d) should be less than n_samples / 2 (%s)" % (n_neighbors, n / 2))


def check_shape(n, d, what="X"):
    _need(3 <= n <= MAX_N, "need 3 <= n <= %d rows, got %d" % (MAX_N, n))
    _need(1 <= d <= MAX_D, "need 1 <= d <= %d features in %s, got %d" % (MAX_D, what, d))


def check_domain(n, d_x, d_y, n_neighbors, n_y=None):
    """raise QualityError unless the shapes and k are inside the supported domain"""
    _need(n_y is None or n_y == n, "X has %d rows, Y %s" % (n, n_y))
    check_shape(n, d_x, "X")
    check_shape(n, d_y, "Y")
    check_neighbors(n, n_neighbors)


def draw_sample(n, sample_size, random_state=None):
    """the evaluated rows of embedding_quality: sorted(check_random_state(random_state).permutation(n)[:sample_size])"""
    _need(is_int(sample_size) and 3 <= sample_size <= min(n, MAX_N),
          "need 3 <= sample_size <= min(n, %d), got %r for %d rows" % (MAX_N, sample_size, n))
    rs = _common.check_random_state(int(random_state) if isinstance(random_state, bool) else random_state, QualityError)
    return np.sort(rs.permutation(n)[:sample_size]).astype(np.int64)


# ---- rules 4 and 5 from a rank table (integers in, one division)

def scores_from_penalties(pen, n, k):
    """(score, point [n] float64) of rule 4 from the int64 penalties"""
    pen = np.asarray(pen, np.int64)
    point = 1.0 - pen * (2.0 / (k * (2.0 * n - 3.0 * k - 1.0)))
    return float(1.0 - int(pen.sum()) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))), point


def penalties(ranks, k):
    """pen [n] int64 of rule 4 from the rank table [n][k]; an invalid entry (rank 0) adds nothing"""
    return np.maximum(np.asarray(ranks, np.int64) - k, 0).sum(axis=1)


def coranking(ranks):
    """(qnx [k], lcmc [k], k_best) of rule 5 from trustworthiness' rank table [n][k]"""
    ranks = np.asarray(ranks, np.int64)
    n, k = ranks.shape
    first = np.maximum(ranks, np.arange(1, k + 1)[None, :])         # the least K at which entry (i, t) counts
    first = first[(ranks > 0) & (first <= k)]
    return _curve(np.bincount(first, minlength=k + 1)[1:k + 1], n, k)


def _curve(hist, n, k):
    K = np.arange(1, k + 1)
    qnx = np.cumsum(np.asarray(hist, np.int64)) / (n * K.astype(np.float64))
    lcmc = qnx - K / (n - 1.0)
    return qnx, lcmc, int(np.argmax(lcmc)) + 1


# ---- CPU checker (float64 numpy)

def _sorted_rows(A, s0, s1):
    """the columns of rows s0 .. s1 - 1 in rule 2's order, the row's own column last"""
    D = d2_rows(A, s0, s1)
    D[np.arange(s1 - s0), np.arange(s0, s1)] = np.inf
    return np.argsort(D, axis=1, kind="stable")


def knn_numpy(B, k):
    """N_B [n][k] int64 of rule 3, by rule 2's difference chains, the row itself left out (tsne.knn_numpy screens by a Gram matrix
    first and tsne.knn_query_numpy leaves nothing out: they stay apart)"""
    B = np.asarray(B, np.float64)
    n = B.shape[0]
    idx = np.empty((n, k), np.int64)
    for s0, s1 in row_chunks(n):
        idx[s0:s1] = _sorted_rows(B, s0, s1)[:, :k]
    return idx


def ranks_numpy(A, idx):
    """rank_A(i, idx[i][t]) int32 [n][k] of rule 2; 0 for an entry outside 0 .. n - 1 or equal to i"""
    A = np.asarray(A, np.float64)
    idx = np.asarray(idx, np.int64)
    n = A.shape[0]
    out = np.zeros(idx.shape, np.int32)
    for s0, s1 in row_chunks(n):
        order = _sorted_rows(A, s0, s1)
        rows = np.arange(s1 - s0)[:, None]
        inv = np.empty((s1 - s0, n), np.int32)
        inv[rows, order] = np.arange(1, n + 1, dtype=np.int32)[None, :]
        j = idx[s0:s1]
        ok = (j >= 0) & (j < n) & (j != np.arange(s0, s1)[:, None])
        out[s0:s1] = np.where(ok, inv[rows, np.where(ok, j, 0)], 0)
    return out


# ---- device

def _ranks_device(L, A, idx, want_ranks=True, want_pen=True):
    """(rank int32 [n][k] or None, pen int64 [n] or None) of ra_embed_ranks, on the device"""
    n, d = (int(s) for s in A.shape)
    k = int(idx.shape[1])
    torch = L.torch
    rank = torch.empty((n, k), dtype=torch.int32, device=L.dev) if want_ranks else None
    pen = torch.empty(n, dtype=torch.int64, device=L.dev) if want_pen else None
    L.call("ra_embed_ranks", ptr(A), n, d, ptr(idx), k, ptr(rank), ptr(pen))
    return rank, pen


def _coranking_device(torch, rank):
    n, k = (int(s) for s in rank.shape)
    r = rank.to(torch.int64)
    first = torch.maximum(r, torch.arange(1, k + 1, device=rank.device, dtype=torch.int64)[None, :])
    first = first[(r > 0) & (first <= k)]
    return _curve(torch.bincount(first, minlength=k + 1)[1:k + 1].cpu().numpy(), n, k)


# ---- public

def _inputs(X, Y, backend):
    X = _common.as_input(X, backend, QualityError, numpy_dtype=np.float32)
    Y = _common.as_input(Y, backend, QualityError, numpy_dtype=np.float32)
    if backend == "device" and Y.device != X.device:
        raise QualityError("X and Y are on different devices")
    return X, Y


def neighbor_ranks(A, idx, backend="device"):
    """int32 [n][k]: rank_A(i, idx[i][t]) of rule 2 for integer lists idx [n][k] that may come from anywhere (1 <= k <= 301, not
    tied to n; an entry may repeat).  An entry outside 0 .. n - 1, or equal to i, gets rank 0."""
    A = _common.as_input(A, backend, QualityError, numpy_dtype=np.float32)
    n, d = (int(s) for s in A.shape)
    check_shape(n, d, "A")
    if not isinstance(idx, np.ndarray) and hasattr(idx, "detach"):
        idx = idx.detach().cpu().numpy()
    idx = np.asarray(idx)
    _need(idx.ndim == 2 and idx.shape[0] == n and np.issubdtype(idx.dtype, np.integer),
          "idx is an integer array [n][k] with A's %d rows, got %s %s" % (n, idx.dtype, idx.shape))
    k = int(idx.shape[1])
    _need(1 <= k <= MAX_K, "need 1 <= k <= %d list entries, got %d" % (MAX_K, k))
    _common.check_finite(A, backend, QualityError)
    if backend == "numpy":
        return ranks_numpy(A, idx)
    idx = np.where((idx >= 0) & (idx < n), idx, -1).astype(np.int32)
    L = Launcher(A)
    with L.torch.cuda.device(L.dev):
        rank, _ = _ranks_device(L, A, L.torch.from_numpy(np.ascontiguousarray(idx)).to(L.dev), want_pen=False)
        return rank.cpu().numpy()


def _one_direction(rank_space, list_space, k, backend, details):
    """rule 4 with neighbours in list_space and ranks in rank_space"""
    n = int(rank_space.shape[0])
    if backend == "numpy":
        idx = knn_numpy(list_space, k)
        ranks = ranks_numpy(rank_space, idx)
        pen = penalties(ranks, k)
    else:
        L = Launcher(rank_space)
        with L.torch.cuda.device(L.dev):
            idx = _graph.knn(L, list_space, k)[0]
            ranks, pen = _ranks_device(L, rank_space, idx, want_ranks=details)
            pen = pen.cpu().numpy()
            if details:
                ranks, idx = ranks.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    score, point = scores_from_penalties(pen, n, k)
    return QualityDetails(score, point, ranks, idx) if details else score


def _checked(X, Y, n_neighbors, backend):
    X, Y = _inputs(X, Y, backend)
    check_domain(int(X.shape[0]), int(X.shape[1]), int(Y.shape[1]), n_neighbors, int(Y.shape[0]))
    _common.check_finite(X, backend, QualityError)
    _common.check_finite(Y, backend, QualityError)
    return X, Y


def trustworthiness(X, Y, n_neighbors=5, backend="device", details=False):
    """T of rule 4 (sklearn.manifold.trustworthiness(X, Y, n_neighbors=n_neighbors)): to what extent the k nearest neighbours in
    the embedding Y are near in X.  details=True: QualityDetails(score, point [n] float64 (trust_i), ranks int32 [n][k]
    (rank_X(i, N_Y(i)[t])), neighbors int64 [n][k] (N_Y)).  The device kNN's float32 screen has its documented limit on uncentred
    data."""
    X, Y = _checked(X, Y, n_neighbors, backend)
    return _one_direction(X, Y, int(n_neighbors), backend, details)


def continuity(X, Y, n_neighbors=5, backend="device", details=False):
    """C of rule 4: trustworthiness with X and Y swapped (neighbours in X, ranks in Y): to what extent the neighbours in X stay
    near in the embedding.  details as trustworthiness."""
    X, Y = _checked(X, Y, n_neighbors, backend)
    return _one_direction(Y, X, int(n_neighbors), backend, details)


def _gather(A, s):
    if isinstance(A, np.ndarray):
        return np.ascontiguousarray(A[s])
    import torch
    return A[torch.from_numpy(s).to(A.device)].contiguous()


def embedding_quality(X, Y, n_neighbors=10, sample_size=None, random_state=None, backend="device"):
    """QualityResult(trustworthiness, continuity, trust_point [n], cont_point [n] (float64), qnx [k], lcmc [k], k_best,
    sample_indices) by rules 4 and 5: one device copy of X and Y, two kNN calls and two rank calls.  With sample_size the pair
    (X[s], Y[s]), s = draw_sample(n, sample_size, random_state), is evaluated instead (the only way past 262144 rows, up to
    4194304); the point arrays are nan outside s and sample_indices is s (None without a sample).  The device kNN's float32 screen
    has its documented limit on uncentred data."""
    _need(backend in ("device", "numpy"), "backend is 'device' or 'numpy', got %r" % (backend,))
    for A in (X, Y):
        _need(hasattr(A, "shape") and len(A.shape) == 2, "X and Y are [n][d] arrays")
    n_all = int(X.shape[0])
    _need(int(Y.shape[0]) == n_all, "X has %d rows, Y %d" % (n_all, int(Y.shape[0])))
    s = None
    if sample_size is not None:
        _need(n_all <= MAX_ROWS, "need at most %d rows, got %d" % (MAX_ROWS, n_all))
        s = draw_sample(n_all, sample_size, random_state)
        X, Y = _gather(X, s), _gather(Y, s)
    X, Y = _checked(X, Y, n_neighbors, backend)
    n, k = int(X.shape[0]), int(n_neighbors)
    if backend == "numpy":
        ranks = ranks_numpy(X, knn_numpy(Y, k))
        pen_t, pen_c = penalties(ranks, k), penalties(ranks_numpy(Y, knn_numpy(X, k)), k)
        qnx, lcmc, k_best = coranking(ranks)
    else:
        L = Launcher(X)
        with L.torch.cuda.device(L.dev):
            ranks, pen_t = _ranks_device(L, X, _graph.knn(L, Y, k)[0])
            _, pen_c = _ranks_device(L, Y, _graph.knn(L, X, k)[0], want_ranks=False)
            qnx, lcmc, k_best = _coranking_device(L.torch, ranks)
            pen_t, pen_c = pen_t.cpu().numpy(), pen_c.cpu().numpy()
    T, tp = scores_from_penalties(pen_t, n, k)
    C, cp = scores_from_penalties(pen_c, n, k)
    if s is not None:
        full_t, full_c = np.full(n_all, np.nan), np.full(n_all, np.nan)
        full_t[s], full_c[s] = tp, cp
        tp, cp = full_t, full_c
    return QualityResult(T, C, tp, cp, qnx, lcmc, k_best, s)


# ---- command line

def check_tool_arguments(ap, n_high, n_low, k, sample_size):
    """the usage errors the quality tool and the tsne tool's --quality share (status 2, before the device is touched); returns
    the number of evaluated rows"""
    if n_high != n_low:
        ap.error("the inputs differ in rows: %d and %d" % (n_high, n_low))
    if sample_size is None and n_high > MAX_N:
        ap.error("%d rows: more than %d need a sample size" % (n_high, MAX_N))
    if sample_size is not None and not 3 <= sample_size <= min(n_high, MAX_N):
        ap.error("the sample size must lie in 3 .. min(n, %d), got %d for %d rows" % (MAX_N, sample_size, n_high))
    n = n_high if sample_size is None else sample_size
    if not 1 <= k <= MAX_K or k >= n / 2:
        ap.error("need 1 <= K <= %d and K < n / 2 for the %d evaluated rows, got K = %d" % (MAX_K, n, k))
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.quality")
    ap.add_argument("high", help="the input space: OUT.npz of the sdr tool, or an [n][d] .npy")
    ap.add_argument("low", help="the embedding: OUT.npz of the tsne tool, or an [n][d] .npy")
    ap.add_argument("output", help="OUT.npz")
    ap.add_argument("--high_key", default="factors", help="array of an .npz HIGH (default factors)")
    ap.add_argument("--low_key", default="embedding", help="array of an .npz LOW (default embedding)")
    ap.add_argument("--k", type=int, default=10, help="neighbours (default 10)")
    ap.add_argument("--sample_size", type=int, default=None, help="evaluate this many drawn rows (--seed); needed above %d rows" % MAX_N)
    ap.add_argument("--seed", type=int, default=None, help="random_state of the sample")
    ap.add_argument("--backend", default="device", choices=("device", "numpy"))
    ap.add_argument("--worst", type=int, default=0, help="print the M rows of least trust_point")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.seed is not None and args.sample_size is None:
        ap.error("--seed goes with --sample_size")
    if args.worst < 0:
        ap.error("--worst must be >= 0")
    try:
        X = _common.read_input(args.high, args.high_key, QualityError)
        Y = _common.read_input(args.low, args.low_key, QualityError)
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    check_tool_arguments(ap, X.shape[0], Y.shape[0], args.k, args.sample_size)
    if args.backend == "device":
        _common.require_gpu("no GPU visible: use --backend numpy for the CPU checker")
    try:
        if args.backend == "device":
            import torch
            with torch.cuda.device(args.device):
                res = embedding_quality(X, Y, args.k, args.sample_size, args.seed, "device")
        else:
            res = embedding_quality(X, Y, args.k, args.sample_size, args.seed, "numpy")
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    s = np.arange(X.shape[0], dtype=np.int64) if res.sample_indices is None else res.sample_indices
    np.savez(args.output, trustworthiness=np.float64(res.trustworthiness), continuity=np.float64(res.continuity),
             trust_point=res.trust_point, cont_point=res.cont_point, qnx=res.qnx, lcmc=res.lcmc, k_best=np.int64(res.k_best),
             sample_indices=s, k=np.int64(args.k), sample_size=np.int64(-1 if args.sample_size is None else args.sample_size),
             seed=np.int64(-1 if args.seed is None else args.seed), backend=np.str_(args.backend), high_key=np.str_(args.high_key),
             low_key=np.str_(args.low_key))
    print("%s: %d of %d rows, %d -> %d features, k = %d: trustworthiness %.6f, continuity %.6f, k_best %d (LCMC %.4f)" % (
        args.output, s.size, X.shape[0], X.shape[1], Y.shape[1], args.k, res.trustworthiness, res.continuity, res.k_best,
        res.lcmc[res.k_best - 1]))
    if args.worst:
        worst = s[np.argsort(res.trust_point[s], kind="stable")[:args.worst]]
        for i in worst:
            print("row %8d: trust %.6f, continuity %.6f" % (i, res.trust_point[i], res.cont_point[i]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
