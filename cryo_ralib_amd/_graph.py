"""Neighbour lists and the CSR graphs built from them: what tsne, umap, spectral, quality, dbscan, hdbscan and ward share below
their own rules.  Like _common, nothing here imports a feature module at module level; torch is imported where tensors are touched.

    knn, knn_query          the exact neighbour lists of ra_tsne_knn / ra_tsne_knn_query (csrc/ralign_knn.h) as device tensors.
    symmetrize_numpy,       a list with one value per entry -> the CSR pattern of the list united with its transpose, and per stored
    symmetrize_torch        entry (i, j) the pair (value of j in i's list, value of i in j's list), 0 where absent.  The caller
                            combines the pair by its own rule (a + b, (a + b) / 2, a + b - a b) and casts the indices.
    row_ids_numpy,          the row of every stored entry of a CSR.
    row_ids_torch
    jump                    pointer doubling.
"""
import numpy as np

from ._common import ptr


# ---- device neighbour lists

def _lists(L, rows, k):
    torch = L.torch
    return torch.empty((rows, k), dtype=torch.int32, device=L.dev), torch.empty((rows, k), dtype=torch.float64, device=L.dev)


def knn(L, X, k):
    """(idx int32 [n][k], dist2 float64 [n][k]) of the k nearest other rows of every row of X, by (squared distance, index); L is
    the Launcher of X's device"""
    n, d = (int(s) for s in X.shape)
    idx, d2 = _lists(L, n, k)
    L.call("ra_tsne_knn", ptr(X), n, d, k, ptr(idx), ptr(d2))
    return idx, d2


def knn_query(L, Q, X, k):
    """(idx int32 [nq][k], dist2 float64 [nq][k]) of the k rows of X nearest every row of Q; no row is left out"""
    nq, d = (int(s) for s in Q.shape)
    idx, d2 = _lists(L, nq, k)
    L.call("ra_tsne_knn_query", ptr(Q), nq, ptr(X), int(X.shape[0]), d, k, ptr(idx), ptr(d2))
    return idx, d2


# ---- list -> symmetric CSR: a stable sort of the keys i n + j of the entries and of their transposes, so a key's (at most two)
# values lie side by side, the list's own entry first unless only the transpose exists; deterministic (no scatter)

def symmetrize_numpy(idx, val):
    """(indptr int64 [n + 1], indices int64 [nnz], first [nnz], second [nnz]) of idx [n][k] (no row lists itself or a row twice)
    and val [n][k]: the columns of a row ascend; first is the entry's value where row i lists j, else the transpose's; second
    is the transpose's value where both exist, else 0"""
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1).astype(np.int64)
    keys = np.concatenate([rows * n + cols, cols * n + rows])
    vals = np.concatenate([val.reshape(-1), val.reshape(-1)])
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    uk, start, counts = np.unique(keys, return_index=True, return_counts=True)
    second = np.where(counts == 2, vals[np.minimum(start + 1, len(vals) - 1)], 0.0)
    indptr = np.searchsorted(uk // n, np.arange(n + 1, dtype=np.int64)).astype(np.int64)
    return indptr, uk % n, vals[start], second


def symmetrize_torch(idx, val):
    """symmetrize_numpy on tensors of any one device (the CPU included), with the same bits"""
    import torch
    n, k = (int(s) for s in idx.shape)
    rows = torch.arange(n, device=idx.device, dtype=torch.int64).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    keys = torch.cat([rows * n + cols, cols * n + rows])
    vals = torch.cat([val.reshape(-1), val.reshape(-1)])
    keys, order = torch.sort(keys, stable=True)
    vals = vals[order]
    uk, counts = torch.unique_consecutive(keys, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    second = vals[torch.clamp(start + 1, max=vals.numel() - 1)]
    second = torch.where(counts == 2, second, torch.zeros_like(second))
    indptr = torch.searchsorted(uk // n, torch.arange(n + 1, device=idx.device, dtype=torch.int64))
    return indptr, uk % n, vals[start], second


# ---- CSR rows

def row_ids_numpy(indptr):
    """int64 [nnz]: the row of every stored entry"""
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def row_ids_torch(indptr):
    import torch
    n = int(indptr.numel()) - 1
    return torch.arange(n, device=indptr.device, dtype=torch.int64).repeat_interleave((indptr[1:] - indptr[:-1]).long())


# ---- pointer doubling

def jump(up):
    """the fixed point of x -> up[x] for every x, by pointer doubling"""
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            return up
        up = nxt
