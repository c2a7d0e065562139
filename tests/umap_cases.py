"""What the UMAP suites (tests/test_umap_cpu.py, tests/test_gpu_umap.py) share: the data generators and the builders of the kernel
tests, with the conditions the GPU file relies on (asserted in the CPU file)."""
import numpy as np

from cryo_ralib_amd import _graph, umap

U = 2.0 ** -53
SK_ROWS = 4                 # rows per workgroup of umap_smooth_kernel
LANES, ROWS = 16, 16        # lanes per row and rows per workgroup of umap_epoch_kernel / umap_place_kernel
MARGIN = 1e-9               # rule 2: a row whose bisection came closer than this to another branch is left out of the entry check
MAX_LEFT_OUT = 0.01         # ... and at most this share of a case's rows
Q_MIN = 1e-30               # no pair of an epoch case has 0 < q < Q_MIN
POW_ULPS = 16               # OpenCL's allowance for pow
A, B = 1.5769434603, 0.8950608779


def blobs(n=1500, d=10, k=6, seed=0):
    """the issue's prototype case: k Gaussian blobs drawn as centres * 4 + N(0, 1): (X float32, truth)"""
    rng = np.random.RandomState(seed)
    cent = rng.standard_normal((k, d)) * 4.0
    lab = rng.randint(0, k, n)
    return (cent[lab] + rng.standard_normal((n, d))).astype(np.float32), lab


# ---- rule 2

def smooth_rows(rows, k, seed, scale=1.0):
    """[rows][k] ascending squared distances of a Gaussian cloud's flavour"""
    rng = np.random.default_rng(seed)
    d = np.sort(scale * (0.5 + np.abs(rng.normal(size=(rows, k))) + 0.3 * rng.uniform(size=(rows, 1))), axis=1)
    return d * d


def smooth_cases():
    """name -> (dist2 [rows][k], n_neighbors): every k at which the kernel's lane plan changes, rows around its tile, and the
    special rows"""
    out = {}
    for k in (1, 2, 14, 63, 64, 65, 301):
        out["k%d" % k] = (smooth_rows(3 * SK_ROWS + 5, k, 100 + k), k + 1)
    for rows in (SK_ROWS - 1, SK_ROWS, SK_ROWS + 1):
        out["rows%d" % rows] = (smooth_rows(rows, 14, 200 + rows), 15)
    out["query"] = (smooth_rows(9, 15, 301), 15)                    # transform: k = n_neighbors, target log2(n_neighbors)
    d2 = smooth_rows(8, 14, 302)
    d2[0, :] = 0.0                                                   # every neighbour a duplicate: rho = 0, w = 1
    d2[1, :3] = 0.0                                                  # three duplicates, then distinct rows
    d2[2, :6] = d2[2, 6]                                             # six rows at the least distance: psum >= 6 > target, the floor
    d2[3] = smooth_rows(1, 14, 303, scale=1e6)[0]                    # mid doubles about twenty times
    d2[4] = smooth_rows(1, 14, 304, scale=1e-6)[0]                   # ... and halves as often
    out["special"] = (d2, 15)
    return out


# ---- rule 6

def csr(lengths, n, seed):
    """a CSR with the given row lengths and ascending distinct columns in 0 .. n - 1 without the diagonal"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    cols = []
    for i, L in enumerate(lengths):
        others = np.delete(np.arange(n), i)
        cols.append(np.sort(rng.choice(others, int(L), replace=False)))
    return indptr, (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)


class EpochCase:
    def __init__(self, lengths, seed, n_epochs=20, neg=5, states=True):
        n = len(lengths)
        rng = np.random.default_rng(seed)
        self.n, self.n_epochs, self.neg, self.seed = n, n_epochs, neg, seed
        self.indptr, self.indices = csr(lengths, n, seed)
        nnz = len(self.indices)
        # positions on a grid of 2^-10 in [1, 9): every difference is exact and q is 0 or >= 2^-20
        Y = 1.0 + np.floor(rng.uniform(0.0, 8.0, (n, 2)) * 1024.0) / 1024.0
        if states and n >= 12:
            g = max(4, n // 6)
            Y[n // 3: n // 3 + g] = Y[n // 3]                       # coincident points: negatives meet q = 0
            near = np.arange(2 * n // 3, 2 * n // 3 + g)            # a clump 2^-10 apart: negatives meet the repulsive clip
            Y[near] = Y[near[0]] + np.stack([np.arange(g) / 1024.0, np.zeros(g)], axis=1)
            # states on attractive entries, from the CSR itself: the first three columns of the first row that has three
            i0 = int(np.nonzero(np.diff(self.indptr) >= 3)[0][0])
            j = self.indices[self.indptr[i0]: self.indptr[i0] + 3]
            Y[j[0]] = Y[i0]                                         # q = 0 on an attractive pair
            Y[j[1]] = Y[i0] + np.array([0.0078125, 0.0])            # a pair at distance 2^-7
            Y[j[2]] = Y[i0] + np.array([1000.0, 0.0])               # a pair at distance 1e3
            self.state_entries = self.indptr[i0] + np.arange(3)
        self.Y = Y.astype(np.float32)
        r = rng.uniform(0.0, 1.0, nnz)
        r[rng.uniform(size=nnz) < 0.3] = 1.0                        # fires in every epoch
        r[rng.uniform(size=nnz) < 0.1] = 0.5 / n_epochs             # r < 1 / n_epochs: never fires
        if states and n >= 12:
            r[self.state_entries] = 1.0                             # the three state entries fire in every epoch
        self.rate = r

    def reference(self, t, seed=42, gamma=1.0, lr=1.0):
        return umap.epoch_numpy(self.Y, self.indptr, self.indices, self.rate, A, B, t, self.n_epochs, gamma, self.neg, lr, seed)

    def terms(self, t):
        """the number of terms vertex i adds in epoch t, [n]"""
        f = umap.fires(self.rate, t)
        return np.bincount(_graph.row_ids_numpy(self.indptr.astype(np.int64))[f], minlength=self.n) * (1 + self.neg)


def epoch_lengths():
    """name -> row lengths: every length at which a lane gains an entry, and n around the rows of a workgroup"""
    rng = np.random.default_rng(7)
    edge = [0, 1, 15, 16, 17, 63, 64, 65, 300]
    out = {"edges": np.array(edge + list(rng.integers(0, 20, 320 - len(edge))))}
    for n in (ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1):
        out["n%d" % n] = rng.integers(0, min(n - 1, 12) + 1, n)
    out["n4"] = np.array([3, 3, 2, 1])
    return out


def epoch_cases():
    """name -> EpochCase"""
    out = {name: EpochCase(L, 11 + i) for i, (name, L) in enumerate(sorted(epoch_lengths().items()))}
    for neg in (0, 1, 16):
        out["neg%d" % neg] = EpochCase(epoch_lengths()["n33"], 40 + neg, neg=neg)
    return out


def epoch_bound(case, t, lr=1.0):
    """[n]: the most the double values behind a coordinate can differ between device and checker: each of the vertex's terms is at
    most 8 in magnitude (a clipped move, doubled for the attraction) and carries a relative error of at most 4 (POW_ULPS + 8) u (pow
    on both sides within POW_ULPS ulps, four operations around it, each side rounding once), times alpha"""
    return case.terms(t) * 8.0 * umap.alpha_at(lr, t, case.n_epochs) * 4.0 * (POW_ULPS + 8) * U


def ulp32(v):
    """the spacing of float32 at |v|"""
    v = np.abs(np.asarray(v, np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


# ---- rule 8

class PlaceCase:
    def __init__(self, n, m, k, seed, neg=5):
        rng = np.random.default_rng(seed)
        self.n, self.m, self.k, self.neg = n, m, k, neg
        self.Yfit = (1.0 + np.floor(rng.uniform(0.0, 8.0, (m, 2)) * 1024.0) / 1024.0).astype(np.float32)
        self.idx = np.stack([rng.choice(m, k, replace=False) for _ in range(n)]).astype(np.int32)
        w = np.sort(rng.uniform(0.05, 1.0, (n, k)), axis=1)[:, ::-1]
        self.rate = np.ascontiguousarray(w / w.max(axis=1)[:, None])
        self.y0 = umap.start_numpy(self.Yfit, self.idx.astype(np.int64), w)

    def reference(self, n_epochs, seed=42, row0=0, rows=None):
        rows = slice(None) if rows is None else rows
        return umap.place_numpy(self.y0[rows], self.Yfit, self.idx[rows], self.rate[rows], A, B, n_epochs, 1.0, self.neg, 1.0, seed, row0)


def place_cases():
    out = {"k%d" % k: PlaceCase(2 * ROWS + 1, 80, k, 60 + k) for k in (1, 2, 15, 64, 65)}
    out["m2"] = PlaceCase(ROWS + 1, 2, 2, 70)
    return out
