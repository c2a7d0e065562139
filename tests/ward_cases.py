"""What the Ward suites (tests/test_ward_cpu.py, tests/test_gpu_ward.py) and tests/golden/make_ward_pins.py share: the data
generators, the cluster-table states of the entry-by-entry kernel tests, and the comparison up to a renaming of labels."""
import numpy as np

MARGIN = 1e-9               # the least row-wise margin and height gap a builder may have (ward.py rule 8)
PIN_NAMES = ("gauss2", "gauss5", "blobs50", "islands", "two", "three")
PIN_KS = (2, 5, 17)


def gaussian(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def blobs(n, d, centers, seed, spread=1.0, box=10.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-box, box, (centers, d))
    which = rng.integers(0, centers, n)
    return (c[which] + spread * rng.normal(size=(n, d))).astype(np.float32)


def islands(n, seed):
    """three Gaussian islands of spread 0.3, 1.0 and 0.1 plus 10 % uniform scatter (the generator of the HDBSCAN pins, without its
    quantisation to a grid: equal distances are ties)"""
    rng = np.random.default_rng(seed)
    ns = n // 10
    m = n - ns
    sizes = [m // 2, m // 3, m - m // 2 - m // 3]
    centres, sig = np.array([[-5.0, -2.0], [4.0, 3.0], [2.0, -6.0]]), (0.3, 1.0, 0.1)
    parts = [centres[j] + sig[j] * rng.normal(size=(sizes[j], 2)) for j in range(3)]
    parts.append(rng.uniform(-10.0, 10.0, (ns, 2)))
    return np.concatenate(parts)[rng.permutation(n)].astype(np.float32)


def pin_inputs():
    """name -> X of the pins of tests/golden/ward_ref.npz"""
    return {"gauss2": gaussian(300, 2, 11), "gauss5": gaussian(1000, 5, 12), "blobs50": blobs(600, 50, 8, 13),
            "islands": islands(2500, 14), "two": gaussian(2, 3, 15), "three": gaussian(3, 2, 16)}


def line(n, seed=0):
    """points on a line, in order, with gaps that grow by 1 % of the first per step (jittered by a fifth of that): every point's
    nearest neighbour is the one before it, so round 0 has the one reciprocal pair (0, 1) and the front of new pairs then moves
    two points per round: about n / 2 rounds, the adversarial chain of the rounds"""
    rng = np.random.default_rng(seed)
    gaps = 1.0 + 0.01 * np.arange(n) + rng.uniform(-0.002, 0.002, n)
    return np.cumsum(gaps)[:, None].astype(np.float32)


def duplicates(seed=21):
    """three copies each of 25 separated points, shuffled: (X [75][3], group [75])"""
    rng = np.random.default_rng(seed)
    base = (rng.permutation(25)[:, None] * 8.0 + rng.uniform(-1.0, 1.0, (25, 3))).astype(np.float32)
    perm = rng.permutation(75)
    return np.repeat(base, 3, axis=0)[perm], np.repeat(np.arange(25), 3)[perm]


def identical(n=70, d=3):
    return np.full((n, d), 1.25, np.float32)


DEAD_PATTERNS = ("none", "alternate", "run", "all_but_two", "sizes")


def table(n, d, dead, seed):
    """a cluster table (C float64 [n][d], size int32 [n]) for the kernel tests: Gaussian centroids, and the slots dead (size 0)
    by pattern: none; every other slot; a run straddling the column-tile boundary at 64 (or the middle of a smaller table); all
    but two; none, with sizes mixed between 1 and 5000"""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(n, d))
    size = np.ones(n, np.int32)
    if dead == "alternate":
        size[1::2] = 0
    elif dead == "run":
        mid = 64 if n > 70 else n // 2
        size[max(0, mid - 5):min(n, mid + 6)] = 0
    elif dead == "all_but_two":
        size[:] = 0
        size[rng.choice(n, 2, replace=False)] = (3, 7)
    elif dead == "sizes":
        size[:] = rng.integers(1, 5001, n)
    elif dead != "none":
        raise ValueError(dead)
    if np.count_nonzero(size) < 2 and n >= 2:           # a table needs two live clusters for a candidate
        size[:2] = 1
    return C, size


def row_list(n, n_rows, seed):
    """n_rows slots of 0 .. n - 1 in no order, with repeats (always, once n_rows > 1), and the first one twice"""
    rows = np.random.default_rng(seed).integers(0, n, n_rows).astype(np.int32)
    if n_rows > 1:
        rows[-1] = rows[0]
    return rows


def same_partition(a, b):
    """labels a and b describe one partition (equal up to a renaming)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape != b.shape:
        return False
    ka, kb = int(a.max()) + 1, int(b.max()) + 1
    pairs = np.unique(a * kb + b)
    return ka == kb and len(pairs) == ka and len(np.unique(pairs // kb)) == ka and len(np.unique(pairs % kb)) == kb


def inertia_direct(X, labels):
    """the within-class sum of squares of the labels, straight from the data"""
    X = np.asarray(X, np.float64)
    tot = 0.0
    for c in range(int(labels.max()) + 1):
        P = X[labels == c]
        tot += float(((P - P.mean(axis=0)) ** 2).sum())
    return tot
