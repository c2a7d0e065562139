"""Input builders for the k-means kernels' tile, run and screen edges (tests/test_gpu_kmeans_edges.py imports them), and the checks
of the builders themselves: every property a device case relies on is asserted here against float64 numpy, without a GPU.

The integer builders keep points and centres integer-valued, so every float64 distance, member sum and potential is an exact
integer whatever the order of its sum; the expected labels, inertia and sums are then exact, not approximate."""
import functools
import math

import numpy as np
import pytest

from cryo_ralib_amd import kmeans

KM_CAP = 16             # candidates per row the screen lists before it falls back to every centre
KM_SEG = 256            # prefix-sum segment of the search
KM_BLOCK = 1024         # points per block of the member lists
U24 = 2.0 ** -24


def run_len(n):
    """members per run of the cluster sums (km_run_len)"""
    return max(256, (n + 4095) // 4096)


def is_exact(X, C=None):
    """integer-valued, unchanged by the float32 round trip, and every total of squares below 2^53"""
    X = np.asarray(X, np.float64)
    ok = np.array_equal(X, np.rint(X)) and np.array_equal(X.astype(np.float32).astype(np.float64), X)
    amax = np.abs(X).max()
    if C is not None:
        C = np.asarray(C, np.float64)
        ok = ok and np.array_equal(C, np.rint(C)) and np.array_equal(C.astype(np.float32).astype(np.float64), C)
        amax = amax + np.abs(C).max()
    # the largest total any test forms: n distances (or n member entries) of at most d * amax^2 each
    return bool(ok) and float(X.shape[0]) * X.shape[1] * amax * amax < 2.0 ** 53


def exact_dist(X, C):
    """[n][k] float64 |x - c|^2 of integer-valued data from the Gram form: every product and partial sum is an integer below
    2^53, so the result is exact in any order (and equal to the difference form, which the CPU tests check)"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    assert is_exact(X, C)
    return (X * X).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * (X @ C.T)


def diff_dist(X, C):
    """[n][k] float64 |x - c|^2 from differences, in row chunks"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    D = np.empty((X.shape[0], C.shape[0]))
    ch = max(1, (1 << 22) // max(1, C.shape[0] * X.shape[1]))
    for s in range(0, X.shape[0], ch):
        D[s:s + ch] = np.sum((X[s:s + ch, None, :] - C[None, :, :]) ** 2, axis=2)
    return D


def first_min(D):
    """(first index of the row minimum, the minimum)"""
    lab = np.argmin(D, axis=1)
    return lab.astype(np.int32), D[np.arange(D.shape[0]), lab]


# ---- integer ties builder (E-step tiling)

TILING_D = [9, 11, 33, 35, 257, 2047, 2048]
TILING_K = [1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256]
TILING_N = [1, 127, 128, 129, 385]


def tiling_cases():
    """(d, k, n): every k at d = 9 and d = 35, every other d at two values of k, every n; k <= n"""
    cases = []
    for d in (9, 35):
        for i, k in enumerate(TILING_K):
            fits = [n for n in TILING_N if n >= k and n > 1]
            cases.append((d, k, fits[(i + (d == 35)) % len(fits)] if k > 1 else (1 if d == 9 else 129)))
    cases += [(11, 17, 127), (11, 256, 385), (33, 16, 128), (33, 129, 129), (257, 33, 129), (257, 255, 385),
              (2047, 15, 127), (2047, 256, 385), (2048, 1, 1), (2048, 65, 128), (2048, 256, 385)]
    return cases


@functools.lru_cache(maxsize=None)
def ties_case(d, k, n):
    """X float32 [n][d] integers in -20 .. 20, C float64 [k][d] even integers in -20 .. 20; every fifth row is the midpoint of a
    centre and its nearest neighbour (an exact tie unless a third centre is nearer).  Returns X, C, labels (first minimum), the minimum distances"""
    rng = np.random.default_rng(1000 * d + k + n)
    C = 2.0 * rng.integers(-10, 11, (k, d))
    X = rng.integers(-20, 21, (n, d)).astype(np.float32)
    if k >= 2:
        CC = ((C[:, None, :] - C[None, :, :]) ** 2).sum(2) + np.diag(np.full(k, np.inf))
        for i in range(0, n, 5):
            a = int(rng.integers(0, k))
            X[i] = ((C[a] + C[np.argmin(CC[a])]) / 2).astype(np.float32)
    lab, dmin = first_min(exact_dist(X, C))
    return X, C, lab, dmin


# ---- crowded-screen builders

def screen_halfwidth(X, C):
    """[n][k] e = 2 (d + 16) 2^-24 (|x| + |c|)^2: the half-width of the kernel's documented screen bound, from the data"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    s = np.sqrt((X * X).sum(1))[:, None] + np.sqrt((C * C).sum(1))[None, :]
    return 2.0 * (X.shape[1] + 16) * U24 * s * s


@functools.lru_cache(maxsize=None)
def crowded_case(d, m, G=3, n=385):
    """G groups of m centres base_g + (-2 .. 2), base in +-20000; points base_g + (-3 .. 3).  Returns X, C, labels, minimum
    distances, D (exact)"""
    rng = np.random.default_rng(77 * d + m)
    base = rng.integers(-20000, 20001, (G, d)).astype(np.float64)
    C = np.concatenate([base[g] + rng.integers(-2, 3, (m, d)) for g in range(G)])
    X = (base[rng.integers(0, G, n)] + rng.integers(-3, 4, (n, d))).astype(np.float32)
    D = exact_dist(X, C)
    lab, dmin = first_min(D)
    return X, C, lab, dmin, D


@functools.lru_cache(maxsize=None)
def copies_case(d, n=385, k=40, copies=24):
    """k = 40 centres of which 24, at scattered positions, are identical copies of one centre; the others lie around the same two
    bases.  Returns X, C, labels, minimum distances, D, the positions of the copies"""
    rng = np.random.default_rng(91 * d + 5)
    base = rng.integers(-20000, 20001, (2, d)).astype(np.float64)
    C = base[rng.integers(0, 2, k)] + rng.integers(-2, 3, (k, d))
    pos = np.sort(rng.choice(np.arange(1, k), copies, replace=False))          # slot 0 is never a copy: a lower distinct centre
    C[pos] = base[0] + rng.integers(-2, 3, d)
    X = (base[0] + rng.integers(-3, 4, (n, d))).astype(np.float32)            # every row near the copies
    X[::7] = C[pos[0]].astype(np.float32)                                     # rows on the copied centre itself
    D = exact_dist(X, C)
    lab, dmin = first_min(D)
    return X, C, lab, dmin, D, pos


# ---- overflowing norms

BIG = 2.0 ** 70          # finite in float32; its square is not


@functools.lru_cache(maxsize=None)
def overflow_case(d, n0=200, nbig=24):
    """ordinary integer rows and centres mixed with rows and centres that carry +-2^70 entries.  Every large row either equals a
    large centre on all its large entries (its distance is then a small exact integer) or misses one large centre in exactly one
    large entry and every other centre in at least two (distances 2^140 against >= 2^141: far beyond rounding).
    Returns X, C, ordinary (bool [n]), labels and minimum distances from float64 differences"""
    rng = np.random.default_rng(13 * d)
    k0 = 10
    C0 = 2.0 * rng.integers(-10, 11, (k0, d))
    pat = np.zeros((3, d))
    pat[0, [0, 3, 5, 8]] = [BIG, -BIG, BIG, BIG]
    pat[1, [1, 3, 7, d - 1]] = [-BIG, BIG, BIG, -BIG]
    pat[2, [0, 3, 5]] = [BIG, -BIG, BIG]                                   # pattern 0 without its entry 8
    # two centres share pattern 0 and differ in small entries only: small exact integers decide between them
    Cb = np.stack([pat[0], pat[0], pat[1], pat[2]])
    small = (Cb == 0)
    Cb = Cb + small * 2.0 * rng.integers(-10, 11, Cb.shape)
    C = np.concatenate([C0[:4], Cb[:2], C0[4:8], Cb[2:], C0[8:]])
    X0 = rng.integers(-20, 21, (n0, d)).astype(np.float64)
    which = rng.integers(0, 4, nbig)
    Xb = Cb[which] + (Cb[which] != pat[[0, 0, 1, 2]][which]) * rng.integers(-3, 4, (nbig, d))
    # rows of pattern 2 that also carry pattern 0's entry 8 negated: one large miss against pattern 2, two or more elsewhere
    odd = np.nonzero(which == 3)[0][::2]
    Xb[odd, 8] = -BIG
    X = np.concatenate([X0, Xb])
    ordinary = np.concatenate([np.ones(n0, bool), np.zeros(nbig, bool)])
    perm = rng.permutation(n0 + nbig)
    X, ordinary = X[perm].astype(np.float32), ordinary[perm]
    lab, dmin = first_min(diff_dist(X, C))
    return X, C, ordinary, lab, dmin


# ---- count-controlled builder (cluster sums)

MULTS = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1025)
MULTS_SHORT = (1, 4, 255, 257, 513)
MULTS_LONG_RUN = (257999, 258000, 258001, 3, 278670)       # n = 1 052 673: runs of 258; counts one under, on and over a multiple


def separated_centres(rng, k, d):
    """k distinct centres with entries in 6 * (-3 .. 3).  For a point x = c_j + delta with delta in {-1, 0, 1}^d and another centre
    c_l = c_j - D, |x - c_l|^2 - |x - c_j|^2 = |D|^2 + 2 delta.D >= sum_t (D_t^2 - 2 |D_t|) > 0, since every nonzero |D_t| >= 6:
    the nearest centre of such a point is c_j, strictly"""
    while True:
        C = 6.0 * rng.integers(-3, 4, (k, d))
        if len(np.unique(C, axis=0)) == k:
            return C


@functools.lru_cache(maxsize=None)
def counted_case(d, mults, seed=0):
    """k = len(mults) separated centres, mults[j] points c_j + (-1 .. 1) each, rows shuffled.  Returns X, C, the planted labels"""
    rng = np.random.default_rng(31 * d + len(mults) + seed)
    k = len(mults)
    C = separated_centres(rng, k, d)
    lab = np.repeat(np.arange(k), mults)
    rng.shuffle(lab)
    X = (C[lab] + rng.integers(-1, 2, (lab.size, d))).astype(np.float32)
    return X, C, lab.astype(np.int32)


@functools.lru_cache(maxsize=None)
def real_case(d=257, counts=(300, 1000)):
    """standard_normal rows around two planted centres +-4: X float32, C, the planted labels"""
    rng = np.random.default_rng(257)
    C = np.stack([np.full(d, 4.0), np.full(d, -4.0)])
    lab = np.repeat(np.arange(2), counts)
    rng.shuffle(lab)
    X = (C[lab] + rng.standard_normal((lab.size, d))).astype(np.float32)
    return X, C, lab.astype(np.int32)


def real_centre_reference(X, lab, k):
    """(centres in longdouble from math.fsum, the bound per entry (L + runs + 2) 2^-53 sum_members |x_t| / count).  The device adds a
    run's members one by one (at most L - 1 roundings of partial sums bounded by sum |x_t|), then the runs (runs - 1 roundings),
    then forms sum * (1 / weight) (two roundings): below (L + runs + 2) u sum |x_t| / count with u = 2^-53"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    L = run_len(n)
    ref = np.zeros((k, d), np.longdouble)
    bound = np.zeros((k, d))
    for j in range(k):
        M = X[lab == j]
        cnt = M.shape[0]
        runs = (cnt + L - 1) // L
        for t in range(d):
            ref[j, t] = np.longdouble(math.fsum(M[:, t])) / cnt
            bound[j, t] = (L + runs + 2) * 2.0 ** -53 * math.fsum(np.abs(M[:, t])) / cnt
    return ref, bound


# ---- relocation builders

def _far_delta(rng, d, sq):
    """a vector of sq entries +-1, the rest 0"""
    v = np.zeros(d)
    v[rng.choice(d, sq, replace=False)] = rng.choice([-1.0, 1.0], sq)
    return v


class Relocation:
    """X float32 [n][d], C float64 [k][d] (the init), labels (planned E-step result), empty (ids of the empty clusters), far (the
    rows that must be relocated, in order), counts_before / counts_after [k] (planned), heavy (the heaviest cluster after
    relocation), emptied (the donor left without members, or None)"""


@functools.lru_cache(maxsize=None)
def relocation_case(d, e, variant, heavy_low=True):
    """k = 6 live clusters and e empty ones whose init centres lie far from every point.

    variant "spread":  three rows at squared distance 3 and four at squared distance 2 from their centres, every other row at most 1;
                       two of the distance-3 rows belong to the same cluster.  The e farthest are the distance-3 rows by index,
                       then the distance-2 rows by index.
    variant "emptied": as "spread", but the two lowest-index distance-3 rows are the only members of one cluster, which the
                       relocation leaves with weight 0 (e >= 2); heavy_low places the heaviest cluster below or above it.
    variant "onpoint": every row equals its centre: nothing is relocated, the empty clusters copy the heaviest one."""
    assert variant in ("spread", "emptied", "onpoint") and d >= 3 and 1 <= e <= 5
    rng = np.random.default_rng(100 * d + 10 * e + len(variant) + int(heavy_low))
    live = 6
    k = live + e
    # empty ids on both sides of the live ones
    empty = np.sort(rng.choice(k, e, replace=False)) if variant != "onpoint" else np.array([0, k - 1][:e])
    ids = np.array([j for j in range(k) if j not in set(empty.tolist())])
    Cl = separated_centres(rng, live, d)
    sizes = np.array([40, 55, 30, 45, 35, 50])
    if variant == "emptied":
        assert e >= 2
        sizes[2] = 2                                    # live cluster 2 is the donor that ends empty
        hv = 0 if heavy_low else live - 1
        sizes[hv] = 90
    lab_l = np.repeat(np.arange(live), sizes)
    rng.shuffle(lab_l)
    n = lab_l.size
    delta = np.zeros((n, d))
    if variant != "onpoint":
        near = rng.integers(0, d + 1, n)                # one entry +-1, or none
        for i in np.nonzero(near < d)[0]:
            delta[i, near[i]] = rng.choice([-1.0, 1.0])
        if variant == "emptied":
            # the donor's two rows come first in index order among the distance-3 rows
            two = np.nonzero(lab_l == 2)[0]
            other = np.nonzero(lab_l != 2)[0]
            third = other[other > two.max()]
            if third.size == 0:                          # move the donor's rows to the front
                swap = other[:2]
                lab_l[two], lab_l[swap] = lab_l[swap], 2
                two, other = np.nonzero(lab_l == 2)[0], np.nonzero(lab_l != 2)[0]
                third = other[other > two.max()]
            d3 = np.concatenate([two, third[:1]])
            rest = np.setdiff1d(other, d3)
        else:
            big = np.nonzero(lab_l == 1)[0]
            d3 = np.concatenate([big[:2], np.nonzero(lab_l == 4)[0][-1:]])         # two donors from cluster 1, the lowest indices
            assert d3[2] > d3[1]
            rest = np.setdiff1d(np.arange(n), d3)
        d2 = rng.choice(rest, 4, replace=False)
        while True:                                      # distinct rows among the farthest, so a test can tell which one moved
            for i in d3:
                delta[i] = _far_delta(rng, d, 3)
            for i in d2:
                delta[i] = _far_delta(rng, d, 2)
            fr = np.concatenate([d3, d2])
            if len(np.unique(Cl[lab_l[fr]] + delta[fr], axis=0)) == len(fr):
                break
    r = Relocation()
    r.C = np.empty((k, d))
    r.C[ids] = Cl
    r.C[empty] = 60.0 + 2.0 * np.arange(e)[:, None]     # even, beyond every point (|x| <= 19)
    r.labels = ids[lab_l].astype(np.int32)
    r.X = (Cl[lab_l] + delta).astype(np.float32)
    r.empty = empty
    r.counts_before = np.bincount(r.labels, minlength=k)
    r.counts_after = r.counts_before.copy()
    if variant == "onpoint":
        r.far = np.zeros(0, np.int64)
    else:
        sq = (delta * delta).sum(1)
        r.far = np.lexsort((np.arange(n), -sq))[:e]
        for nw, f in zip(empty, r.far):
            r.counts_after[nw] += 1
            r.counts_after[r.labels[f]] -= 1
    r.heavy = int(np.argmax(r.counts_after))
    r.emptied = int(ids[2]) if variant == "emptied" else None
    return r


RELOCATION_CASES = [("spread", 1, True), ("spread", 2, True), ("spread", 5, True), ("emptied", 2, True), ("emptied", 2, False),
                    ("emptied", 5, True), ("emptied", 5, False), ("onpoint", 2, True)]


def expected_update(r):
    """the centres sklearn's _average_centers forms from the planned relocation, in float64 with exact integer sums"""
    k, d = r.C.shape
    X = r.X.astype(np.float64)
    sums = np.zeros((k, d))
    np.add.at(sums, r.labels, X)
    for nw, f in zip(r.empty, r.far):
        sums[r.labels[f]] -= X[f]
        sums[nw] = X[f]
    Cn = sums.copy()
    for j in range(k):
        if r.counts_after[j] > 0:
            Cn[j] *= 1.0 / r.counts_after[j]
        else:
            Cn[j] = Cn[r.heavy]
    return Cn


# ---- search builder

@functools.lru_cache(maxsize=None)
def search_case(n):
    """integer weights 0 .. 4 with a zero plateau, and 16 values: on a cumulative entry, between two entries, 0, the total, above
    it, on the last element of a 256-segment and just past it (the first element of the next), around the plateau.
    Returns w float64 [n], vals float64 [16], the reference indices, and the hand-placed (value, index) pairs"""
    rng = np.random.default_rng(n)
    w = rng.integers(0, 5, n).astype(np.float64)
    w[0] = 3.0
    p0 = n // 3
    p1 = p0 + min(300, max(1, n // 4))
    if n >= 3:
        w[p0:p1] = 0.0                                  # up to 300 zeros: across a segment boundary when n allows
        w[p0 - 1] = 1.0
        if p1 < n:
            w[p1] = 2.0
    placed = [(0.0, 0)]
    for b in (KM_SEG, KM_SEG * KM_SEG):                 # the end of segment 0 and of segment 255 (the last one of the scan's first pass)
        if n > b and not (p0 - 1 <= b - 1 <= p1):
            w[b - 1], w[b] = 1.0, 2.0
    cum = np.cumsum(w)
    total = cum[-1]
    for b in (KM_SEG, KM_SEG * KM_SEG):
        if n > b and not (p0 - 1 <= b - 1 <= p1):
            placed += [(cum[b - 1], b - 1), (cum[b - 1] + 0.5, b), (cum[b - 1] + 2.0, b)]
    if n >= 3:
        placed += [(cum[p0 - 1], p0 - 1)]               # on the entry the plateau repeats: the first of the equal entries
        if p1 < n:
            placed += [(cum[p0 - 1] + 1.0, p1)]         # past the plateau
    last = int(np.nonzero(w)[0][-1])
    placed += [(total, last), (total + 1.0, n - 1), (total - 0.5, last)]
    vals = [v for v, _ in placed]
    while len(vals) < 16:
        j = int(rng.integers(0, n))
        vals.append(cum[j] - (0.5 if len(vals) % 2 else 0.0))
    vals = np.array(vals[:16])
    ref = np.minimum(np.searchsorted(cum, vals), n - 1).astype(np.int32)
    return w, vals, ref, placed[:16]


SEARCH_N = [1, 255, 256, 257, 65536, 65537, 400000]


# ---- seed builder

SEED_SHAPES = [(1, 1), (1, 2048), (257, 8), (257, 9), (257, 2048), (65537, 1), (65537, 9), (70000, 8), (70000, 9)]


@functools.lru_cache(maxsize=None)
def seed_case(n, d):
    """integer rows in -20 .. 20 whose last row repeats row 0, a first centre, and candidate lists of 1, 2 and 16 rows for the later
    steps: the 2-list holds two distinct rows of equal potential (the copy before the original), the 16-list holds duplicates"""
    rng = np.random.default_rng(3 * n + d)
    X = rng.integers(-20, 21, (n, d)).astype(np.float32)
    X[n - 1] = X[0]
    first = int(rng.integers(0, n))
    c16 = rng.integers(0, n, 16)
    c16[5], c16[11] = c16[2], c16[2]
    c16[15], c16[7] = n - 1, 0
    lists = [np.array([int(rng.integers(0, n))]), np.array([n - 1, 0]), c16]
    return X, first, [np.asarray(c, np.int32) for c in lists]


def seed_reference(X, first, lists):
    """the steps in float64: [(chosen, its potential, all potentials, closest after the step)] for the first centre, then each list"""
    X = np.asarray(X, np.float64)
    out = []
    closest = np.sum((X - X[first]) ** 2, axis=1)
    out.append((first, closest.sum(), np.array([closest.sum()]), closest.copy()))
    for cand in lists:
        D = np.minimum(closest[None, :], np.stack([np.sum((X - X[c]) ** 2, axis=1) for c in cand]))
        pots = D.sum(axis=1)
        best = int(np.argmin(pots))
        closest = D[best]
        out.append((int(cand[best]), pots[best], pots, closest.copy()))
    return out


@functools.lru_cache(maxsize=None)
def plusplus_case(n=70000, d=9):
    rng = np.random.default_rng(70)
    return rng.integers(-20, 21, (n, d)).astype(np.float32)


# ---- the builders' own properties

@pytest.mark.parametrize("d,k,n", [(9, 17, 127), (35, 33, 385), (257, 33, 129)])
def test_gram_distances_equal_difference_distances(d, k, n):
    X, C, lab, dmin = ties_case(d, k, n)
    D = diff_dist(X, C)
    assert np.array_equal(D, exact_dist(X, C)) and np.array_equal(D, np.rint(D))
    assert np.array_equal(lab, np.argmin(D, axis=1))


@pytest.mark.parametrize("d,k,n", tiling_cases())
def test_ties_builder_is_exact_and_has_ties(d, k, n):
    X, C, lab, dmin = ties_case(d, k, n)
    assert X.dtype == np.float32 and X.shape == (n, d) and C.shape == (k, d) and k <= n
    assert is_exact(X, C) and np.abs(X).max() <= 20 and np.abs(C).max() <= 20 and np.all(C % 2 == 0)
    D = exact_dist(X, C)
    assert np.array_equal(D, np.rint(D)) and float(np.sum(dmin)) < 2.0 ** 53
    ties = np.sum(D == dmin[:, None], axis=1) > 1
    if k >= 2 and n >= 100:
        assert ties.sum() >= n // 10, (ties.sum(), n)
    # the lowest index among equal minima is the label
    assert np.array_equal(lab, np.array([np.nonzero(D[i] == dmin[i])[0][0] for i in range(n)]))
    nl, inertia = kmeans.labels_for(X, C, backend="numpy")
    assert np.array_equal(nl, lab) and inertia == float(np.sum(dmin))


def test_tiling_cases_cover_the_issue():
    cases = tiling_cases()
    for d in (9, 35):
        assert sorted(k for dd, k, n in cases if dd == d) == TILING_K
    for d in TILING_D:
        assert len({k for dd, k, n in cases if dd == d}) >= 2
    assert {n for d, k, n in cases} == set(TILING_N)


@pytest.mark.parametrize("d", [9, 35, 128])
@pytest.mark.parametrize("m", [16, 17, 20])
def test_crowded_builder_fills_the_screen(d, m):
    X, C, lab, dmin, D = crowded_case(d, m)
    assert is_exact(X, C) and np.array_equal(D, np.rint(D)) and C.shape[0] == 3 * m
    within = D - dmin[:, None] <= screen_halfwidth(X, C)
    assert within.sum(1).min() >= m, within.sum(1).min()
    # the group's spread is of the size of float32's spacing at |x|^2, far inside the half-width
    nearest_m = np.sort(D, axis=1)[:, m - 1] - dmin
    assert nearest_m.max() <= 25 * d and nearest_m.max() < screen_halfwidth(X, C).min()
    eq = D == dmin[:, None]
    assert np.array_equal(lab, np.argmax(eq, axis=1))         # unique, or the lowest index of an exact tie
    print("d %d m %d: %d exact ties, spread %g" % (d, m, int(np.sum(eq.sum(1) > 1)), nearest_m.max()))


@pytest.mark.parametrize("d", [9, 35, 128])
def test_copies_builder(d):
    X, C, lab, dmin, D, pos = copies_case(d)
    assert is_exact(X, C) and C.shape[0] == 40 and len(pos) == 24 and np.all(C[pos] == C[pos[0]])
    assert len(np.unique(C, axis=0)) == 40 - 24 + 1
    within = D - dmin[:, None] <= screen_halfwidth(X, C)
    assert within.sum(1).min() >= 24
    won = np.isin(lab, pos)
    assert won.sum() >= X.shape[0] // 7 and np.all(lab[won] == pos[0])       # the lowest copy wins
    assert np.all(np.sum(D[won] == dmin[won, None], axis=1) >= 24)


@pytest.mark.parametrize("d", [12, 40])
def test_overflow_builder(d):
    X, C, ordinary, lab, dmin = overflow_case(d)
    assert X.dtype == np.float32 and np.all(np.isfinite(X)) and np.all(np.isfinite(C.astype(np.float32)))
    with np.errstate(over="ignore"):
        nx = (X * X).sum(1, dtype=np.float32)
        nc = (C.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    assert np.all(np.isinf(nx[~ordinary])) and np.all(np.isfinite(nx[ordinary])) and np.isinf(nc).sum() == 4
    D = diff_dist(X, C)
    srt = np.sort(D, axis=1)
    # the winner is unique with a margin no rounding reaches, or decided by exact small integers
    small = dmin < 2.0 ** 52
    assert np.all(dmin[small] == np.rint(dmin[small])) and np.all(ordinary <= small)
    assert np.all((srt[:, 1] > srt[:, 0]) | small)
    assert np.all(srt[~small, 1] >= 1.9 * srt[~small, 0]) and (~small).sum() >= 2
    big_c = np.nonzero(np.isinf(nc))[0]
    assert np.all(np.isin(lab[~ordinary], big_c)) and not np.any(np.isin(lab[ordinary], big_c))
    assert len(np.unique(lab[~ordinary])) >= 3
    # the ordinary rows alone give the same labels and distances
    l0, d0 = first_min(diff_dist(X[ordinary], C))
    assert np.array_equal(l0, lab[ordinary]) and np.array_equal(d0, dmin[ordinary])
    nl, _ = kmeans.labels_for(X, C, backend="numpy")
    assert np.array_equal(nl, lab)


@pytest.mark.parametrize("d,mults", [(9, MULTS), (255, MULTS), (256, MULTS), (257, MULTS), (513, MULTS), (2048, MULTS_SHORT)])
def test_counted_builder(d, mults):
    X, C, lab = counted_case(d, mults)
    assert is_exact(X, C) and np.abs(X).max() <= 20 and np.all(C % 2 == 0)
    assert np.array_equal(np.bincount(lab), mults)
    B = kmeans._Numpy(X)
    nl, dist = B.assign(C)
    assert np.array_equal(nl, lab) and dist.max() <= d
    # several blocks of the member lists hold members of the large clusters
    if len(lab) > KM_BLOCK:
        big = int(np.argmax(mults))
        assert len({i // KM_BLOCK for i in np.nonzero(lab == big)[0]}) >= 2
    assert run_len(len(lab)) == 256
    if mults == MULTS:
        assert {m % 4 for m in mults} == {0, 1, 2, 3} and {255, 256, 257} <= set(mults)


def test_counted_builder_long_runs():
    X, C, lab = counted_case(9, MULTS_LONG_RUN)
    n = len(lab)
    assert n == 1052673 and run_len(n) == 258 and is_exact(X, C)
    assert [m % 258 for m in MULTS_LONG_RUN[:3]] == [257, 0, 1]
    nl, dist = kmeans._Numpy(X).assign(C)
    assert np.array_equal(nl, lab)


def test_real_builder_labels_are_unambiguous():
    X, C, lab = real_case()
    D = diff_dist(X, C)
    assert np.array_equal(np.argmin(D, axis=1), lab) and np.abs(D[:, 0] - D[:, 1]).min() > 1000
    assert np.array_equal(np.bincount(lab), (300, 1000))
    Cn, _, _ = kmeans._Numpy(X).lloyd(C)
    ref, bound = real_centre_reference(X, lab, 2)
    # numpy's member-by-member sums sit inside their own bound, (count + 2) u sum |x_t| / count, around the same reference
    cnt = np.bincount(lab)[:, None]
    assert np.all(np.abs(Cn.astype(np.longdouble) - ref) <= bound * (cnt + 2) / ((cnt + 255) // 256 + 258))


@pytest.mark.parametrize("d", [3, 40])
@pytest.mark.parametrize("variant,e,heavy_low", RELOCATION_CASES)
def test_relocation_builder_scenarios_occur(d, variant, e, heavy_low):
    r = relocation_case(d, e, variant, heavy_low)
    k = r.C.shape[0]
    assert is_exact(r.X, r.C) and k == 6 + e and np.all(r.C % 2 == 0)
    B = kmeans._Numpy(r.X)
    lab, dist = B.assign(r.C)
    assert np.array_equal(lab, r.labels)
    cb = np.bincount(lab, minlength=k)
    assert np.array_equal(cb, r.counts_before) and np.array_equal(np.nonzero(cb == 0)[0], r.empty)
    Cn, shift, changed = B.lloyd(r.C)
    assert changed == len(lab)
    if variant == "onpoint":
        assert dist.max() == 0 and len(r.far) == 0 and np.array_equal(r.counts_after, r.counts_before)
        assert r.empty[0] < r.heavy < r.empty[1]                   # one copy of an averaged centre, one of a plain sum
        assert np.array_equal(Cn[r.empty[1]], Cn[r.heavy]) and np.array_equal(Cn[r.empty[0]], r.C[r.heavy] * cb[r.heavy])
        assert not np.array_equal(Cn[r.empty[0]], Cn[r.empty[1]])
    else:
        # equal distances among the farthest: the tie rule decides
        order = np.lexsort((np.arange(len(lab)), -dist))
        assert np.array_equal(order[:e], r.far)
        assert dist[order[0]] == 3 and np.sum(dist == 3) == 3 and np.sum(dist == 2) == 4 and np.sum(dist > 3) == 0
        assert dist[order[e]] == dist[order[e - 1]]                # the cut falls inside a group of equal distances
        # the rows relocated are the planned ones: each empty cluster's new centre is its row (rows are distinct)
        Xf = r.X[r.far].astype(np.float64)
        assert len(np.unique(Xf, axis=0)) == e
        assert np.array_equal(Cn[r.empty], Xf)
        if variant == "spread":
            donors = lab[r.far]
            assert e < 2 or donors[0] == donors[1]                 # two donors from the same cluster
            assert r.counts_after.min() >= 1
    assert np.array_equal(Cn, expected_update(r))
    if variant == "emptied":
        assert r.counts_before[r.emptied] == 2 and r.counts_after[r.emptied] == 0 and np.sum(r.counts_after == 0) == 1
        assert (r.heavy < r.emptied) == heavy_low
        X = r.X.astype(np.float64)
        hs = X[(lab == r.heavy)].sum(0)
        for f in r.far:
            if lab[f] == r.heavy:
                hs -= X[f]
        want = hs * (1.0 / r.counts_after[r.heavy]) if heavy_low else hs
        assert np.array_equal(Cn[r.emptied], want)
        assert heavy_low or not np.array_equal(Cn[r.emptied], Cn[r.heavy])


@pytest.mark.parametrize("n", SEARCH_N)
def test_search_builder(n):
    w, vals, ref, placed = search_case(n)
    assert np.array_equal(w, np.rint(w)) and w.min() >= 0 and w.max() <= 4 and w.sum() > 0 and len(vals) == 16
    cum = np.cumsum(w)
    for (v, idx), r in zip(placed, ref):
        assert r == idx, (n, v, idx, r)
    assert ref[0] == 0 and (n - 1) in ref
    if n >= 3:
        z = np.nonzero(w == 0)[0]
        assert z.size >= min(300, max(1, n // 4))                  # the plateau
    if n > KM_SEG:
        assert KM_SEG - 1 in ref and KM_SEG in ref
    if n > KM_SEG * KM_SEG:
        assert KM_SEG * KM_SEG - 1 in ref and KM_SEG * KM_SEG in ref
    if n == 400000:
        p0 = n // 3
        assert (p0 - 1) // KM_SEG != (p0 + 299) // KM_SEG          # the plateau crosses a segment boundary
    B = kmeans._Numpy(np.zeros((n, 1)))
    B.closest = w
    assert np.array_equal(B.search(vals), ref)
    # side left: on an entry exactly, the entry itself; just above, the next non-zero weight
    on = [i for i, v in enumerate(vals) if v in cum]
    assert len(on) >= 2
    for i in on:
        assert cum[ref[i]] == vals[i] and (ref[i] == 0 or cum[ref[i] - 1] < vals[i])


@pytest.mark.parametrize("n,d", SEED_SHAPES)
def test_seed_builder(n, d):
    X, first, lists = seed_case(n, d)
    assert is_exact(X) and [len(c) for c in lists] == [1, 2, 16]
    steps = seed_reference(X, first, lists)
    for chosen, pot, pots, closest in steps:
        assert np.array_equal(closest, np.rint(closest)) and pot == closest.sum() and pot < 2.0 ** 53
    # the 2-list: equal potentials, the first candidate (the copy, row n - 1) wins
    assert steps[2][2][0] == steps[2][2][1] and steps[2][0] == n - 1
    assert len(np.unique(lists[2])) < 16 or n == 1
    # the numpy backend walks the same steps
    B = kmeans._Numpy(X)
    got = [B.seed([first], True)] + [B.seed(c, False) for c in lists]
    assert [(int(a), float(b)) for a, b in got] == [(s[0], float(s[1])) for s in steps]
    assert np.array_equal(B.closest, steps[-1][3])


def test_plusplus_builder():
    X = plusplus_case()
    assert is_exact(X) and X.shape == (70000, 9)
    idx = kmeans._plusplus(kmeans._Numpy(X), 8, np.random.RandomState(11))
    assert len(idx) == 8 and kmeans.n_local_trials(8) == 4
