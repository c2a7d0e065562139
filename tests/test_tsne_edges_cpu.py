"""Input builders and float64 references for the t-SNE kernels' list, lane and segment edges (tests/test_gpu_tsne_edges.py imports
them), and the checks of the builders themselves: every property a device case relies on is asserted here, without a GPU.

Exact cases (integer coordinates, counted embeddings) are built so that every float32 and float64 value the kernels form is
exact; their expected results are compared for equality.  Toleranced cases carry a bound computed here from term counts and the
magnitudes of the float64 reference, never from a device result."""
import functools
import math

import numpy as np
import pytest

from cryo_ralib_amd import tsne

U24 = 2.0 ** -24        # float32 unit roundoff
U53 = 2.0 ** -53        # float64 unit roundoff
KNN_TILE, KNN_MARGIN, KNN_SLACK = 64, 32, 256
REP_ROWS, REP_MAXSEG = 1024, 64


def segment(n):
    """tsne_segment: columns per repulsion segment"""
    per = (n + REP_MAXSEG * REP_ROWS - 1) // (REP_MAXSEG * REP_ROWS)
    return REP_ROWS * max(per, 1)


def knn_plan(n, k):
    """(C survivors, cap list capacity) of tsne_knn_kernel"""
    C = min(n - 1, k + KNN_MARGIN)
    return C, C + KNN_SLACK


# ---- 1. kNN, exact

def brute_knn(X, k):
    """(idx [n][k] int64, dist2 [n][k]) by float64 differences over all pairs and np.lexsort((index, distance)) per row"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    idx = np.empty((n, k), np.int64)
    d2 = np.empty((n, k))
    ar = np.arange(n)
    for i in range(n):
        D = np.sum((X[i] - X) ** 2, axis=1)
        D[i] = np.inf
        o = np.lexsort((ar, D))[:k]
        idx[i], d2[i] = o, D[o]
    return idx, d2


def all_dist(X):
    X = np.asarray(X, np.float64)
    return np.stack([np.sum((X[i] - X) ** 2, axis=1) for i in range(X.shape[0])])


def gram_exact(X):
    """integer coordinates, unchanged by float32, and every value of |x_i|^2 + |x_j|^2 - 2 x_i.x_j (partial sums included)
    below 2^24: the float32 Gram distances and the double distances are exact"""
    X64 = np.asarray(X, np.float64)
    ok = np.asarray(X).dtype == np.float32 and np.array_equal(X64, np.rint(X64))
    return bool(ok) and 4.0 * float(np.max(np.sum(X64 * X64, axis=1))) < 2.0 ** 24


LINE_N = [2, 3, 16, 17, 63, 64, 65, 124, 125, 257, 700, 1100]
LINE_CASES = [(n, k) for n in LINE_N for k in (1, 5, 91) if k <= n - 1] + [(n, 301) for n in (302, 334, 335, 1100)]


def line_points(n, reverse):
    j = np.arange(n, dtype=np.float32)
    return (n - 1 - j if reverse else j).reshape(n, 1)


@functools.lru_cache(maxsize=None)
def line_case(n, k, reverse):
    X = line_points(n, reverse)
    return (X,) + brute_knn(X, k)


@functools.lru_cache(maxsize=None)
def identical_case(n=700, d=3, k=91):
    X = np.tile(np.array([3.0, -1.0, 2.0], np.float32)[:d], (n, 1))
    return (X,) + brute_knn(X, k)


@functools.lru_cache(maxsize=None)
def grid_case(k, side=32):
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)
    X = g[np.random.default_rng(32).permutation(side * side)].astype(np.float32)
    return (X,) + brute_knn(X, k)


FEATURE_D = [1, 2, 3, 4, 5, 7, 8, 50, 625, 2047, 2048]


@functools.lru_cache(maxsize=None)
def feature_case(d, n=130, k=31):
    X = np.random.default_rng(d).integers(-2, 3, (n, d)).astype(np.float32)
    return (X,) + brute_knn(X, k)


def stream_trace(Drow, i, C, cap):
    """the kernel's streaming list of one row on screen distances Drow: (entries held at the first compaction, compactions in
    the tile loop, candidates accepted after the first compaction)"""
    n = len(Drow)
    lst, full, td, first, ncomp, after = [], False, np.inf, None, 0, 0
    for j0 in range(0, n, KNN_TILE):
        for j in range(j0, min(n, j0 + KNN_TILE)):
            if j != i and (not full or Drow[j] < td):
                lst.append((Drow[j], j))
                after += full
        if len(lst) > cap - KNN_TILE:
            first = len(lst) if first is None else first
            lst = sorted(lst)[:C]
            td, full, ncomp = lst[-1][0], True, ncomp + 1
    return first, ncomp, after


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n,k", LINE_CASES)
def test_line_builder(n, k, reverse):
    X, idx, d2 = line_case(n, k, reverse)
    assert gram_exact(X) and X.shape == (n, 1)
    assert np.all(np.diff(d2, axis=1) >= 0) and not np.any(idx == np.arange(n)[:, None])
    # neighbours at i - m and i + m tie and come in index order
    D = np.sort(all_dist(X) + np.diag(np.full(n, np.inf)), axis=1)
    ties = int(np.sum(D[:, k - 1] == D[:, k])) if k < n - 1 else 0
    assert ties == max(0, n - k - 1)                    # k is odd: every row with (k + 1) / 2 points on either side
    same = d2[:, 1:] == d2[:, :-1]
    assert np.all(idx[:, 1:][same] > idx[:, :-1][same])
    if n >= 700:
        assert 4 * ties >= n
        C, cap = knn_plan(n, k)
        Dm = all_dist(X)
        if reverse:
            # the last rows see ever closer candidates: every tile is appended and the list compacts again and again
            first, ncomp, after = stream_trace(Dm[n - 1], n - 1, C, cap)
            assert first > cap - KNN_TILE and ncomp >= 2 and after == n - 1 - first
        else:
            # row 0 sees ever farther candidates: nothing is accepted once the list is full
            first, ncomp, after = stream_trace(Dm[0], 0, C, cap)
            assert first > cap - KNN_TILE and ncomp == 1 and after == 0


def test_line_cases_straddle_the_survivor_cap():
    assert knn_plan(124, 91)[0] == 123 == 91 + 32 and knn_plan(125, 91)[0] == 123 < 124      # n - 1 = k + 32, then above it
    assert knn_plan(334, 301)[0] == 333 and knn_plan(335, 301)[0] == 333 and knn_plan(302, 301)[0] == 301
    assert (2, 1) in LINE_CASES and (1100, 301) in LINE_CASES and (63, 91) not in LINE_CASES


def test_identical_points_builder():
    X, idx, d2 = identical_case()
    assert gram_exact(X) and X.shape == (700, 3) and np.all(d2 == 0.0)
    for i in (0, 50, 91, 92, 699):
        assert np.array_equal(idx[i], [j for j in range(93) if j != i][:91])


@pytest.mark.parametrize("k", [8, 91])
def test_grid_builder(k):
    X, idx, d2 = grid_case(k)
    assert gram_exact(X) and X.shape == (1024, 2) and len(np.unique(X, axis=0)) == 1024
    D = np.sort(all_dist(X) + np.diag(np.full(1024, np.inf)), axis=1)
    cut = D[:, k - 1] == D[:, k]
    group = np.sum(D == D[:, k - 1:k], axis=1)
    if k == 8:
        # an interior point has 4 + 4 neighbours at 1 and 2: the cut falls at the end of a tie group of 4, and through a group
        # for the points near the border
        assert np.mean(group == 4) > 0.8 and 0 < np.sum(cut) < 1024 // 8
    else:
        assert np.mean(cut) >= 0.25 and group.max() >= 8                # the cut runs through a tie group


@pytest.mark.parametrize("d", FEATURE_D)
def test_feature_builder(d):
    X, idx, d2 = feature_case(d)
    assert gram_exact(X) and X.shape == (130, d) and np.abs(X).max() == 2
    assert np.array_equal(d2, np.rint(d2))
    if d <= 8:
        D = np.sort(all_dist(X) + np.diag(np.full(130, np.inf)), axis=1)
        assert np.any(D[:, 30] == D[:, 31])


def test_brute_force_agrees_with_the_numpy_backend():
    X = np.random.default_rng(0).normal(size=(300, 7)).astype(np.float32)
    idx, d2 = brute_knn(X, 20)
    ni, nd = tsne.knn_numpy(X, 20)
    assert np.array_equal(idx, ni) and np.allclose(d2, nd, rtol=1e-12, atol=0)


# ---- 2. kNN, real-valued with a planted gap

GAP_N, GAP_D, GAP_K = 600, 50, 30
GAP_r, GAP_R = 0.25, 1.0


def screen_error(X):
    """[n] E_i >= |fl(|x_i|^2) + fl(|x_j|^2) - 2 fl32(x_i.x_j) - |x_i - x_j|^2| for every j, all in float32 with unit roundoff u:
    the two norms are rounded once each (2 u (a^2 + b^2) with the rounding of their sum, a = |x_i|, b = |x_j|), the dot product
    of d terms carries at most (d + 2) u a b however the MFMA orders it, doubled, and the last subtraction rounds a value of at
    most a^2 + b^2 + 2 a b.  Together at most 3 u (a^2 + b^2) + (2 d + 6) u a b <= (d + 6) u (a + b)^2, taken at the largest b."""
    X = np.asarray(X, np.float64)
    a = np.sqrt(np.sum(X * X, axis=1))
    return (X.shape[1] + 6) * U24 * (a + a.max()) ** 2


@functools.lru_cache(maxsize=None)
def gap_case(shifted):
    """19 tight groups of k + 1 = 31 points: the k group-mates of a point lie within r, everything else beyond R.  n = 600 is
    not a multiple of 31, so the last 11 points form a group of radius r / 1000 at 2 R from group 0, and group 0 is a ladder
    of 31 points along the line away from it: the 11 see their 10 mates, then the ladder's points one by one, about
    2 (2 R) (r / 31) apart in squared distance.  Returns X, idx, dist2 (float64 brute force), the k-th and (k + 1)-th squared distance per row."""
    n, d, k, r, R = GAP_N, GAP_D, GAP_K, GAP_r, GAP_R
    rng = np.random.default_rng(600)
    X = np.empty((n, d))
    for g in range(19):
        c = np.zeros(d)
        c[g] = 4.0 * R
        v = rng.normal(size=(k + 1, d))
        X[31 * g:31 * g + 31] = c + v / np.linalg.norm(v, axis=1, keepdims=True) * (r / 2) * rng.uniform(0.2, 1.0, (k + 1, 1))
    X[0:31] = 0.0
    X[0:31, 0] = 4.0 * R
    X[0:31, 20] = -np.arange(31) * (r / 31)
    X[0:31] += rng.normal(size=(31, d)) * (r * 1e-4)
    X[589:] = 0.0
    X[589:, 0] = 4.0 * R
    X[589:, 20] = 2.0 * R
    X[589:] += rng.normal(size=(11, d)) * (r * 1e-3 / math.sqrt(d))
    X -= X.mean(axis=0)
    if shifted:
        X += 10.0 * R / math.sqrt(d)                        # a constant vector of squared norm 100 R^2
    X = X.astype(np.float32)
    D = np.sort(all_dist(X) + np.diag(np.full(n, np.inf)), axis=1)
    idx, d2 = brute_knn(X, k)
    return X, idx, d2, D[:, k - 1], D[:, k]


@pytest.mark.parametrize("shifted", [False, True])
def test_gap_builder(shifted):
    X, idx, d2, rk, rk1 = gap_case(shifted)
    n, k = GAP_N, GAP_K
    assert X.shape == (n, GAP_D) and not np.array_equal(X, np.rint(X))
    sq = np.sum(X.astype(np.float64) ** 2, axis=1)
    if shifted:
        assert 90 * GAP_R ** 2 < sq.min() and sq.max() < 160 * GAP_R ** 2
    # the planted radii of the 19 full groups
    assert np.all(rk[:589] <= GAP_r ** 2) and np.all(rk1[:589] >= GAP_R ** 2)
    assert np.all(idx[:589] // 31 == (np.arange(589) // 31)[:, None])
    # the last group: 10 mates, then the first 20 rungs of the ladder
    for i in range(589, 600):
        assert sorted(idx[i]) == list(range(20)) + [j for j in range(589, 600) if j != i]
    # the float32 screen cannot lose a true neighbour: the gap exceeds twice its error, for every row
    E = screen_error(X)
    assert np.all(rk1 - rk > 2 * E), float(np.min((rk1 - rk) / (2 * E)))
    assert np.all(d2[:, 1:] > d2[:, :-1])                   # no ties: the order inside the k is decided too
    gaps = (d2[:, 1:] - d2[:, :-1]) / d2[:, 1:]
    assert gaps.min() > 1e3 * (GAP_D + 2) * U53             # ... far beyond the rounding of a double distance


def gap_limit(d):
    """the ratio (largest squared norm) / (R^2 - r^2) at which R^2 - r^2 > 2 E stops holding when every norm is the same:
    2 (d + 6) 2^-24 (2 |x|)^2 = gap"""
    return 2.0 ** 21 / (d + 6)


def test_gap_limit_figure():
    assert 37000 < gap_limit(50) < 38000


# ---- 3. perplexity search

AFF_N = 1027
AFF_CASES = [(1, 1.5), (2, 1.5), (16, 5), (63, 20), (64, 20), (65, 21), (128, 40), (129, 42), (192, 60), (193, 64), (256, 85),
             (257, 85), (301, 100)]
AFF_SCALES = [1.0, 1e4, 1e-6]
TINY_SUM = 1e-290
MARGIN = 1e-10


def traced_search(dist2, perplexity):
    """tsne.binary_search_perplexity with a trace.  Returns P and, per row: the least min(|diff|, ||diff| - tol|) over all steps
    (less the step's subnormal uncertainty, below), whether sum_p was ever non-zero but below 1e-290, the steps run (101:
    never converged), the last beta, the last sum_p (after the floor) and the last diff.

    Subnormal uncertainty: an exponential below 2^-1022 is off by up to one subnormal spacing h = 2^-1074 whatever the
    library (a normal one by 2^-52 of itself, a zero stays zero).  With m = sum_p / h, perturbing the c subnormal
    exponentials by h each moves diff = log s + beta sum d_j p_j by at most (c / m) (2 + ln m): each entry counts through log s (1 / m) and through its own term, beta (d_j - mean d) <= ln m for
    every entry that is not zero.  For a normal sum_p this is below 1e-300."""
    D = np.asarray(dist2, np.float32).astype(np.float64)
    n = D.shape[0]
    desired = math.log(float(np.float32(perplexity)))
    tol, floor_sum = float(np.float32(1e-5)), float(np.float32(1e-8))
    beta, bmin, bmax = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    P = np.zeros_like(D)
    live = np.ones(n, bool)
    least, tiny, steps = np.full(n, np.inf), np.zeros(n, bool), np.zeros(n, int)
    last_beta, last_sum, last_diff = np.ones(n), np.zeros(n), np.zeros(n)
    for _ in range(100):
        r = np.nonzero(live)[0]
        if r.size == 0:
            break
        p = np.exp(-D[r] * beta[r, None])
        s = p.sum(axis=1)
        tiny[r] |= (s != 0.0) & (s < TINY_SUM)
        nsub = np.sum((p > 0.0) & (p < 2.0 ** -1022), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lnm = np.log(s) + 1074.0 * math.log(2.0)
            unc = np.where(s > 0.0, nsub * (2.0 ** -1074 / s) * (2.0 + np.maximum(lnm, 0.0)), 0.0)
        s[s == 0.0] = floor_sum
        p /= s[:, None]
        P[r] = p
        diff = np.log(s) + beta[r] * np.sum(D[r] * p, axis=1) - desired
        least[r] = np.minimum(least[r], np.minimum(np.abs(diff), np.abs(np.abs(diff) - tol)) - unc)
        steps[r] += 1
        last_beta[r], last_sum[r], last_diff[r] = beta[r], s, diff
        done = np.abs(diff) <= tol
        up = ~done & (diff > 0)
        dn = ~done & ~(diff > 0)
        ru, rd = r[up], r[dn]
        bmin[ru] = beta[ru]
        beta[ru] = np.where(bmax[ru] == np.inf, beta[ru] * 2.0, (beta[ru] + bmax[ru]) / 2.0)
        bmax[rd] = beta[rd]
        beta[rd] = np.where(bmin[rd] == -np.inf, beta[rd] / 2.0, (beta[rd] + bmin[rd]) / 2.0)
        live[r[done]] = False
    converged = np.abs(last_diff) <= tol
    return P, least, tiny, np.where(converged, steps, 101), last_beta, last_sum, last_diff


def affinity_bound(D32, k, beta, sum_p):
    """(rel [n], absolute [n], a [n]): |p_device - p_reference| <= rel p_reference + absolute per entry, for two evaluations of
    exp(-d beta) / sum that follow the same beta path.  With u = 2^-53 and a = max_j d_j beta: the argument d beta is rounded
    (a u relative in the exponential) and exp is good to one ulp (2 u): (a + 2) u per exponential, once in the entry and once
    through the sum; the sum of k terms and the division round k times: (k + 8) u with the issue's allowance.  That is the
    error of one evaluation; two evaluations differ by at most twice it.  An exponential in the subnormal range is off by up
    to the subnormal spacing 2^-1074 instead, which the division by sum_p turns into the absolute term."""
    a = np.max(np.asarray(D32, np.float64), axis=1) * beta
    rel = 2.0 * ((k + 8) * U53 + 2.0 * (a + 2.0) * U53)
    return rel, 4.0 * 2.0 ** -1074 / sum_p, a


def entropy_bound(rel, a, sum_p):
    """|H(p) - log(perplexity)| - tol at a converged row, H(p) = -sum p log p of the returned p in exact arithmetic: with
    p_j = e_j / s (1 + delta_j) and log e_j = -d_j beta + eps_j, H(p) = log s sum p + beta sum d_j p_j - sum p_j (eps_j +
    delta_j): it differs from the kernel's diff + log(perplexity) by the roundings of that expression, terms of size at most
    |log s| + a each to rel / 2, by (sum p - 1) log s and by the eps and delta themselves"""
    return 4.0 * rel * (1.0 + a + np.abs(np.log(sum_p)))


@functools.lru_cache(maxsize=None)
def affinity_case(k, perplexity, scale, n=AFF_N):
    """sorted gamma(2, 1) draws times scale, float64 (not float32-representable).  Returns D, P, marginal rows, converged rows,
    rel, absolute, a, the last sum_p, the rows whose sum_p was ever non-zero but below 1e-290.

    A row is marginal when a decision of the search (diff > 0, |diff| <= tol) came within 1e-10 of flipping, after the
    subnormal uncertainty of traced_search.  The bare flag `sum_p < 1e-290` is not part of it: at scale 1e4 beta halves from
    where every exponential underflows, and d_min beta lands in 668 .. 745 for one row in seven (log2(745 / 668) = 0.16), so
    the flag alone marks 11 % to 16 % of the rows of every case; what an exponential near underflow can actually move is
    the uncertainty term, and it leaves more rows in the comparison, not fewer."""
    rng = np.random.default_rng(1000 * k + int(round(math.log10(scale))) + 7)
    D = np.sort(rng.gamma(2.0, 1.0, (n, k)), axis=1) * scale
    return (D,) + affinity_reference(D, perplexity)


def affinity_reference(D, perplexity):
    k = D.shape[1]
    P, least, tiny, steps, beta, s, diff = traced_search(D, perplexity)
    rel, ab, a = affinity_bound(np.asarray(D, np.float32), k, beta, s)
    return P, least < MARGIN, steps <= 100, rel, ab, a, s, tiny


@functools.lru_cache(maxsize=None)
def affinity_blocks(k=64, perplexity=20.0, rows=128):
    """rows of k equal distances, then rows of zeros, then rows of distances near 1e36.  Equal distances c keep P uniform and
    the entropy log k above the target at every beta, so beta doubles for all 100 steps; c <= 2^-91 keeps c beta <= 512 and exp
    away from its underflow.  At 1e36 every exponential is zero down to beta = 2^-99: the search ends on the sum_p == 0 floor
    and P is 0 / 1e-8 = 0 (without the floor it is 0 / 0)."""
    rng = np.random.default_rng(64)
    c = rng.gamma(2.0, 1.0, (rows, 1)) * 2.0 ** -95
    huge = np.sort(rng.gamma(2.0, 1.0, (rows, k)), axis=1) * 1e36
    D = np.concatenate([np.repeat(c, k, axis=1), np.zeros((rows, k)), huge])
    return (D,) + affinity_reference(D, perplexity)


@functools.lru_cache(maxsize=None)
def affinity_pair():
    D = np.array([[0.7], [0.7]])
    return (D,) + affinity_reference(D, 1.5)


@pytest.mark.parametrize("scale", AFF_SCALES)
@pytest.mark.parametrize("k,perplexity", AFF_CASES)
def test_affinity_builder(k, perplexity, scale):
    D, P, marginal, conv, rel, ab, a, s, tiny = affinity_case(k, perplexity, scale)
    assert D.shape == (AFF_N, k) and AFF_N % 4 == 3
    assert np.mean(np.asarray(D, np.float32).astype(np.float64) != D) > 0.9          # a missing (float) cast would show
    assert np.array_equal(P, tsne.binary_search_perplexity(D, perplexity))
    assert np.sum(marginal) <= AFF_N // 100, int(np.sum(marginal))
    assert np.all(rel < 1e-11) and np.all(np.isfinite(ab))
    if k > 1:
        assert np.mean(conv) > 0.9
        assert np.all(np.abs(P[conv].sum(axis=1) - 1.0) <= (k + 8) * 2.0 ** -52)
    else:
        assert not np.any(conv) and np.all(P == 1.0)                                 # diff = -log 1.5 at every beta


@pytest.mark.parametrize("k,perplexity", AFF_CASES)
def test_large_scale_reaches_the_sum_floor(k, perplexity):
    case = affinity_case(k, perplexity, 1e4)
    D, tiny = case[0], case[-1]
    floored = np.sum(np.exp(-np.asarray(D, np.float32).astype(np.float64)), axis=1) == 0.0      # the first step, beta = 1
    # a row floors when all its k draws exceed 745 / 1e4: with probability ((1 + x) exp(-x))^k, x = 0.0745; the float32 rounding
    # of exp's underflow point does not matter at this width (four standard deviations of 1027 draws)
    expect = ((1.0 + 0.0745) * math.exp(-0.0745)) ** k
    assert abs(float(np.mean(floored)) - expect) < 0.065 and np.mean(floored) > 0.4
    # beta then halves through the range where sum_p is below 1e-290: that flag alone marks far more than 1 % of the rows,
    # which is why it is not part of `marginal` (affinity_case)
    assert np.mean(tiny) > 0.05


def test_affinity_blocks_builder():
    D, P, marginal, conv, rel, ab, a, s, tiny = affinity_blocks()
    assert not np.any(marginal) and not np.any(conv)
    assert np.all(np.abs(P[:256] - 1.0 / 64) <= 2.0 ** -52) and np.all(P[128:256] == 1.0 / 64)
    D32 = np.asarray(D[256:], np.float32).astype(np.float64)
    assert np.all(np.isfinite(D32)) and np.all(np.exp(-D32 * 2.0 ** -99) == 0.0) and np.all(P[256:] == 0.0)
    assert np.all(s[256:] == float(np.float32(1e-8))) and not np.any(tiny)
    D, P, marginal, conv, rel, ab, a, s, tiny = affinity_pair()
    assert np.all(P == 1.0) and not np.any(marginal)


# ---- 4. repulsion and Z, counted

COUNTED_N = [2, 255, 257, 511, 513, 1024, 1025, 65536, 65537, 262144]
COUNTED_PAIRS = [((0, 0), (1, 0)), ((0, 0), (0, 1)), ((5, -3), (6, -3))]


@functools.lru_cache(maxsize=None)
def counted_case(n, pair):
    """Y [n][2] float32 on the two locations of COUNTED_PAIRS[pair] (distance exactly 1), assigned by a fixed-seed coin (one
    point each at n = 2).  Returns Y, Z, the expected gradient float32(-(rep / Z)) * 4 and the float64 sum of its squares"""
    a, b = (np.array(p, np.float64) for p in COUNTED_PAIRS[pair])
    coin = np.random.default_rng(n + pair).integers(0, 2, n) if n > 2 else np.array([0, 1])
    c1 = int(coin.sum())
    c0 = n - c1
    Y = np.where(coin[:, None] == 0, a, b).astype(np.float32)
    Z = float(c0 * c0 + c1 * c1 + c0 * c1 - n)
    rep = np.where(coin[:, None] == 0, (a - b) * (c1 / 4.0), (b - a) * (c0 / 4.0))
    grad = (-(rep / Z)).astype(np.float32) * np.float32(4.0)
    gn = math.fsum((grad.astype(np.float64) ** 2).ravel())
    return Y, Z, grad, gn, (c0, c1)


@pytest.mark.parametrize("pair", range(len(COUNTED_PAIRS)))
@pytest.mark.parametrize("n", COUNTED_N)
def test_counted_builder(n, pair):
    Y, Z, grad, gn, (c0, c1) = counted_case(n, pair)
    assert c0 >= 1 and c1 >= 1 and Y.shape == (n, 2)
    d2 = np.sum((Y[:1].astype(np.float64) - Y[np.argmax(np.any(Y != Y[0], axis=1))]) ** 2)
    assert d2 == 1.0                                                    # w = 1 or 1/2, w^2 dy = 0, +-1/4
    # every float32 partial is a multiple of 1/4 below 2^24 / 4: the z of a segment is at most its length, and exact
    assert segment(n) < 2 ** 22 and Z < 2.0 ** 53 and Z == c0 * (c0 - 1) + c1 * (c1 - 1) + c0 * c1
    assert grad.dtype == np.float32 and np.all(np.isfinite(grad)) and gn > 0
    if n <= 1025:
        empty = (np.zeros(n + 1, np.int64), np.zeros(0, np.int64), np.zeros(0))
        err, g = tsne.gradient_numpy(Y, empty)
        assert err == 0.0
        assert np.allclose(g, grad, rtol=1e-6, atol=0)


def test_counted_sizes_cover_the_segment_change():
    assert segment(65536) == 1024 and segment(65537) == 2048 and -(-65537 // 2048) == 33 and 65536 // 1024 == 64
    assert segment(262144) == 4096 and 262144 // 4096 == 64


# ---- 5. gradient, statistics and one step, real-valued

GRAD_N = [2, 3, 255, 256, 257, 1023, 1025, 1537, 2049, 3073]
GRAD_SCALES = [1e-4, 5.0, 50.0]
MOMENTUM, LEARNING_RATE = 0.5, 200.0


@functools.lru_cache(maxsize=None)
def grad_csr(n):
    """(indptr, indices, P rounded to float32) for n points: by hand up to n = 17, else the numpy backend's affinities of random
    factors at perplexity 5"""
    if n == 2:
        return np.array([0, 1, 2]), np.array([1, 0]), np.array([0.5, 0.5])
    if n <= 17:
        idx = np.array([[j for j in range(n) if j != i] for i in range(n)])
        P = np.random.default_rng(n).uniform(0.5, 1.5, (n, n))
        P = (P + P.T)[np.arange(n)[:, None], idx]
        return np.arange(n + 1) * (n - 1), idx.ravel(), (P / P.sum()).astype(np.float32).astype(np.float64).ravel()
    X = np.random.default_rng(n).normal(size=(n, 10)).astype(np.float32)
    ip, ix, P = tsne.affinities(X, 5.0, backend="numpy")
    return ip, ix, P.astype(np.float32).astype(np.float64)


def hostile_csr(n=1025):
    """a CSR that breaks every promise: empty rows, one row of 602 entries, column indices -1, n and 2^31 - 1, a row pointer
    above nnz and one that decreases.  Returns (indptr, indices, P) as int64 / float64 holding int32 / float32 values"""
    rng = np.random.default_rng(1025)
    counts = rng.integers(0, 12, n)
    counts[::7] = 0
    counts[300] = 602
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, n, nnz).astype(np.int64)
    indices[::53] = -1
    indices[1::59] = n
    indices[2::61] = 2 ** 31 - 1
    P = rng.uniform(0.0, 2.0 / nnz, nnz).astype(np.float32).astype(np.float64)
    indptr[500] = nnz + 1000                # above nnz: row 499 runs to the end, row 500 is empty
    indptr[800] = indptr[799] - 5           # decreasing: row 799 is empty, row 800 starts 5 entries early
    return indptr, indices, P


def sanitise_csr(csr, n):
    """the contract's reading of any CSR: row pointers clamped into [0, nnz] and kept non-decreasing within a row, column
    indices outside [0, n) skipped.  Returns a valid CSR with the surviving entries in their order"""
    indptr, indices, P = csr
    nnz = len(indices)
    rows, cols, vals = [], [], []
    for i in range(n):
        e0 = min(max(int(indptr[i]), 0), nnz)
        e1 = min(max(int(indptr[i + 1]), e0), nnz)
        for e in range(e0, e1):
            if 0 <= indices[e] < n:
                rows.append(i), cols.append(int(indices[e])), vals.append(P[e])
    ip = np.searchsorted(np.array(rows), np.arange(n + 1))
    return ip, np.array(cols, np.int64), np.array(vals)


def gradient_terms(Y, csr, exaggeration):
    """the float64 reference with its sums of absolute terms: (KL, grad, A, R, Z, kl_abs, psum, rowlen): grad = 4 (attr - rep /
    Z); A [n][2] = sum |attraction terms|, R [n][2] = sum |repulsion terms| per row and component; kl_abs = sum |KL terms|,
    psum = sum of e p"""
    Y = np.asarray(Y, np.float64)
    indptr, indices, P = csr
    n = Y.shape[0]
    D = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + np.sum(D * D, axis=2))
    np.fill_diagonal(w, 0.0)
    Z = max(float(np.sum(w)), tsne.MACHINE_EPSILON)
    t = (w * w)[:, :, None] * D
    rep, R = t.sum(axis=1), np.abs(t).sum(axis=1)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    De = Y[rows] - Y[indices]
    we = 1.0 / (1.0 + np.sum(De * De, axis=1))
    pe = exaggeration * np.asarray(P, np.float64)
    f = (pe * we)[:, None] * De
    attr = np.stack([np.bincount(rows, f[:, c], n) for c in (0, 1)], axis=1)
    A = np.stack([np.bincount(rows, np.abs(f[:, c]), n) for c in (0, 1)], axis=1)
    kt = pe * np.log(np.maximum(pe, tsne.FLOAT32_TINY) / np.maximum(we / Z, tsne.FLOAT32_TINY))
    return float(np.sum(kt)), 4.0 * (attr - rep / Z), A, R, Z, float(np.sum(np.abs(kt))), float(np.sum(pe)), np.diff(indptr)


def gradient_bound(n, A, R, Z, rowlen):
    """per entry: (L + 8) 2^-24 times the reference's sums of absolute terms, 4 (sum |attraction terms| + sum |repulsion
    terms| / Z), with L the longest float32 chain behind each sum: the CSR row for the attraction (one product chain per
    term of about 8 roundings: the difference, the squared distance, the division, e p, f, f dx; then one addition each), the
    segment for the repulsion (the difference, two FMAs, v_rcp_f32 to one ulp, w^2, one FMA per column; the segment partials
    and Z's block partials are then added in double)"""
    Ls = min(n, segment(n))
    return 4.0 * U24 * ((rowlen[:, None] + 8) * A + (Ls + 8) * R / Z)


def kl_bound(n, kl_abs, psum):
    """the KL statistic: every term e p log(e p / (w / Z)) is formed in double from float32 e p (one rounding: the term and its
    derivative, |t| + e p), a float32 w (about 8 roundings: 8 e p) and the Z of float32 partials over chains of L columns
    ((L + 8) e p)"""
    Ls = min(n, segment(n))
    return U24 * (kl_abs + (Ls + 17) * psum)


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def gradient_case(n, scale, hostile=False):
    """Y (float32 normal draws times scale), the CSR as the device takes it, exaggeration, and the reference: KL, grad, the
    gradient bound, the KL bound, the squared norm and its bound"""
    rng = np.random.default_rng(n * 7 + int(scale * 10))
    Y = (rng.normal(size=(n, 2)) * scale).astype(np.float32)
    raw = hostile_csr(n) if hostile else grad_csr(n)
    exag = 12.0 if n == 2 or (n + int(scale)) % 2 else 1.0      # at n = 2 and e = 1 the gradient cancels to zero
    kl, g, A, R, Z, kl_abs, psum, rowlen = gradient_terms(Y, sanitise_csr(raw, n) if hostile else raw, exag)
    gb = gradient_bound(n, A, R, Z, rowlen)
    gn = float(np.sum(g * g))
    return Y, raw, exag, kl, g, gb, kl_bound(n, kl_abs, psum), gn, float(np.sum(2.0 * np.abs(g) * gb + gb * gb)) + n * U53 * gn


@functools.lru_cache(maxsize=None)
def step_case(n, scale):
    """the state before one ra_tsne_step and the expected state after it.  Returns update, gains (float32), the float32 gains
    expected, the entries where the gain's branch is decided beyond the gradient bound, update' and y' in float64 and their
    bounds"""
    Y, csr, exag, kl, g, gb, klb, gn, gnb = gradient_case(n, scale)
    rng = np.random.default_rng(n + 1)
    upd = (rng.normal(size=(n, 2)) * 0.1 * scale).astype(np.float32)
    gains = rng.uniform(0.5, 2.0, (n, 2)).astype(np.float32)
    gains[::3] = np.float32(0.011)
    upd[1::11] = 0.0
    inc = upd.astype(np.float64) * g < 0.0
    new_gains = np.maximum(np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01)).astype(np.float32)
    # the branch reads the sign of u g: decided when g_ref is farther from zero than its bound (u = 0 never increments), and
    # the float32 product does not underflow
    decided = (np.abs(g) > gb) & (np.abs(upd.astype(np.float64) * g) > 1e-37) | (upd == 0.0)
    G = new_gains.astype(np.float64)
    t1, t2 = MOMENTUM * upd.astype(np.float64), LEARNING_RATE * g * G
    new_upd = t1 - t2
    ub = LEARNING_RATE * G * gb + 2.0 * ulp32(np.maximum(np.maximum(np.abs(t1), np.abs(t2)), np.abs(new_upd)))
    new_y = Y.astype(np.float64) + new_upd
    yb = ub + 2.0 * ulp32(np.maximum(np.abs(Y.astype(np.float64)), np.abs(new_y)))
    return upd, gains, new_gains, decided, new_upd, ub, new_y, yb


@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("n", GRAD_N)
def test_gradient_builder(n, scale):
    Y, csr, exag, kl, g, gb, klb, gn, gnb = gradient_case(n, scale)
    assert Y.dtype == np.float32 and Y.shape == (n, 2)
    assert np.array_equal(np.asarray(csr[2], np.float32).astype(np.float64), csr[2]) and len(csr[0]) == n + 1
    e2, g2 = tsne.gradient_numpy(Y, csr, exag)
    assert np.allclose(g, g2, rtol=1e-9, atol=1e-300) and abs(kl - e2) <= 1e-9 * abs(e2) + 1e-300
    assert np.all(gb > 0) and np.all(np.isfinite(gb)) and klb > 0
    upd, gains, new_gains, decided, new_upd, ub, new_y, yb = step_case(n, scale)
    assert np.mean(decided) >= 0.95, float(np.mean(decided))
    if n >= 255:
        inc = upd.astype(np.float64) * g < 0.0
        assert np.any(inc & decided) and np.any(~inc & decided)                       # both branches of the gain
        assert np.any((new_gains == np.float32(0.01)) & decided)                      # and the floor
        assert np.any(new_gains[decided] > 1.0)


def test_hostile_csr_builder():
    n = 1025
    indptr, indices, P = hostile_csr(n)
    nnz = len(indices)
    assert np.any(np.diff(indptr) == 0) and np.max(np.diff(indptr)[:499]) == 602
    assert np.any(indices == -1) and np.any(indices == n) and np.any(indices == 2 ** 31 - 1)
    assert indptr.max() > nnz and np.any(np.diff(indptr) < 0) and nnz <= 2 * n * 301
    assert np.all(np.abs(indptr) < 2 ** 31) and np.all(np.abs(indices) < 2 ** 31)
    ip, ix, pv = sanitise_csr((indptr, indices, P), n)
    assert np.all(np.diff(ip) >= 0) and ip[-1] == len(ix) and np.all((ix >= 0) & (ix < n))
    assert ip[500] - ip[499] == nnz - indptr[499] - np.sum((indices[indptr[499]:] < 0) | (indices[indptr[499]:] >= n))
    assert ip[501] == ip[500] and ip[800] == ip[799]
    Y, raw, exag, kl, g, gb, klb, gn, gnb = gradient_case(n, 5.0, True)
    assert np.all(np.isfinite(g)) and np.isfinite(kl)
