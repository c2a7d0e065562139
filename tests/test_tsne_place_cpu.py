"""Out-of-sample t-SNE without a GPU: the float64 checker of tsne.transform (its gradient against finite differences, the bound of
rule 4, rule 7, the start rules, the label vote, tsne_large's draw, the domain errors and the tool), and the input builders and
float64 references that tests/test_gpu_tsne_place.py imports.  Every property a device case relies on is asserted here.

Exact cases (integer coordinates, counted embeddings) are built so that every float32 and float64 value the kernels form is exact.
Toleranced cases carry a bound computed here from term counts and the magnitudes of the float64 reference, never from a device
result.  The placement kernel's column order (tsne_place_kernel): the fitted points go through LDS in chunks of PLACE_CHUNK; of a
chunk, lane l of the 64 takes columns l, l + 64, ..., at most RUN = PLACE_CHUNK / 64 of them, adds them in float32 and adds that
partial to a double; the 64 doubles are added by a butterfly.  So the longest float32 run is RUN whatever m."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from cryo_ralib_amd import tsne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
KNN_MARGIN = 32
PLACE_CHUNK, PLACE_WAVE_ROWS, PLACE_ROWS = 2048, 4, 16
RUN = PLACE_CHUNK // 64


# ---- 1. kNN of query rows against base rows, exact

def brute_query(Q, X, k):
    """(idx [nq][k] int64, dist2 [nq][k]) by float64 differences over all pairs and np.lexsort((index, distance)) per row"""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    ar = np.arange(X.shape[0])
    idx = np.empty((Q.shape[0], k), np.int64)
    d2 = np.empty((Q.shape[0], k))
    for i in range(Q.shape[0]):
        D = np.sum((Q[i] - X) ** 2, axis=1)
        o = np.lexsort((ar, D))[:k]
        idx[i], d2[i] = o, D[o]
    return idx, d2


def gram_exact(*arrays):
    """integer coordinates, unchanged by float32, and 4 max |x|^2 < 2^24 over all rows: the float32 Gram screen and the double
    distances are exact"""
    for A in arrays:
        A64 = np.asarray(A, np.float64)
        if A.dtype != np.float32 or not np.array_equal(A64, np.rint(A64)) or 4.0 * float(np.max(np.sum(A64 * A64, axis=1))) >= 2.0 ** 24:
            return False
    return True


LINE_M = [1, 2, 16, 17, 63, 64, 65, 257, 1100]
LINE_NQ = [1, 15, 16, 17, 33]
LINE_CASES = sorted({(m, k) for k in (1, 5, 91, 301) for m in LINE_M + [k + KNN_MARGIN, k + KNN_MARGIN + 1] if k <= m}
                    | {(m, m) for m in LINE_M if m <= 301})
LINE_CASES = [(m, k, LINE_NQ[i % len(LINE_NQ)]) for i, (m, k) in enumerate(LINE_CASES)]


@functools.lru_cache(maxsize=None)
def line_case(m, k, nq, reverse):
    """base points 0 .. m - 1 on a line (or reversed), nq integer queries from -3 to m + 2: some equal to base points, some
    between ties, some outside the line"""
    j = np.arange(m, dtype=np.float32)
    X = (m - 1 - j if reverse else j).reshape(m, 1)
    Q = ((np.arange(nq) * 7) % (m + 6) - 3).astype(np.float32).reshape(nq, 1)
    return (Q, X) + brute_query(Q, X, k)


FEATURE_D = [1, 2, 3, 4, 5, 7, 8, 50, 2047, 2048]


@functools.lru_cache(maxsize=None)
def feature_case(d, m=130, nq=33, k=31):
    rng = np.random.default_rng(d)
    X, Q = rng.integers(-2, 3, (m, d)).astype(np.float32), rng.integers(-2, 3, (nq, d)).astype(np.float32)
    return (Q, X) + brute_query(Q, X, k)


@functools.lru_cache(maxsize=None)
def identical_case(m=700, k=91):
    """700 identical base points; queries on them and off them"""
    X = np.tile(np.array([3.0, -1.0, 2.0], np.float32), (m, 1))
    Q = np.array([[3, -1, 2], [3, -1, 3], [0, 0, 0], [3, -1, 2], [-40, 7, 2]], np.float32)
    return (Q, X) + brute_query(Q, X, k)


@functools.lru_cache(maxsize=None)
def grid_case(k, side=32):
    """a shuffled side x side grid; the queries are 300 of its own points (each lists itself first) and 100 points off the grid"""
    rng = np.random.default_rng(32)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)
    X = g[rng.permutation(side * side)].astype(np.float32)
    Q = np.concatenate([X[rng.permutation(side * side)[:300]], rng.integers(-4, side + 4, (100, 2)).astype(np.float32)])
    return (Q, X) + brute_query(Q, X, k)


def duplicate_free(n=600, d=7, seed=11):
    """rows without duplicates or tied distances to speak of: knn_query(X, X, k + 1) must list row i first"""
    X = np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)
    assert len(np.unique(X, axis=0)) == n
    return X


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("m,k,nq", LINE_CASES)
def test_line_builder(m, k, nq, reverse):
    Q, X, idx, d2 = line_case(m, k, nq, reverse)
    assert gram_exact(Q, X) and X.shape == (m, 1) and Q.shape == (nq, 1) and idx.shape == (nq, k)
    assert np.all(np.diff(d2, axis=1) >= 0)
    same = d2[:, 1:] == d2[:, :-1]
    assert np.all(idx[:, 1:][same] > idx[:, :-1][same])                # ties in index order
    on = np.nonzero((Q[:, 0] >= 0) & (Q[:, 0] <= m - 1))[0]
    assert np.all(d2[on, 0] == 0.0) and np.all(X[idx[on, 0], 0] == Q[on, 0])     # a query on a base point lists it first
    ni, nd = tsne.knn_query_numpy(Q, X, k)
    assert np.array_equal(ni, idx) and np.array_equal(nd, d2)


def test_line_cases_cover_the_lists():
    ms, ks, nqs = ({c[i] for c in LINE_CASES} for i in range(3))
    assert ms >= set(LINE_M) | {33, 34, 37, 38, 123, 124, 333, 334} and ks >= {1, 5, 91, 301} and nqs == set(LINE_NQ)
    assert {(m, k) for m, k, _ in LINE_CASES} >= {(m, m) for m in LINE_M if m <= 301}
    assert len(LINE_CASES) < 40


def test_special_builders():
    Q, X, idx, d2 = identical_case()
    assert gram_exact(Q, X) and np.all(idx == np.arange(91)) and np.all(d2[0] == 0.0) and np.all(d2[1] == 1.0)
    for k in (8, 91):
        Q, X, idx, d2 = grid_case(k)
        assert gram_exact(Q, X) and len(np.unique(X, axis=0)) == 1024
        assert np.all(d2[:300, 0] == 0.0) and np.all(X[idx[:300, 0]] == Q[:300])
        assert np.mean(d2[:, k - 1] == np.sort(np.sum((Q[:, None, :].astype(np.float64) - X[None]) ** 2, axis=2), axis=1)[:, k]) > 0.2
    for d in FEATURE_D:
        Q, X, idx, d2 = feature_case(d)
        assert gram_exact(Q, X) and X.shape == (130, d) and np.array_equal(d2, np.rint(d2))


def test_knn_query_checker_lists_an_equal_row_first():
    X = duplicate_free()
    idx, d2 = tsne.knn_query(X, X, 11, backend="numpy")
    assert np.array_equal(idx[:, 0], np.arange(len(X))) and np.all(d2[:, 0] == 0.0)
    ki, kd = tsne.knn_numpy(X, 10)
    assert np.array_equal(idx[:, 1:], ki) and np.allclose(d2[:, 1:], kd, rtol=1e-12, atol=0)
    bi, bd = brute_query(X[:50], X, 11)
    assert np.array_equal(idx[:50], bi) and np.allclose(d2[:50], bd, rtol=1e-12, atol=0)


# ---- 2. repulsion and Z_i, counted

COUNTED_PAIRS = [((0, 0), (1, 0)), ((0, 0), (0, 1)), ((5, -3), (6, -3))]
COUNTED_M = [1, 2, 255, 257, 511, 513, 1024, 1025, 65536, 65537, 262144]
PLAN_M = [63, 64, 65, PLACE_CHUNK - 1, PLACE_CHUNK, PLACE_CHUNK + 1, 2 * PLACE_CHUNK, 2 * PLACE_CHUNK + 1]     # lanes; chunks
COUNTED_N = [1, 3, 1025]
PLAN_N = [PLACE_WAVE_ROWS, PLACE_WAVE_ROWS + 1, PLACE_ROWS, PLACE_ROWS + 1]                      # a wave's rows; a workgroup's
COUNTED_CASES = [(m, n) for m in COUNTED_M + PLAN_M for n in COUNTED_N] + [(m, n) for m in (257, PLACE_CHUNK + 1) for n in PLAN_N]
COUNTED_CASES = [(m, n, i % len(COUNTED_PAIRS)) for i, (m, n) in enumerate(COUNTED_CASES)]


@functools.lru_cache(maxsize=None)
def counted_case(m, n, pair):
    """fitted points Y [m][2] and new points y [n][2] on the two locations of COUNTED_PAIRS[pair] (distance exactly 1) by
    fixed-seed coins; an empty attraction (every list entry is -1).  Returns Y, y, idx, p, Z_i, the row repulsion sum_j w^2 (y_i -
    Y_j) and the gradient float32(4 (0 - rep / Z)): w is 1 or 1/2, w^2 d is 0 or +-1/4, so every partial sum is exact"""
    a, b = (np.array(q, np.float64) for q in COUNTED_PAIRS[pair])
    rng = np.random.default_rng(m * 7 + n + pair)
    cf, cn = rng.integers(0, 2, m), rng.integers(0, 2, n)
    Y, y = (np.where(c[:, None] == 0, a, b).astype(np.float32) for c in (cf, cn))
    c1 = int(cf.sum())
    c0 = m - c1
    Z = np.where(cn == 0, c0 + c1 / 2.0, c1 + c0 / 2.0)
    rep = np.where(cn[:, None] == 0, (a - b) * (c1 / 4.0), (b - a) * (c0 / 4.0))
    grad = (4.0 * (0.0 - rep / Z[:, None])).astype(np.float32)
    return Y, y, np.full((n, 1), -1, np.int32), np.ones((n, 1), np.float32), Z, rep, grad


@pytest.mark.parametrize("m,n,pair", COUNTED_CASES)
def test_counted_builder(m, n, pair):
    Y, y, idx, p, Z, rep, grad = counted_case(m, n, pair)
    assert Y.shape == (m, 2) and y.shape == (n, 2) and np.all(Z >= m / 2.0) and np.all(np.isfinite(grad))
    assert RUN * 1.0 < 2 ** 22 and m < 2 ** 51                           # float32 partials are multiples of 1/4 up to RUN
    if m <= 1025:
        g, kl, z = tsne.place_gradient_numpy(y, Y, idx, p)
        assert np.array_equal(z, Z) and np.all(kl == 0.0) and np.array_equal(g.astype(np.float32), grad)


def test_counted_sizes_cover_the_plan():
    ms, ns = {c[0] for c in COUNTED_CASES}, {c[1] for c in COUNTED_CASES}
    assert ms >= set(COUNTED_M) | {63, 64, 65, 2047, 2048, 2049, 4096, 4097} and ns >= {1, 3, 4, 5, 16, 17, 1025}
    assert {c[2] for c in COUNTED_CASES} == {0, 1, 2}


# ---- 3. gradient, KL_i and Z_i, real-valued

GRAD_M = [1, 2, 3, 255, 256, 257, 1023, 1025, 3073]
GRAD_N = [1, 5, 257]
GRAD_SCALES = [1e-4, 5.0, 50.0]


def random_lists(rng, n, m, k):
    """idx [n][k] distinct fitted rows per new point, p [n][k] float32 values summing to about 1"""
    idx = np.stack([rng.permutation(m)[:k] for _ in range(n)]).astype(np.int64)
    p = rng.uniform(0.2, 1.0, (n, k))
    return idx, (p / p.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def hostile_lists(n=257, m=1025, k=12):
    """lists that break every promise: columns -1, m and 2^31 - 1, and rows of zero p"""
    rng = np.random.default_rng(1025)
    idx, p = random_lists(rng, n, m, k)
    flat = idx.reshape(-1)
    flat[::53], flat[1::59], flat[2::61] = -1, m, 2 ** 31 - 1
    p[::9] = 0.0
    return idx, p


def place_terms(y, Y, idx, p, exaggeration):
    """the float64 reference with its sums of absolute terms: grad, KL_i, Z_i, A [n][2] = sum |e p w d|, R [n][2] = sum |w^2 d|,
    kl_abs [n] = sum |KL terms|, psum [n]; list entries outside 0 .. m - 1 are skipped"""
    y, Y = np.asarray(y, np.float64), np.asarray(Y, np.float64)
    m = Y.shape[0]
    grad, kl, Z = tsne.place_gradient_numpy(y, Y, idx, p, exaggeration)
    D = y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + np.sum(D * D, axis=2))
    R = np.abs((w * w)[:, :, None] * D).sum(axis=1)
    ok = (idx >= 0) & (idx < m)
    j = np.where(ok, idx, 0)
    pv = np.where(ok, p, 0.0)
    De = y[:, None, :] - Y[j]
    we = 1.0 / (1.0 + np.sum(De * De, axis=2))
    A = np.abs((exaggeration * pv * we)[:, :, None] * De).sum(axis=1)
    kt = pv * np.log(np.maximum(pv, tsne.FLOAT32_TINY) / np.maximum(we / Z[:, None], tsne.FLOAT32_TINY))
    assert np.allclose(kt.sum(axis=1), kl, rtol=1e-12, atol=1e-300)
    return grad, kl, Z, A, R, np.abs(kt).sum(axis=1), pv.sum(axis=1)


def gradient_bound(k, A, R, Z):
    """per entry, the form of the fit's bound (tests/test_tsne_edges_cpu.py): 4 2^-24 ((k + 8) sum |attraction terms| + (L + 8)
    sum |repulsion terms| / Z_i), L = RUN the longest float32 run of the column order.  Attraction: a term is formed in float32
    with about 8 roundings (two differences, the squared distance, 1 +, the division, p w, times d), widened to double and added
    in double, so 8 already covers it and k + 8 is the issue's form.  Repulsion: a term carries about 7 roundings (difference,
    two FMAs, v_rcp_f32 to one ulp, w^2, the FMA into the run) and a run adds at most RUN of them in float32; the runs are added
    in double.  Z_i's own relative error (the same runs, all terms positive) multiplies |rep| / Z_i <= R / Z_i and would in the
    worst case double the repulsion part; the form keeps one L, as the fit's does: the roundings of a run do not all align, and
    the measured share of the bound is recorded in DESIGN.md section 4.18.  The rounding of g itself to float32 is within the 8s."""
    return 4.0 * U24 * ((k + 8) * A + (RUN + 8) * R / Z[:, None])


def kl_bound(kl_abs, psum):
    """KL_i: every term p log(p / (w / Z_i)) is formed in double from a float32 p (exact), a float32 w (about 8 roundings: 8 p
    2^-24) and Z_i (runs of RUN: (RUN + 8) p 2^-24); |t| 2^-24 covers the double arithmetic with room"""
    return U24 * (kl_abs + (RUN + 17) * psum)


def z_bound(Z):
    """Z_i: positive terms of about 5 roundings each in float32 runs of RUN"""
    return (RUN + 8) * U24 * Z


@functools.lru_cache(maxsize=None)
def gradient_case(m, n, scale, hostile=False):
    """fitted Y and new y (float32 normal draws times scale), lists, exaggeration and the reference with its bounds"""
    rng = np.random.default_rng(m * 11 + n * 3 + int(scale * 10))
    Y, y = (rng.normal(size=(m, 2)) * scale).astype(np.float32), (rng.normal(size=(n, 2)) * scale).astype(np.float32)
    k = 12 if hostile else min(m, 17)
    idx, p = hostile_lists(n, m, k) if hostile else random_lists(rng, n, m, k)
    exag = 4.0 if (m + n) % 2 else 1.0
    g, kl, Z, A, R, kl_abs, psum = place_terms(y, Y, idx, p, exag)
    return Y, y, idx, p, exag, g, kl, Z, gradient_bound(k, A, R, Z), kl_bound(kl_abs, psum), z_bound(Z)


@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("m", GRAD_M)
def test_gradient_builder(m, scale):
    for n in GRAD_N:
        Y, y, idx, p, exag, g, kl, Z, gb, klb, zb = gradient_case(m, n, scale)
        assert Y.dtype == np.float32 and y.shape == (n, 2) and np.array_equal(p.astype(np.float32).astype(np.float64), p)
        assert np.all(np.isfinite(g)) and np.all(gb > 0) and np.all(klb > 0) and np.all(Z > 0)
        assert np.max(np.abs(g)) <= 2.0 * (exag + 1.0)


def test_hostile_lists_builder():
    idx, p = hostile_lists()
    assert np.any(idx == -1) and np.any(idx == 1025) and np.any(idx == 2 ** 31 - 1) and np.any(np.all(p == 0.0, axis=1))
    Y, y, idx, p, exag, g, kl, Z, gb, klb, zb = gradient_case(1025, 257, 5.0, True)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(kl)) and np.all(kl[::9] == 0.0)


# ---- 4. one and five iterations

PLACE_CASES = [(3, 5), (257, 257), (1025, 5), (3073, 257)]
PLACE_ITERS = [1, 5]
MOMENTUM, LEARNING_RATE = 0.8, 0.1
STEADY_GAIN = np.float32(0.8) + np.float32(0.2) + np.float32(0.2) + np.float32(0.2) + np.float32(0.2)    # one decrement, then up


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def jacobian_norm(y, Y, idx, p, exag, h):
    """[n] the largest absolute row sum of d g_i / d y_i (2 x 2: points do not interact) by central differences of the reference"""
    J = np.zeros((y.shape[0], 2, 2))
    for c in (0, 1):
        e = np.zeros(2)
        e[c] = h
        J[:, :, c] = (tsne.place_gradient_numpy(y + e, Y, idx, p, exag, want_kl=False)[0]
                      - tsne.place_gradient_numpy(y - e, Y, idx, p, exag, want_kl=False)[0]) / (2 * h)
    return np.abs(J).sum(axis=2).max(axis=1)


@functools.lru_cache(maxsize=None)
def place_case(m, n, scale, iters):
    """the float64 run of `iters` iterations of rule 6 from gradient_case's start, with a first-order propagated bound.  Returns
    the float32 gains expected, the entries whose gain branch was decided beyond the bound at every iteration, y in float64 and
    its bound.  The gradient the device forms at iteration t differs from the reference's by its own bound gb_t plus the
    reference's sensitivity to the y error so far, 2 |J_t| yb_t (|J| by central differences; the factor 2 for the second order);
    update and y add two float32 roundings each per iteration."""
    Y, y0, idx, p, exag = gradient_case(m, n, scale)[:5]
    k = idx.shape[1]
    y = y0.astype(np.float64)
    upd, gains = np.zeros_like(y), np.ones((n, 2), np.float32)
    ub, yb = np.zeros_like(y), np.zeros_like(y)
    decided = np.ones((n, 2), bool)
    for _ in range(iters):
        g, _, Z, A, R, _, _ = place_terms(y, Y, idx, p, exag)
        geb = gradient_bound(k, A, R, Z) + 2.0 * jacobian_norm(y, Y, idx, p, exag, 1e-6 * max(scale, 1e-3))[:, None] * yb.max(axis=1)[:, None]
        inc = upd * g < 0.0
        # u = 0 never increments; else the sign of g must stand beyond its bound, the sign of u beyond its own, no underflow
        decided &= (upd == 0.0) & (ub == 0.0) | (np.abs(g) > geb) & (np.abs(upd) > ub) & (np.abs(upd * g) > 1e-37)
        gains = np.maximum(np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01)).astype(np.float32)
        G = gains.astype(np.float64)
        t1, t2 = MOMENTUM * upd, LEARNING_RATE * G * g
        new_upd = t1 - t2
        ub = MOMENTUM * ub + LEARNING_RATE * G * geb + 3.0 * ulp32(np.maximum(np.maximum(np.abs(t1), np.abs(t2)), np.abs(new_upd)))
        new_y = y + new_upd
        yb = yb + ub + 2.0 * ulp32(np.maximum(np.abs(y), np.abs(new_y)))
        upd, y = new_upd, new_y
    return gains, decided, y, yb


@pytest.mark.parametrize("iters", PLACE_ITERS)
@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("m,n", PLACE_CASES)
def test_place_builder(m, n, scale, iters):
    gains, decided, y, yb = place_case(m, n, scale, iters)
    assert np.mean(decided) >= 0.95, float(np.mean(decided))
    assert np.all(np.isfinite(y)) and np.all(yb > 0)
    if iters == 1:
        assert np.all(gains == np.float32(0.8)) and np.all(decided)           # update = 0: no increment
    elif n >= 257 and scale >= 5.0:
        assert np.any(gains[decided] == STEADY_GAIN) and np.any(gains[decided] < np.float32(0.8))           # both branches
    elif scale < 1.0:
        assert np.all(gains == STEADY_GAIN)            # a steady descent: at 1e-4 every w is 1 and g does not depend on y
    Y, y0, idx, p, exag = gradient_case(m, n, scale)[:5]
    ref = tsne.place_numpy(y0, Y, idx, p, exag, MOMENTUM, LEARNING_RATE, iters)[0]
    assert np.allclose(ref, y, rtol=1e-6, atol=1e-7 * scale)          # the checker's gains are doubles, 0.8 is not float32(0.8)


# ---- 5. the checker itself

def clusters(n, d, seed, ncl=5):
    """(rows [n][d] float32, class [n]) of ncl Gaussian clusters with the centres of seed 5"""
    c = np.random.default_rng(5).normal(0.0, 3.0, (ncl, d))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, ncl, n)
    return (c[lab] + rng.normal(size=(n, d))).astype(np.float32), lab


@functools.lru_cache(maxsize=None)
def small_fit(m=600, d=20):
    """600 fitted rows of the clusters, embedded by the numpy backend (max_iter = 250), and 400 held-out draws"""
    Xf, lf = clusters(m, d, 1)
    Xn, ln = clusters(400, d, 2)
    Yf = tsne.tsne(Xf, max_iter=250, random_state=0, backend="numpy").embedding
    return Xf, lf, Yf, Xn, ln


@functools.lru_cache(maxsize=None)
def small_placed():
    Xf, lf, Yf, Xn, ln = small_fit()
    return tsne.transform(Xn, Xf, Yf, backend="numpy", details=True)


def checker_margin(y0, Yf, idx, p, kl64, **kw):
    """10 x the checker's own spread: |mean KL_i of its float64 run - mean KL_i of a float32 run of the same numpy loop|"""
    kl32 = tsne.place_numpy(y0, Yf, idx, p, dtype=np.float32, **kw)[1]
    return 10.0 * abs(float(np.mean(kl64)) - float(np.mean(kl32.astype(np.float64))))


def test_checker_gradient_against_finite_differences():
    rng = np.random.default_rng(7)
    n, m, k = 7, 40, 9
    Y, y = rng.normal(size=(m, 2)) * 3.0, rng.normal(size=(n, 2)) * 3.0
    idx, p = random_lists(rng, n, m, k)
    g = tsne.place_gradient_numpy(y, Y, idx, p)[0]
    h = 1e-6
    for c in (0, 1):
        e = np.zeros(2)
        e[c] = h
        fd = (tsne.place_gradient_numpy(y + e, Y, idx, p)[1] - tsne.place_gradient_numpy(y - e, Y, idx, p)[1]) / (2 * h)
        # d KL_i / d y_i = 2 (sum p w d - (sum p) sum w^2 d / Z_i) = g_i / 2 at e = 1 when the list's p sum to 1
        assert np.allclose(fd, g[:, c] / 2.0, rtol=0, atol=1e-7 + 1e-6 * np.abs(g[:, c]).max()), (fd, g[:, c])


def test_gradient_is_bounded_on_hostile_y():
    rng = np.random.default_rng(3)
    m, n, k = 300, 64, 31
    idx, p = random_lists(rng, n, m, k)
    for scale in (1e-4, 5.0, 1e4):
        for e in (1.0, 12.0):
            Y, y = rng.normal(size=(m, 2)) * scale, rng.normal(size=(n, 2)) * scale
            y[::5] = Y[idx[::5, 0]] + (rng.normal(size=(len(y[::5]), 2)))          # at distance about 1 of a neighbour: |w d| near 1/2
            g = tsne.place_gradient_numpy(y, Y, idx, p, e)[0]
            assert np.max(np.abs(g)) <= 2.0 * (e + 1.0)


def test_checker_is_independent_of_the_batch():
    Xf, lf, Yf, Xn, ln = small_fit()
    one = tsne.transform(Xn[:130], Xf, Yf, n_iter=20, backend="numpy", details=True)
    for b in (1, 7, 64):
        got = tsne.transform(Xn[:130], Xf, Yf, n_iter=20, batch=b, backend="numpy", details=True)
        assert all(np.array_equal(a, c) for a, c in zip(one, got))
    perm = np.random.default_rng(0).permutation(130)
    got = tsne.transform(Xn[:130][perm], Xf, Yf, n_iter=20, backend="numpy", details=True)
    assert all(np.array_equal(a[perm], c) for a, c in zip(one, got))


def test_init_rules_and_no_points():
    Xf, lf, Yf, Xn, ln = small_fit()
    d = tsne.transform(Xn[:9], Xf, Yf, n_iter=0, backend="numpy", details=True)
    want = np.zeros((9, 2))
    for j in range(d.idx.shape[1]):
        want = want + d.p[:, j, None] * Yf[d.idx[:, j]].astype(np.float64)
    assert np.array_equal(d.embedding, want.astype(np.float32)) and np.array_equal(d.kl, d.kl_init)
    assert d.idx.shape == (9, 91) and np.allclose(d.p.sum(axis=1), 1.0)
    near = tsne.transform(Xn[:9], Xf, Yf, n_iter=0, init="nearest", backend="numpy")
    assert np.array_equal(near, Yf[d.idx[:, 0]])
    given = np.arange(18, dtype=np.float32).reshape(9, 2)
    assert np.array_equal(tsne.transform(Xn[:9], Xf, Yf, n_iter=0, init=given, backend="numpy"), given)
    assert np.array_equal(tsne.transform(Xf, Xf, Yf, n_iter=0, init="nearest", backend="numpy"), Yf)       # each row lists itself
    e = tsne.transform(Xn[:0], Xf, Yf, backend="numpy", details=True)
    assert e.embedding.shape == (0, 2) and e.embedding.dtype == np.float32 and e.kl.shape == (0,) and e.idx.shape == (0, 91)
    assert tsne.transform(Xn[:0], Xf, Yf, backend="numpy").shape == (0, 2)


def bad_transform_cases():
    Xf, Yf, Xn = np.zeros((40, 3), np.float32), np.zeros((40, 2), np.float32), np.zeros((5, 3), np.float32)
    nan = Xn.copy()
    nan[2, 1] = np.nan
    inf = Yf.copy()
    inf[0, 0] = np.inf
    return [
        dict(X_fit=Xf[:39]), dict(Y_fit=np.zeros((40, 3), np.float32)), dict(X_new=np.zeros((5, 4), np.float32)),
        dict(X_new=np.zeros(5, np.float32)), dict(X_fit=Xf[:1], Y_fit=Yf[:1]), dict(perplexity=0.0), dict(perplexity=101.0),
        dict(perplexity=40.0), dict(perplexity="30"), dict(learning_rate=0.0), dict(learning_rate=float("inf")),
        dict(momentum=1.0), dict(momentum=-0.1), dict(exaggeration=0.5), dict(exaggeration=float("nan")), dict(n_iter=-1),
        dict(n_iter=2.5), dict(batch=0), dict(batch=262145), dict(init="pca"), dict(init=np.zeros((4, 2), np.float32)),
        dict(init=np.full((5, 2), np.nan, np.float32)), dict(X_new=nan), dict(Y_fit=inf), dict(backend="cuda"),
        dict(X_new=np.zeros((5, 2049), np.float32), X_fit=np.zeros((40, 2049), np.float32)),
    ]


@pytest.mark.parametrize("bad", range(len(bad_transform_cases())))
def test_transform_domain_errors(bad):
    args = dict(X_new=np.zeros((5, 3), np.float32), X_fit=np.zeros((40, 3), np.float32), Y_fit=np.zeros((40, 2), np.float32),
                perplexity=5.0, backend="numpy")
    args.update(bad_transform_cases()[bad])
    with pytest.raises(tsne.TsneError):
        tsne.transform(args.pop("X_new"), args.pop("X_fit"), args.pop("Y_fit"), **args)


def test_other_domain_errors():
    X = np.zeros((40, 3), np.float32)
    for Q, B, k in ((X[:0], X, 3), (X, X[:0], 1), (X, X, 0), (X, X, 41), (X, np.zeros((400, 3), np.float32), 302),
                    (X, np.zeros((40, 4), np.float32), 3), (X, X, 2.0)):
        with pytest.raises(tsne.TsneError):
            tsne.knn_query(Q, B, k, backend="numpy")
    for fit_size, n in ((1, 40), (41, 40), (2.0, 40)):
        with pytest.raises(tsne.TsneError):
            tsne.tsne_large(X[:n], fit_size, backend="numpy")
    with pytest.raises(tsne.TsneError):
        tsne.check_large_domain(tsne.MAX_NEW + 1, 100)
    with pytest.raises(tsne.TsneError):
        tsne.check_large_domain(300000, 262145)
    with pytest.raises(tsne.TsneError):                                   # the fit itself keeps its limit
        tsne.check_domain(262145, 3)
    idx, p = np.zeros((3, 2), np.int64), np.ones((3, 2))
    for a, b, c in ((idx, p, np.zeros(4)), (idx, p[:, :1], np.zeros(4, int)), (idx.astype(float), p, np.zeros(4, int)),
                    (idx, p, np.zeros((4, 1), int)), (idx, p, np.zeros(0, int))):
        with pytest.raises(tsne.TsneError):
            tsne.vote_labels(a, b, c)


def test_vote_labels():
    labels = np.array([3, -1, 7, 3, -1, 9])
    idx = np.array([[0, 1, 2], [1, 2, 4], [2, 0, 3], [5, 1, 0], [5, 6, -1]])
    p = np.array([[0.25, 0.5, 0.25],      # 3: .25, -1: .5, 7: .25 -> noise wins: -1 competes
                  [0.25, 0.5, 0.25],      # -1: .25 + .25 = .5, 7: .5 -> a tie: the lowest label, -1
                  [0.5, 0.25, 0.25],      # 7: .5, 3: .25 + .25 = .5 -> a tie: 3
                  [0.125, 0.125, 0.75],   # 9, -1, 3 -> 3 with .75
                  [0.5, 0.3, 0.2]])       # entries 6 and -1 are outside the fitted rows: skipped
    lab, conf = tsne.vote_labels(idx, p, labels)
    assert lab.dtype == np.int32 and conf.dtype == np.float64
    assert np.array_equal(lab, [-1, -1, 3, 3, 9]) and np.array_equal(conf, [0.5, 0.5, 0.5, 0.75, 0.5])
    e = tsne.vote_labels(np.zeros((0, 3), np.int64), np.zeros((0, 3)), labels)
    assert e[0].shape == (0,) and e[1].shape == (0,)
    # the confidence is the sum in list order, in double
    q = np.array([[0.1, 0.2, 0.3, 0.4]])
    lab, conf = tsne.vote_labels(np.array([[0, 3, 3, 0]]), q, labels)
    assert lab[0] == 3 and conf[0] == ((0.1 + 0.2) + 0.3) + 0.4


def test_tsne_large_draw_and_fitted_rows():
    X, lab = clusters(90, 6, 4)
    r = tsne.tsne_large(X, 60, random_state=5, transform_kwargs=dict(n_iter=30, perplexity=8.0), perplexity=8.0, max_iter=250,
                        backend="numpy")
    want = np.array(sorted(np.random.RandomState(5).permutation(90)[:60]))
    assert np.array_equal(r.fit_indices, want) and np.array_equal(tsne.draw_fit_rows(90, 60, 5), want)
    fit = tsne.tsne(X[want], perplexity=8.0, max_iter=250, random_state=5, backend="numpy")
    assert np.array_equal(r.embedding[want], fit.embedding) and np.array_equal(r.fit.embedding, fit.embedding)
    rest = np.setdiff1d(np.arange(90), want)
    assert np.all(np.isnan(r.kl_point[want])) and np.all(np.isfinite(r.kl_point[rest])) and r.embedding.shape == (90, 2)
    placed = tsne.transform(X[rest], X[want], fit.embedding, n_iter=30, perplexity=8.0, backend="numpy", details=True)
    assert np.array_equal(r.embedding[rest], placed.embedding) and np.array_equal(r.kl_point[rest], placed.kl)
    full = tsne.tsne_large(X, 90, random_state=5, perplexity=8.0, max_iter=250, backend="numpy")            # nothing to place
    assert np.all(np.isnan(full.kl_point)) and np.array_equal(full.fit_indices, np.arange(90))


def test_prototype_property():
    """mean KL_i falls and no point ends above its start (the defaults, m = 600, n = 400)"""
    d = small_placed()
    print("KL_i mean %.6f -> %.6f, worse %d" % (d.kl_init.mean(), d.kl.mean(), int(np.sum(d.kl > d.kl_init))))
    assert d.kl.mean() < d.kl_init.mean() and not np.any(d.kl > d.kl_init)
    Xf, lf, Yf, Xn, ln = small_fit()
    lab, conf = tsne.vote_labels(d.idx, d.p, lf)
    assert np.mean(lab == ln) > 0.95 and np.all((conf > 0) & (conf <= 1.0 + 1e-12))
    y0 = tsne.initial_placement_numpy("weighted", Yf, d.idx, d.p)
    assert checker_margin(y0, Yf, d.idx, d.p, d.kl) > 0.0


# ---- 6. the tool

def run_tool(*argv, cwd=None):
    return subprocess.run([sys.executable, "-m", "cryo_ralib_amd.tsne"] + [str(a) for a in argv], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def tool_files(tmp_path_factory):
    t = tmp_path_factory.mktemp("place")
    X, lab = clusters(60, 5, 8)
    np.save(t / "new.npy", X[40:])
    np.save(t / "all.npy", X)
    np.savez(t / "fit_in.npz", factors=X[:40])
    np.save(t / "fit_wide.npy", np.zeros((40, 6), np.float32))
    np.save(t / "fit_short.npy", X[:39])
    np.savez(t / "fit_out.npz", embedding=np.random.default_rng(0).normal(size=(40, 2)).astype(np.float32), perplexity=np.float64(5.0))
    np.save(t / "labels.npy", lab[:40])
    np.savez(t / "labels_tool.npz", labels=lab[:40].astype(np.int32), inertia=np.float64(1.0))
    np.save(t / "labels_short.npy", lab[:39])
    return t


def test_tool_usage_errors_exit_with_status_2(tool_files):
    t = tool_files
    new, allx, out = t / "new.npy", t / "all.npy", t / "o.npz"
    cases = [
        [allx, out, "--fit_size", 40, "--place_into", t / "fit_out.npz", "--fit_input", t / "fit_in.npz"],   # both modes
        [new, out, "--place_into", t / "fit_out.npz"],                                                      # no --fit_input
        [new, out, "--place_into", t / "fit_out.npz", "--fit_input", t / "fit_short.npy"],                  # rows disagree
        [new, out, "--place_into", t / "fit_out.npz", "--fit_input", t / "fit_wide.npy"],                   # features disagree
        [new, out, "--place_into", t / "fit_out.npz", "--fit_input", t / "fit_in.npz", "--fit_labels", t / "labels_short.npy"],
        [allx, out, "--fit_size", 40, "--fit_labels", t / "labels_short.npy"],
        [allx, out, "--fit_labels", t / "labels.npy"], [allx, out, "--place_iter", 10], [allx, out, "--place_lr", 0.5],
        [allx, out, "--place_exaggeration", 2], [allx, out, "--place_perplexity", 5], [allx, out, "--fit_input", t / "fit_in.npz"],
        [allx, out, "--fit_size", 1], [allx, out, "--fit_size", 61], [allx, out, "--fit_size", -3],
    ]
    for argv in cases:
        r = run_tool(*argv, "--backend", "numpy", "--perplexity", 5)
        assert r.returncode == 2 and "usage:" in r.stderr, (argv, r.returncode, r.stderr)
        assert not out.exists()


def test_tool_modes_on_the_numpy_backend(tool_files):
    t = tool_files
    X, lab = clusters(60, 5, 8)
    out = t / "placed.npz"
    r = run_tool(t / "new.npy", out, "--place_into", t / "fit_out.npz", "--fit_input", t / "fit_in.npz", "--place_iter", 20,
                 "--fit_labels", t / "labels_tool.npz", "--backend", "numpy")
    assert r.returncode == 0, r.stderr
    o = np.load(out)
    assert sorted(o.files) == ["embedding", "kl_point", "label_confidence", "labels"]
    Yf = np.load(t / "fit_out.npz")["embedding"]
    d = tsne.transform(X[40:], X[:40], Yf, perplexity=5.0, n_iter=20, backend="numpy", details=True)        # the stored perplexity
    assert np.array_equal(o["embedding"], d.embedding) and np.array_equal(o["kl_point"], d.kl)
    want = tsne.vote_labels(d.idx, d.p, lab[:40])
    assert np.array_equal(o["labels"], want[0]) and np.array_equal(o["label_confidence"], want[1])
    out2 = t / "large.npz"
    r = run_tool(t / "all.npy", out2, "--fit_size", 40, "--seed", 2, "--perplexity", 5, "--max_iter", 250, "--place_iter", 20,
                 "--fit_labels", t / "labels.npy", "--backend", "numpy")
    assert r.returncode == 0, r.stderr
    o = np.load(out2)
    big = tsne.tsne_large(X, 40, random_state=2, transform_kwargs=dict(perplexity=5.0, n_iter=20), perplexity=5.0, max_iter=250,
                          backend="numpy")
    assert np.array_equal(o["fit_indices"], big.fit_indices) and np.array_equal(o["embedding"], big.embedding)
    assert np.array_equal(o["kl_point"], big.kl_point, equal_nan=True) and o["labels"].shape == (60,)
    old = {"embedding", "kl_divergence", "n_iter", "errors", "perplexity", "early_exaggeration", "learning_rate", "max_iter", "init",
           "seed", "backend"}
    assert set(o.files) == old | {"fit_indices", "kl_point", "labels", "label_confidence"}
    # every row votes among the fitted rows' labels; a fitted row lists itself first
    idx, p = tsne.affinities_query(X, X[big.fit_indices], 5.0, backend="numpy")
    assert np.array_equal(idx[big.fit_indices, 0], np.arange(40))
    want = tsne.vote_labels(idx, p, lab[:40])
    assert np.array_equal(o["labels"], want[0]) and np.array_equal(o["label_confidence"], want[1])


def test_old_command_line_is_unchanged(tool_files):
    t = tool_files
    out = t / "plain.npz"
    r = run_tool(t / "all.npy", out, "--backend", "numpy", "--perplexity", 5, "--max_iter", 250, "--init", "random", "--seed", 3)
    assert r.returncode == 0, r.stderr
    o = np.load(out)
    assert o.files == ["embedding", "kl_divergence", "n_iter", "errors", "perplexity", "early_exaggeration", "learning_rate",
                       "max_iter", "init", "seed", "backend"]
    X = np.load(t / "all.npy")
    want = tsne.tsne(X, 5.0, max_iter=250, init="random", random_state=3, backend="numpy")
    assert np.array_equal(o["embedding"], want.embedding) and int(o["n_iter"]) == want.n_iter
    assert r.stdout.strip() == "%s: 60 points x 5, %d iterations, KL %.6f" % (out, want.n_iter, want.kl_divergence)
    bad = run_tool(t / "all.npy", out, "--backend", "numpy", "--perplexity", 500)
    assert bad.returncode == 1 and bad.stderr.startswith("error: ") and "perplexity" in bad.stderr
