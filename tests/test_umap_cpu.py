"""The float64 checker of cryo_ralib_amd.umap (backend="numpy") against literal restatements of its rules, the whole fit on the
issue's prototype case, the out-of-sample placement, the conditions the builders of tests/umap_cases.py promise to the GPU file, and
the tool's usage errors.  No GPU."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import umap_cases as uc
from cryo_ralib_amd import _graph, tsne, umap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1


# ---- rule 4

def test_find_ab_pin():
    a, b = umap.find_ab(1.0, 0.1)
    assert abs(a - 1.5769434603) <= 1e-6 * 1.5769434603
    assert abs(b - 0.8950608779) <= 1e-6 * 0.8950608779


# ---- rule 2 against a scalar restatement

def scalar_smooth(d2row, n_neighbors):
    d = [math.sqrt(v) for v in d2row]
    nz = [v for v in d if v > 0]
    rho = min(nz) if nz else 0.0
    target = math.log2(n_neighbors)

    def psum(sig):
        s = 0.0
        for v in d:
            x = v - rho
            s += math.exp(-x / sig) if x > 0 else 1.0
        return s
    lo, hi, mid, stopped = 0.0, math.inf, 1.0, False
    for _ in range(64):
        ps = psum(mid)
        if abs(ps - target) < 1e-5:
            stopped = True
            break
        if ps > target:
            hi = mid
            mid = (lo + hi) / 2
        else:
            lo = mid
            mid = mid * 2 if hi == math.inf else (lo + hi) / 2
    mean = 0.0
    for v in d:
        mean += v
    mean /= len(d)
    sigma = max(mid, 1e-3 * mean)
    w = [1.0 if (v - rho <= 0 or sigma == 0) else math.exp(-(v - rho) / sigma) for v in d]
    return rho, sigma, w, stopped, psum(sigma), 1e-3 * mean > mid


@pytest.fixture(scope="module")
def smooth():
    return {name: (d2, nn, umap.smooth_knn_numpy(d2, nn)) for name, (d2, nn) in uc.smooth_cases().items()}


@pytest.mark.parametrize("name", ["k2", "k14", "k65", "query", "special"])
def test_smooth_knn_matches_scalar_restatement(smooth, name):
    d2, nn, sk = smooth[name]
    target = math.log2(nn)
    for i in range(d2.shape[0]):
        rho, sigma, w, stopped, ps, floored = scalar_smooth(d2[i], nn)
        assert sk.rho[i] == rho and bool(sk.stopped[i]) == stopped and bool(sk.floored[i]) == floored
        assert abs(sk.sigma[i] - sigma) <= 1e-12 * sigma                # math.exp and numpy.exp may differ by an ulp near a branch
        np.testing.assert_allclose(sk.w[i], w, rtol=1e-9, atol=0)
        if stopped and not floored:
            assert abs(ps - target) < 1e-5
        d = np.sqrt(d2[i])
        first = np.nonzero(d > 0)[0]
        if len(first):
            assert sk.w[i, first[0]] == 1.0                             # the first non-duplicate neighbour


def test_smooth_knn_special_rows(smooth):
    d2, nn, sk = smooth["special"]
    assert sk.rho[0] == 0.0 and np.all(sk.w[0] == 1.0)                  # all duplicates
    assert np.all(sk.w[1, :3] == 1.0) and sk.rho[1] == np.sqrt(d2[1, 3])
    assert sk.floored[2] and not sk.stopped[2]                          # six rows at the least distance: the floor, 64 trips
    assert sk.stopped[3] and sk.sigma[3] > 1e5                          # many doublings
    assert sk.stopped[4] and sk.sigma[4] < 1e-5


def test_builder_smooth_margins(smooth):
    for name, (d2, nn, sk) in smooth.items():
        if name == "special":
            continue
        assert np.mean(sk.margin < uc.MARGIN) <= uc.MAX_LEFT_OUT, name
    d2, nn, sk = smooth["special"]
    assert np.all(sk.margin >= uc.MARGIN)


# ---- rule 3

def test_fuzzy_union_is_symmetric_and_matches_dense():
    X, _ = uc.blobs(200, 5, 3, 1)
    indptr, indices, s, rho, sigma = umap.fuzzy_graph(X, 10, backend="numpy")
    n = 200
    idx, d2 = tsne.knn_numpy(X, 9)
    W = np.zeros((n, n))
    W[np.repeat(np.arange(n), 9), idx.reshape(-1)] = umap.smooth_knn_numpy(d2, 10).w.reshape(-1)
    S = np.zeros((n, n))
    rows = _graph.row_ids_numpy(indptr.astype(np.int64))
    S[rows, indices] = s
    assert np.array_equal(S, S.T)                                       # bit for bit
    assert np.all(s >= 0) and np.all(s <= 1)
    keys = rows * n + indices
    assert np.all(np.diff(keys) > 0)                                    # ascending columns, no duplicates
    np.testing.assert_allclose(S, W + W.T - W * W.T, rtol=1e-15, atol=0)
    assert np.array_equal(S > 0, (W + W.T) > 0)


# ---- rule 5

def test_schedule():
    E = 37
    r = np.array([1.0, np.nextafter(1.0 / E, 0.0), 0.5, 0.31, 1.0 / 3.0, 0.999])
    count = np.zeros(len(r), int)
    for t in range(1, E + 1):
        f = umap.fires(r, t)
        assert f[0]
        assert not f[1]
        count += f
    assert np.array_equal(count, np.floor(E * r).astype(int))
    assert umap.alpha_at(2.0, 1, E) == 2.0 and umap.alpha_at(2.0, E, E) == 2.0 * (1.0 - (E - 1) / E)
    assert np.array_equal(umap.rates(np.array([0.5, 0.25, 0.125])), [1.0, 0.5, 0.25])


# ---- rule 6's generator

def splitmix(z):
    """pure Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def test_splitmix_is_the_published_generator():
    # the first outputs of splitmix64 seeded with 0 and 1234567 (Vigna's splitmix64.c: the state advances by the golden gamma)
    assert splitmix(0) == 0xE220A8397B1DCDAF
    assert splitmix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert splitmix(1234567) == 6457827717110365317


def test_samples_match_python_integers():
    seed, t, p, n = 42, 7, 123456, 50000
    want = []
    for s in range(8):
        z = splitmix((seed * 0xD1342543DE82EF95 + t * 0xA0761D6478BD642F + 16 * p + s) & MASK)
        want.append(((z >> 32) * n) >> 32)
    # written out: the values of the pure-Python restatement above for (42, 7, 123456), n = 50000
    assert want == PINNED_SAMPLES
    got = [int(umap.draw(seed, t, np.array([p]), s, n)[0]) for s in range(8)]
    assert got == want
    big = umap.draw(2 ** 32 - 1, 10000, np.arange(0, 2 ** 31, 9999991, dtype=np.int64), 15, 262144)
    assert big.min() >= 0 and big.max() < 262144
    assert np.all(umap.draw(1, 1, np.arange(1000), 0, 4) < 4)


PINNED_SAMPLES = [17189, 14845, 31830, 38589, 17861, 33826, 23445, 46744]


# ---- rule 6

def scalar_epoch(case, t, seed=42, gamma=1.0, lr=1.0):
    """rule 6 with Python floats: per lane in walk order, then the xor tree"""
    a, b, n = uc.A, uc.B, case.n
    Y = case.Y.astype(np.float64)
    key = (seed * 0xD1342543DE82EF95 + t * 0xA0761D6478BD642F) & MASK
    alpha = lr * (1.0 - (t - 1) / case.n_epochs)
    out = np.empty_like(case.Y)

    def clip(v):
        return max(-4.0, min(4.0, v))
    for i in range(n):
        acc = [[0.0, 0.0] for _ in range(16)]
        for p in range(case.indptr[i], case.indptr[i + 1]):
            r = case.rate[p]
            if not math.floor(t * r) > math.floor((t - 1) * r):
                continue
            lane = acc[(p - case.indptr[i]) % 16]
            j = case.indices[p]
            dx, dy = Y[i, 0] - Y[j, 0], Y[i, 1] - Y[j, 1]
            q = dx * dx + dy * dy
            if q > 0:
                qb = q ** b
                c = ((-2.0 * a) * b * qb / q) / (1.0 + a * qb)
                lane[0] += 2.0 * clip(c * dx)
                lane[1] += 2.0 * clip(c * dy)
            for s in range(case.neg):
                z = splitmix((key + 16 * p + s) & MASK)
                k = ((z >> 32) * n) >> 32
                if k == i:
                    continue
                dx, dy = Y[i, 0] - Y[k, 0], Y[i, 1] - Y[k, 1]
                q = dx * dx + dy * dy
                if q > 0:
                    c = ((2.0 * gamma) * b) / ((0.001 + q) * (1.0 + a * q ** b))
                    lane[0] += clip(c * dx)
                    lane[1] += clip(c * dy)
                else:
                    lane[0] += 4.0
                    lane[1] += 4.0
        for c in range(2):
            v = [lane[c] for lane in acc]
            for m in (8, 4, 2, 1):
                v = [v[l] + v[l ^ m] for l in range(16)]
            out[i, c] = np.float32(Y[i, c] + alpha * v[0])
    return out


@pytest.fixture(scope="module")
def epoch_cases():
    return uc.epoch_cases()


@pytest.mark.parametrize("name,t", [("n33", 1), ("n4", 3), ("n17", 20), ("neg16", 2), ("neg0", 5)])
def test_epoch_matches_scalar_restatement(epoch_cases, name, t):
    case = epoch_cases[name]
    ref, lit = case.reference(t), scalar_epoch(case, t)
    # numpy's and Python's pow may differ by an ulp: the double sums agree to ~1e-15, so the float32 roundings differ by one ulp at most
    assert np.all(np.abs(ref.astype(np.float64) - lit) <= uc.ulp32(lit))
    assert np.mean(ref != lit) < 0.01
    assert not np.array_equal(ref, case.Y)


def test_epoch_edges_case_matches_scalar_restatement(epoch_cases):
    case = epoch_cases["edges"]
    ref, lit = case.reference(2), scalar_epoch(case, 2)
    assert np.all(np.abs(ref.astype(np.float64) - lit) <= uc.ulp32(lit))


def test_builder_epoch_conditions(epoch_cases):
    for name, case in epoch_cases.items():
        Y = case.Y.astype(np.float64)
        rows = _graph.row_ids_numpy(case.indptr.astype(np.int64))
        cols = case.indices.astype(np.int64)
        q_att = np.sum((Y[rows] - Y[cols]) ** 2, axis=1)
        assert not np.any((q_att > 0) & (q_att < uc.Q_MIN)), name
        zero_rep = clipped_rep = hit_self = 0
        for t in (1, 2, case.n_epochs):
            f = umap.fires(case.rate, t)
            for s in range(case.neg):
                k = umap.draw(42, t, np.arange(len(rows)), s, case.n)
                d = Y[rows] - Y[k]
                q = np.sum(d ** 2, axis=1)
                assert not np.any((q > 0) & (q < uc.Q_MIN)), name
                other = f & (k != rows)
                hit_self += int(np.sum(f & (k == rows)))
                zero_rep += int(np.sum(other & (q == 0)))
                qs = np.where(q > 0, q, 1.0)
                g = 2.0 * uc.B / ((0.001 + qs) * (1.0 + uc.A * qs ** uc.B))
                clipped_rep += int(np.sum(other & (q > 0) & (np.abs(g[:, None] * d).max(axis=1) > 4.0)))
        if name in ("edges", "n33", "neg1", "neg16"):
            # the states the GPU file relies on, each on a firing entry or a drawn pair of the tested epochs
            e = case.state_entries
            assert np.all(case.rate[e] == 1.0)
            assert q_att[e[0]] == 0.0 and q_att[e[1]] == 2.0 ** -14 and q_att[e[2]] == 1e6
            assert zero_rep > 0 and clipped_rep > 0, (name, zero_rep, clipped_rep)
        if name == "n4":
            assert hit_self > 0                                         # negatives that draw the vertex itself
        for t in (1, 2, case.n_epochs):
            ref = case.reference(t)
            # a double value off by the bound changes the float32 rounding by one ulp at most
            assert np.all(uc.epoch_bound(case, t)[:, None] < 0.5 * uc.ulp32(ref)), (name, t)
        f = [umap.fires(case.rate, t) for t in range(1, case.n_epochs + 1)]
        assert np.any(np.all(f, axis=0)) and np.any(~np.any(f, axis=0)) or len(case.rate) < 8


def test_epoch_seeds_differ(epoch_cases):
    case = epoch_cases["n33"]
    assert not np.array_equal(case.reference(1, seed=1), case.reference(1, seed=2))
    assert np.array_equal(case.reference(1, seed=1), case.reference(1, seed=1))


# ---- the whole fit

@pytest.fixture(scope="module")
def blob_fit():
    X, truth = uc.blobs()
    return X, truth, umap.umap(X, n_neighbors=15, n_epochs=200, init="pca", backend="numpy")


def test_whole_fit_prototype_case(blob_fit):
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score, silhouette_score
    X, truth, res = blob_fit
    Y = res.embedding
    assert Y.shape == (1500, 2) and Y.dtype == np.float32 and np.all(np.isfinite(Y))
    assert res.init == "pca" and res.n_epochs == 200
    again = umap.umap(X, n_neighbors=15, n_epochs=200, init="pca", backend="numpy").embedding
    assert np.array_equal(Y, again)
    labels = KMeans(6, n_init=10, random_state=0).fit(Y).labels_
    assert adjusted_rand_score(truth, labels) == 1.0
    assert silhouette_score(Y, truth) > silhouette_score(X, truth)


def test_layout_in_pieces_is_the_same(blob_fit):
    X, truth, res = blob_fit
    indptr, indices, s = res.graph
    Y0 = umap.pca_start(X)
    kw = dict(a=res.a, b=res.b, n_epochs=12, backend="numpy")
    whole = umap.layout(indptr, indices, s, Y0, **kw)
    Y = Y0
    for e0 in (1, 5, 9):
        Y = umap.layout(indptr, indices, s, Y, epoch0=e0, count=4, **kw)
    assert np.array_equal(whole, Y)


@pytest.mark.parametrize("n", [4, 17])
def test_small_inputs_stay_finite(n):
    X = np.random.RandomState(n).standard_normal((n, 3)).astype(np.float32)
    for init in ("pca", "spectral", "random"):
        res = umap.umap(X, n_neighbors=min(n, 15), n_epochs=30, init=init, backend="numpy")
        assert np.all(np.isfinite(res.embedding))


def test_duplicate_rows_stay_finite():
    X = np.repeat(np.random.RandomState(3).standard_normal((5, 4)).astype(np.float32), 8, axis=0)
    res = umap.umap(X, n_neighbors=15, n_epochs=30, init="pca", backend="numpy")
    assert np.all(np.isfinite(res.embedding))


def test_disconnected_graph_warns_once_and_takes_pca(blob_fit):
    X, _, _ = blob_fit
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = umap.umap(X[:300], n_neighbors=5, n_epochs=2, backend="numpy")
    mine = [w for w in seen if issubclass(w.category, umap.UmapWarning)]
    assert len(mine) == 1 and "connected components" in str(mine[0].message) and res.init == "pca"


def test_start_rescale():
    F = np.array([[1.0, 3.0], [2.0, 3.0], [5.0, 3.0]])
    assert np.array_equal(umap.rescale(F), np.array([[0.0, 5.0], [2.5, 5.0], [10.0, 5.0]], np.float32))
    Y0 = umap.initial_embedding(np.zeros((6, 3), np.float32), None, "random", 42)[0]
    assert np.array_equal(Y0, np.random.RandomState(42).uniform(-10, 10, (6, 2)).astype(np.float32))


def test_domain():
    X = np.zeros((10, 3), np.float32)
    for kw in (dict(n_neighbors=1), dict(n_neighbors=11), dict(min_dist=2.0), dict(n_epochs=0), dict(n_epochs=10001),
               dict(negative_sample_rate=17), dict(learning_rate=0.0), dict(repulsion_strength=-1.0), dict(init="nope"),
               dict(random_state=-1), dict(a=1.0)):
        with pytest.raises(umap.UmapError):
            umap.umap(X, backend="numpy", **kw)
    with pytest.raises(umap.UmapError):
        umap.umap(np.zeros((3, 3), np.float32), n_neighbors=2, backend="numpy")
    with pytest.raises(umap.UmapError):
        umap.umap(np.zeros((10, 1), np.float32), init="pca", backend="numpy")
    bad = X.copy()
    bad[0, 0] = np.nan
    with pytest.raises(umap.UmapError):
        umap.umap(bad, backend="numpy")
    assert umap.transform(np.zeros((0, 3), np.float32), X, np.zeros((10, 2), np.float32), backend="numpy").shape == (0, 2)
    with pytest.raises(umap.UmapError):
        umap.transform(X, X[:1], np.zeros((1, 2), np.float32), backend="numpy")
    umap.check_transform_domain(2 ** 48, 10, 3)
    with pytest.raises(umap.UmapError):
        umap.check_transform_domain(2 ** 48 + 1, 10, 3)


def test_place_checker_far_rows():
    """the checker's key index at the last rows the domain takes: the samples are those of Python integers"""
    row0, k, m, t = 2 ** 48 - 3, 15, 80, 2
    p = (row0 + np.arange(3)) * k + 7
    for s in (0, 15):
        want = [((splitmix((42 * 0xD1342543DE82EF95 + t * 0xA0761D6478BD642F + 16 * int(v) + s) & MASK) >> 32) * m) >> 32 for v in p]
        assert umap.draw(42, t, p, s, m).tolist() == want


# ---- rule 8

def test_transform(blob_fit):
    X, truth, res = blob_fit
    fit, held = np.arange(100, 1500), np.arange(0, 100)
    Yf = np.ascontiguousarray(res.embedding[fit])
    kw = dict(a=res.a, b=res.b, n_epochs=30, backend="numpy")
    det = umap.transform(X[held], X[fit], Yf, details=True, **kw)
    assert np.all(np.isfinite(det.embedding)) and det.idx.shape == (100, 15)
    for batch in (1, 7, 64):
        assert np.array_equal(umap.transform(X[held], X[fit], Yf, batch=batch, **kw), det.embedding)
    labels, conf = tsne.vote_labels(det.idx, det.w, truth[fit])
    assert np.array_equal(labels, truth[held])
    # a new row equal to a fitted row lists it first and starts at a mean dominated by it
    same = umap.transform(X[fit][:5], X[fit], Yf, details=True, **kw)
    assert np.array_equal(same.idx[:, 0], np.arange(5))
    assert np.all(same.w[:, 0] == 1.0) and np.all(same.w[:, 0] >= same.w.max(axis=1))
    near = np.linalg.norm(same.start - Yf[:5], axis=1)
    spread = np.linalg.norm(Yf[same.idx[:, 1:]] - Yf[:5, None], axis=2).max(axis=1)
    assert np.all(near <= spread)


# ---- the tool

def tool(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "cryo_ralib_amd.umap", *args, "--backend", "numpy"], capture_output=True, text=True,
                          env=env)


def test_tool_usage_errors_and_a_run(tmp_path):
    X, truth = uc.blobs(120, 4, 3, 5)
    a, b, out = str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), str(tmp_path / "out.npz")
    np.save(a, X)
    np.save(b, X[:, :3])
    np.save(str(tmp_path / "lab.npy"), truth.astype(np.int64))
    ok = tool(a, out, "--n_epochs", "20", "--init", "pca", "--quality", "5")
    assert ok.returncode == 0, ok.stderr
    with np.load(out) as z:
        assert z["embedding"].shape == (120, 2) and z["embedding"].dtype == np.float32 and str(z["init"]) == "pca"
        assert int(z["n_epochs"]) == 20 and 0.0 < float(z["trustworthiness"]) <= 1.0
        assert {"a", "b", "n_neighbors", "seed", "continuity"} <= set(z.files)
    placed = str(tmp_path / "placed.npz")
    ok = tool(a, placed, "--place_into", out, "--fit_input", a, "--fit_labels", str(tmp_path / "lab.npy"), "--n_epochs", "5")
    assert ok.returncode == 0, ok.stderr
    with np.load(placed) as z:
        assert np.array_equal(z["labels"], truth)
    for bad in ([a, out, "--place_into", out],
                [b, out, "--place_into", out, "--fit_input", a],
                [a, out, "--fit_labels", str(tmp_path / "lab.npy")],
                [a, out, "--batch", "10"],
                [a, out, "--n_neighbors", "1"],
                [a, out, "--n_neighbors", "500"],
                [a, out, "--min_dist", "3"],
                [a, out, "--negative_sample_rate", "17"],
                [a, out, "--init", "pca", "--n_epochs", "0"]):
        r = tool(*bad)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
