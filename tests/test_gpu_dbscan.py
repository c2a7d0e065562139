"""DBSCAN on the device (ra_dbscan_count / ra_dbscan_step behind dbscan.dbscan, ra_tsne_knn behind dbscan.kdistances): every
scikit-learn 1.7 pin of tests/golden/dbscan_ref.npz, the shapes around the kernel's tiles and the column list's padding against the
float64 numpy backend, unquantised data, the edge inputs, the last round's contract, bitwise repeatability, the C entries'
rejections and the tool.

Every comparison is an equality.  The pins and the generated cases are quantised to 1/64 with eps a multiple of 1/16: every term
of D2 and eps^2 are exact in double, so the device's fused multiply-adds and numpy's unfused ones decide alike.  The unquantised
case first asserts, on the CPU, that no pair lies within d 2^-50 eps^2 of eps^2 (the two chains differ by at most d 2^-52 D2)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, dbscan, kmeans  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan_ref.npz")
CASES = "abcdefgh"
TC = 64             # the kernel's row and column tiles (csrc/ralign_dbscan.h)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def case(z, c):
    return z["X_" + c], float(z["eps_" + c]), int(z["min_samples_" + c])


def q64(v):
    return (np.round(np.asarray(v, np.float64) * 64) / 64).astype(np.float32)


def same(r, ref):
    return (np.array_equal(r.labels, ref.labels) and np.array_equal(r.core_mask, ref.core_mask) and np.array_equal(r.counts, ref.counts)
            and r.n_clusters == ref.n_clusters)


def check_against_numpy(X, eps, ms, dev, what):
    r = dbscan.dbscan(torch.from_numpy(X).to(dev), eps, ms)
    ref = dbscan.dbscan(X, eps, ms, backend="numpy")
    print("%s: n = %d, d = %d, eps = %g, min_samples = %d: %d clusters, %d core, %d noise, %d rounds; labels differ at %d, counts at %d" % (
        what, X.shape[0], X.shape[1], eps, ms, r.n_clusters, r.core_mask.sum(), r.n_noise, r.n_rounds,
        np.count_nonzero(r.labels != ref.labels), np.count_nonzero(r.counts != ref.counts)))
    assert r.labels.dtype == np.int32 and r.counts.dtype == np.int32 and r.core_mask.dtype == np.bool_
    assert same(r, ref)
    return r


@pytest.mark.parametrize("c", CASES)
def test_device_equals_sklearn(dev, z, c):
    X, eps, ms = case(z, c)
    r = check_against_numpy(X, eps, ms, dev, "pin " + c)
    assert np.array_equal(r.labels, z["labels_" + c])
    assert np.array_equal(r.core_sample_indices, z["core_sample_indices_" + c])
    assert r.n_clusters == int(z["labels_" + c].max()) + 1


def tile_case(n, d, seed):
    """quantised points, and an eps (a multiple of 1/16) near the median distance to the second nearest other point: with
    min_samples = 3 that leaves core, border and noise points"""
    X = q64(np.random.default_rng(seed).normal(size=(n, d)))
    if n < 3:
        return X, 1.0
    kd = dbscan.kdistances(X, 3, backend="numpy")
    return X, max(1, int(np.ceil(np.median(kd) * 16))) / 16.0


@pytest.mark.parametrize("d", [1, 2, 3, 31, 32, 33, 65])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 129, 257])
def test_shapes_around_the_tiles(dev, n, d):
    X, eps = tile_case(n, d, 1000 * n + d)
    r = check_against_numpy(X, eps, 3, dev, "shape")
    if n >= 63 and d >= 2:
        assert 0 < r.core_mask.sum() < n        # continuous data: the median rule leaves both kinds (d = 1 has many ties)
    if n < 3:
        assert r.n_noise == n and same(dbscan.dbscan(torch.from_numpy(X).to(dev), eps, 1), dbscan.dbscan(X, eps, 1, backend="numpy"))


@pytest.mark.parametrize("m", [TC - 1, TC, TC + 1, 2 * TC])
def test_core_count_at_the_column_padding(dev, m):
    """exactly m core points (a line at spacing 1/8 with eps 1/2, min_samples 4), one border point at exactly eps from the line's
    end and three noise points, rows shuffled: the compacted core list is m long, padded to the column tile"""
    line = np.arange(m) / 8.0
    x = np.concatenate([line, [line[-1] + 0.5, 100.0, 200.0, 300.0]])
    perm = np.random.default_rng(m).permutation(len(x))
    X = np.stack([x, np.zeros_like(x)], axis=1).astype(np.float32)[perm]
    r = check_against_numpy(X, 0.5, 4, dev, "padding")
    assert r.core_mask.sum() == m and r.n_noise == 3 and r.n_clusters == 1
    assert r.labels[np.argsort(perm)][m] == 0 and not r.core_mask[np.argsort(perm)][m]


def test_unquantised_data(dev):
    n, d = 1000, 50
    X = np.random.default_rng(2024).normal(size=(n, d)).astype(np.float32)
    eps = float(np.quantile(dbscan.kdistances(X, 5, backend="numpy"), 0.6))
    Xd = X.astype(np.float64)
    D2 = np.zeros((n, n))
    for t in range(d):
        df = Xd[:, t, None] - Xd[None, :, t]
        D2 += df * df
    gap = np.abs(D2 - eps * eps).min()
    print("unquantised: eps = %.17g, least |D2 - eps^2| = %.3g, excluded band %.3g" % (eps, gap, d * 2.0 ** -50 * eps * eps))
    assert gap > d * 2.0 ** -50 * eps * eps          # a condition of the test: no decision can depend on the fusing
    r = check_against_numpy(X, eps, 5, dev, "unquantised")
    assert 0 < r.core_mask.sum() < n


def test_edge_inputs(dev):
    rng = np.random.default_rng(8)
    X = q64(rng.normal(size=(300, 4)))
    r = check_against_numpy(X, 0.5, 1, dev, "min_samples = 1")
    assert r.core_mask.all() and r.n_noise == 0
    r = check_against_numpy(X, 0.0625, 2, dev, "all noise")
    assert r.n_clusters == 0 and r.n_noise == 300 and r.n_rounds == 1 and np.all(r.counts == 1)
    r = check_against_numpy(X, 1.0, 301, dev, "min_samples > n")
    assert r.n_noise == 300 and r.n_rounds == 1
    r = check_against_numpy(np.full((130, 5), 1.25, np.float32), 0.5, 5, dev, "identical points")
    assert np.all(r.labels == 0) and np.all(r.counts == 130) and r.core_mask.all()
    r = check_against_numpy(X, 1000.0, 300, dev, "everything within eps")
    assert np.all(r.labels == 0) and np.all(r.counts == 300)


def test_border_point_takes_the_lower_cluster(dev):
    """two far clusters and one border point at exactly eps from a core point of each: the cluster numbered first wins"""
    hi, lo, mid = [[10.0], [10.25], [10.5], [10.75]], [[8.0], [7.75], [7.5], [7.25]], [[9.0]]
    for first, second in ((hi, lo), (lo, hi)):
        r = check_against_numpy(np.array(first + mid + second, np.float32), 1.0, 4, dev, "border")
        assert r.labels.tolist() == [0] * 5 + [1] * 4 and not r.core_mask[4] and r.counts[4] == 3


def test_chains(dev):
    """1000 points at a spacing of exactly eps: in index order, reversed and shuffled, always one cluster"""
    x = (np.arange(1000) * 0.25).astype(np.float32)
    for what, order in (("chain", np.arange(1000)), ("reversed chain", np.arange(1000)[::-1]),
                        ("shuffled chain", np.random.default_rng(9).permutation(1000))):
        r = check_against_numpy(np.ascontiguousarray(x[order, None]), 0.25, 2, dev, what)
        assert np.all(r.labels == 0) and r.core_mask.all() and r.counts.max() == 3 and r.counts.min() == 2
        assert r.n_rounds <= 1000
    # the same chain cut in the middle: 0.5 between points 499 and 500
    x[500:] += 0.25
    r = check_against_numpy(np.ascontiguousarray(x[:, None]), 0.25, 2, dev, "cut chain")
    assert r.labels.tolist() == [0] * 500 + [1] * 500


def test_last_round_contract(dev, z):
    """the C entries by hand on pin d: rounds until d_changed is 0; then a core point's label is the lowest core index of its
    component, a border point's the least such root among its core neighbours, noise is -1, and one more round moves nothing"""
    X, eps, ms = case(z, "d")
    L = api.load_library()
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    a = torch.empty(n, dtype=torch.int32, device=dev)
    b = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ch = torch.full((1,), -7, dtype=torch.int32, device=dev)
    assert L.ra_dbscan_count(P(x), n, d, eps, ms, P(cnt), P(a), stream()) == 0
    ref = dbscan.dbscan(X, eps, ms, backend="numpy")
    core = ref.core_mask
    assert np.array_equal(cnt.cpu().numpy(), ref.counts)
    assert np.array_equal(a.cpu().numpy(), np.where(core, np.arange(n), -1))
    rounds, moved = 0, []
    while True:
        assert L.ra_dbscan_step(P(x), n, d, eps, P(cnt), ms, P(a), P(b), P(ch), stream()) == 0
        rounds += 1
        a, b = b, a
        moved.append(int(ch.item()))
        if moved[-1] == 0:
            break
        assert rounds <= core.sum()
    print("pin d: core points moved per round:", moved)
    lab = a.cpu().numpy()
    root = np.full(ref.n_clusters, n)
    np.minimum.at(root, ref.labels[core], np.nonzero(core)[0])
    assert np.array_equal(lab[core], root[ref.labels[core]])
    assert np.array_equal(lab[~core], np.where(ref.labels[~core] >= 0, root[np.maximum(ref.labels[~core], 0)], -1))
    assert all(u > 0 for u in moved[:-1]) and rounds == dbscan.dbscan(x, eps, ms).n_rounds
    assert L.ra_dbscan_step(P(x), n, d, eps, P(cnt), ms, P(a), P(b), P(ch), stream()) == 0
    assert int(ch.item()) == 0 and torch.equal(a, b)


def test_bitwise_repeatable(dev, z):
    for c in "bd":
        X, eps, ms = case(z, c)
        Xd = torch.from_numpy(X).to(dev)
        r0, r1 = dbscan.dbscan(Xd, eps, ms), dbscan.dbscan(Xd, eps, ms)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            r2 = dbscan.dbscan(Xd, eps, ms)
        s.synchronize()
        for r in (r1, r2):
            assert r.labels.tobytes() == r0.labels.tobytes() and r.counts.tobytes() == r0.counts.tobytes()
            assert r.core_mask.tobytes() == r0.core_mask.tobytes() and r.n_rounds == r0.n_rounds


@pytest.mark.parametrize("c", "abd")
def test_kdistances_identity_on_the_device(dev, z, c):
    X, eps, ms = case(z, c)
    Xd = torch.from_numpy(X).to(dev)
    kd = dbscan.kdistances(Xd, ms)
    assert kd.dtype == np.float64 and kd.shape == (len(X),)
    assert np.array_equal(dbscan.dbscan(Xd, eps, ms).core_mask, kd <= eps)
    assert np.all(dbscan.kdistances(Xd, 1) == 0.0) and np.all(np.isinf(api.dbscan_kdistances(Xd, len(X) + 1)))
    with pytest.raises(dbscan.DbscanError):
        dbscan.kdistances(Xd, 303)


def test_entry_points_reject_and_launch_nothing(dev):
    L = api.load_library()
    x = torch.zeros((8, 4), device=dev)
    cnt = torch.full((8,), 7, dtype=torch.int32, device=dev)
    lab = torch.full((8,), 7, dtype=torch.int32, device=dev)
    out = torch.full((8,), 7, dtype=torch.int32, device=dev)
    ch = torch.full((1,), 7, dtype=torch.int32, device=dev)
    s = stream()
    count, step = L.ra_dbscan_count, L.ra_dbscan_step
    nan, inf = float("nan"), float("inf")
    bad = [count(P(x), 0, 4, 1.0, 2, P(cnt), P(lab), s), count(P(x), 262145, 4, 1.0, 2, P(cnt), P(lab), s),
           count(P(x), 8, 0, 1.0, 2, P(cnt), P(lab), s), count(P(x), 8, 2049, 1.0, 2, P(cnt), P(lab), s),
           count(P(x), 8, 4, 0.0, 2, P(cnt), P(lab), s), count(P(x), 8, 4, -1.0, 2, P(cnt), P(lab), s),
           count(P(x), 8, 4, nan, 2, P(cnt), P(lab), s), count(P(x), 8, 4, inf, 2, P(cnt), P(lab), s),
           count(P(x), 8, 4, 1.0, 0, P(cnt), P(lab), s), count(None, 8, 4, 1.0, 2, P(cnt), P(lab), s),
           count(P(x), 8, 4, 1.0, 2, None, P(lab), s), count(P(x), 8, 4, 1.0, 2, P(cnt), None, s),
           step(P(x), 0, 4, 1.0, P(cnt), 2, P(lab), P(out), P(ch), s), step(P(x), 262145, 4, 1.0, P(cnt), 2, P(lab), P(out), P(ch), s),
           step(P(x), 8, 0, 1.0, P(cnt), 2, P(lab), P(out), P(ch), s), step(P(x), 8, 2049, 1.0, P(cnt), 2, P(lab), P(out), P(ch), s),
           step(P(x), 8, 4, 0.0, P(cnt), 2, P(lab), P(out), P(ch), s), step(P(x), 8, 4, -2.0, P(cnt), 2, P(lab), P(out), P(ch), s),
           step(P(x), 8, 4, nan, P(cnt), 2, P(lab), P(out), P(ch), s), step(P(x), 8, 4, 1.0, P(cnt), 0, P(lab), P(out), P(ch), s),
           step(None, 8, 4, 1.0, P(cnt), 2, P(lab), P(out), P(ch), s), step(P(x), 8, 4, 1.0, None, 2, P(lab), P(out), P(ch), s),
           step(P(x), 8, 4, 1.0, P(cnt), 2, None, P(out), P(ch), s), step(P(x), 8, 4, 1.0, P(cnt), 2, P(lab), None, P(ch), s),
           step(P(x), 8, 4, 1.0, P(cnt), 2, P(lab), P(out), None, s), step(P(x), 8, 4, 1.0, P(cnt), 2, P(lab), P(lab), P(ch), s)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ra_dbscan_step" in L.ra_last_error()
    torch.cuda.synchronize()
    assert torch.all(cnt == 7) and torch.all(lab == 7) and torch.all(out == 7) and torch.all(ch == 7)
    # labels outside 0 .. n - 1 in d_label address nothing
    assert count(P(x), 8, 4, 1.0, 2, P(cnt), P(lab), s) == 0
    wild = torch.tensor([-5, 0, 1, 9, 1, 0, 100000, -1], dtype=torch.int32, device=dev)
    assert step(P(x), 8, 4, 1.0, P(cnt), 2, P(wild), P(out), P(ch), s) == 0
    torch.cuda.synchronize()
    assert torch.all((out >= 0) & (out < 8))
    # the python layer: errors before a launch
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(torch.zeros((8, 4), device=dev, dtype=torch.float64), 1.0)
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(torch.zeros((8, 4), device=dev).t(), 1.0)
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(x, float("nan"))
    bx = torch.zeros((8, 4), device=dev)
    bx[3, 1] = float("nan")
    with pytest.raises(dbscan.DbscanError):
        dbscan.dbscan(bx, 1.0)


def test_tool_end_to_end_with_averages(dev, z, tmp_path, capsys):
    """pin b through the tool with --averages on a small synthetic stack: noise particles are left out of the averages"""
    from cryo_ralib_amd import geometry, synth
    X, eps, ms = case(z, "b")
    n, nx, ou = len(X), 32, 12
    refs = synth.make_references(3, nx, ou)
    parts, truth = synth.make_particles(refs, n, 2, 2, 0.3, ou=ou)
    inv = np.array([geometry.inverse_transform2(float(a), float(sx), float(sy), int(m))
                    for a, sx, sy, m in zip(truth["ang"], truth["sx"], truth["sy"], truth["mir"])], np.float64)
    np.save(tmp_path / "x.npy", X)
    np.save(tmp_path / "stack.npy", parts)
    np.savetxt(tmp_path / "init.txt", inv)
    assert dbscan.main([str(tmp_path / "x.npy"), str(tmp_path / "o.npz"), "--eps", str(eps), "--min_samples", str(ms), "--kdist",
                        "--stack", str(tmp_path / "stack.npy"), "--params", str(tmp_path / "init.txt"), "--ou", str(ou),
                        "--averages", str(tmp_path / "avg.npy")]) == 0
    o = np.load(tmp_path / "o.npz")
    lab = z["labels_b"]
    assert str(o["backend"]) == "device" and np.array_equal(o["labels"], lab) and int(o["n_clusters"]) == lab.max() + 1
    assert int(o["n_noise"]) == np.count_nonzero(lab < 0) > 0 and o["kdist"].shape == (n,) and np.all(np.diff(o["kdist"]) >= 0)
    assert np.array_equal(np.nonzero(o["core_mask"])[0], z["core_sample_indices_b"]) and int(o["n_rounds"]) >= 1
    avg = np.load(tmp_path / "avg.npy")
    keep = lab >= 0
    want = kmeans.class_averages(parts[keep], inv[keep], lab[keep], int(lab.max()) + 1, ou)
    assert avg.shape == (lab.max() + 1, nx, nx) and np.array_equal(avg, want)
    withnoise = kmeans.class_averages(parts, inv, np.maximum(lab, 0), int(lab.max()) + 1, ou)
    assert not np.array_equal(avg[0], withnoise[0])
    lines = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("cluster") for ln in lines) == lab.max() + 1 and any(ln.startswith("noise: ") for ln in lines)
