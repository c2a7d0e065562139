"""HDBSCAN on the device (ra_hdbscan_core / ra_hdbscan_round behind hdbscan.hdbscan): every pin of tests/golden/hdbscan_ref.npz, the
shapes around the kernel's tiles and feature chunks, one Boruvka round on hand-set components, min_samples at ra_tsne_knn's cap,
bitwise repeatability, the C entries' rejections and the tool.

Every comparison is an equality against the float64 numpy backend.  All data lies on a 1/1024 grid with |x| <= 16 (integers for the
lattice): differences, squares and sums are exact in double, so the device's fused multiply-adds and numpy's unfused ones give
the same D2 bit for bit, and with it the same core distances, tree edges, labels, probabilities and tie sets."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, hdbscan, kmeans  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan_ref.npz")
CASES = "abcdefghi"


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
    ms = int(z["min_samples_" + c])
    return z["X_" + c], int(z["min_cluster_size_" + c]), None if ms < 0 else ms, str(z["method_" + c])


def grid(v):
    return (np.clip(np.round(np.asarray(v, np.float64) * 1024), -16 * 1024, 16 * 1024) / 1024).astype(np.float32)


def same(r, ref):
    return (np.array_equal(r.core_distances, ref.core_distances) and all(np.array_equal(a, b) for a, b in zip(r.mst, ref.mst))
            and np.array_equal(r.labels, ref.labels) and np.array_equal(r.probabilities, ref.probabilities)
            and np.array_equal(r.tie_mask, ref.tie_mask) and r.n_clusters == ref.n_clusters
            and all(np.array_equal(a, b) for a, b in zip(r.condensed, ref.condensed)) and np.array_equal(r.stabilities, ref.stabilities))


def check_against_numpy(X, mcs, ms, method, dev, what):
    r = hdbscan.hdbscan(torch.from_numpy(X).to(dev), mcs, ms, method)
    ref = hdbscan.hdbscan(X, mcs, ms, method, backend="numpy")
    n = len(X)
    print("%s: n = %d, d = %d, min_cluster_size = %d, min_samples = %s, %s: %d clusters, %d noise, |T| = %d, %d rounds; core2 differ at %d, "
          "edges at %d, labels at %d, probabilities at %d" % (
              what, n, X.shape[1], mcs, ms, method, r.n_clusters, r.n_noise, r.tie_mask.sum(), r.n_rounds,
              np.count_nonzero(r.core_distances != ref.core_distances),
              np.count_nonzero((r.mst[0] != ref.mst[0]) | (r.mst[1] != ref.mst[1]) | (r.mst[2] != ref.mst[2])),
              np.count_nonzero(r.labels != ref.labels), np.count_nonzero(r.probabilities != ref.probabilities)))
    assert r.labels.dtype == np.int32 and r.probabilities.dtype == np.float64 and r.tie_mask.dtype == np.bool_
    assert r.mst[0].dtype == np.int32 and r.mst[2].dtype == np.float64 and len(r.mst[0]) == n - 1
    assert same(r, ref)
    assert 1 <= r.n_rounds <= int(np.ceil(np.log2(n))) + 1
    return r


@pytest.mark.parametrize("c", CASES)
def test_device_equals_checker_and_pins(dev, z, c):
    X, mcs, ms, method = case(z, c)
    r = check_against_numpy(X, mcs, ms, method, dev, "pin " + c)
    assert np.array_equal(r.labels, z["labels_" + c]) and np.array_equal(r.probabilities, z["probabilities_" + c])
    assert np.array_equal(r.tie_mask, z["tie_mask_" + c])


@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 65])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 129, 257])
def test_shapes_around_the_tiles(dev, n, d):
    rng = np.random.default_rng(1000 * n + d)
    X = grid(rng.normal(size=(n, d)) + 4.0 * rng.integers(0, 2, (n, 1)))
    r = check_against_numpy(X, min(5, n), min(3, n), "eom", dev, "shape")
    if n == 2:
        assert r.mst[0].tolist() == [0] and r.mst[1].tolist() == [1] and r.n_rounds == 1


def device_core2(X, ms, dev):
    L = api.load_library()
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    out = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    assert L.ra_hdbscan_core(P(x), n, d, ms, P(out), stream()) == 0
    return out.cpu().numpy()


def device_round(X, core2, comp, dev):
    L = api.load_library()
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    c2 = torch.from_numpy(np.asarray(core2, np.float64)).to(dev)
    cp = torch.from_numpy(np.asarray(comp, np.int32)).to(dev)
    w2 = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    lo = torch.full((n,), -7, dtype=torch.int32, device=dev)
    hi = torch.full((n,), -7, dtype=torch.int32, device=dev)
    assert L.ra_hdbscan_round(P(x), n, d, P(c2), P(cp), P(w2), P(lo), P(hi), stream()) == 0
    return w2.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()


def numpy_round(X, core2, comp):
    """the least (w2, lo, hi) edge leaving every component, at its root; +inf, -1, -1 everywhere else"""
    n = len(X)
    Xd = X.astype(np.float64)
    D2 = np.zeros((n, n))
    for t in range(X.shape[1]):
        df = Xd[:, t, None] - Xd[None, :, t]
        D2 += df * df
    W = np.maximum(np.maximum(D2, core2[:, None]), core2[None, :])
    w2, lo, hi = np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for root in np.unique(comp):
        i, j = np.nonzero((comp == root)[:, None] & (comp != root)[None, :])
        if len(i) == 0:
            continue
        a, b, w = np.minimum(i, j), np.maximum(i, j), W[i, j]
        e = np.lexsort((b, a, w))[0]
        w2[root], lo[root], hi[root] = w[e], a[e], b[e]
    return w2, lo, hi


def check_round(X, core2, comp, dev):
    got, want = device_round(X, core2, comp, dev), numpy_round(X, core2, np.asarray(comp))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return got


def test_round_on_hand_set_components(dev):
    n, d = 150, 3
    X = grid(np.random.default_rng(5).normal(size=(n, d)))
    core2 = hdbscan.core2_numpy(X, 4)
    assert np.array_equal(device_core2(X, 4, dev), core2)
    # all singletons: every point's least edge
    w2, lo, hi = check_round(X, core2, np.arange(n), dev)
    assert np.all(np.isfinite(w2)) and np.all((lo == np.arange(n)) | (hi == np.arange(n)))
    # two components that meet between rows 63 and 64
    comp = np.where(np.arange(n) < 64, 0, 64)
    w2, lo, hi = check_round(X, core2, comp, dev)
    assert lo[0] == lo[64] and hi[0] == hi[64] and w2[0] == w2[64] and lo[0] < 64 <= hi[0]
    assert np.all(np.isinf(np.delete(w2, [0, 64]))) and np.all(np.delete(lo, [0, 64]) == -1)
    # interleaved components, and roots that are not 0
    check_round(X, core2, np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 1, 2)), dev)
    # one component: no edge, the sentinel everywhere
    w2, lo, hi = check_round(X, core2, np.zeros(n, np.int64), dev)
    assert np.all(np.isinf(w2)) and np.all(lo == -1) and np.all(hi == -1)
    # comp values outside 0 .. n - 1 address nothing
    wild = np.arange(n)
    wild[[3, 70]] = [-5, 100000]
    w2, lo, hi = device_round(X, core2, wild, dev)
    assert np.all((lo >= -1) & (lo < n) & (hi >= -1) & (hi < n)) and np.isinf(w2[3]) and np.isinf(w2[70])


def test_round_on_identical_points_and_on_a_lattice(dev):
    n = 130
    X = np.full((n, 5), 1.25, np.float32)
    w2, lo, hi = check_round(X, np.zeros(n), np.arange(n), dev)
    assert np.all(w2 == 0) and lo.tolist() == [0] * n and hi.tolist() == [1] + list(range(1, n))      # every i > 0 picks (0, i)
    r = check_against_numpy(X, 5, 5, "eom", dev, "identical points")
    assert r.mst[0].tolist() == [0] * (n - 1) and r.mst[1].tolist() == list(range(1, n)) and np.all(r.labels == -1)
    # an integer lattice: many equal D2, shuffled rows
    g = np.stack(np.meshgrid(np.arange(12), np.arange(11)), -1).reshape(-1, 2).astype(np.float32)
    g = g[np.random.default_rng(3).permutation(len(g))]
    for ms in (1, 3):
        core2 = hdbscan.core2_numpy(g, ms)
        assert np.array_equal(device_core2(g, ms, dev), core2)
        check_round(g, core2, np.arange(len(g)), dev)
        check_round(g, core2, np.where(np.arange(len(g)) < 70, 0, 70), dev)
    check_against_numpy(g, 4, 3, "eom", dev, "lattice")
    check_against_numpy(g, 4, 1, "leaf", dev, "lattice")


@pytest.mark.parametrize("n", [302, 303])
@pytest.mark.parametrize("ms", [1, 2, 302])
def test_min_samples_at_the_neighbour_cap(dev, n, ms):
    rng = np.random.default_rng(n + ms)
    X = grid(rng.normal(size=(n, 2)) + 5.0 * rng.integers(0, 2, (n, 1)))
    assert np.array_equal(device_core2(X, ms, dev), hdbscan.core2_numpy(X, ms))
    check_against_numpy(X, 10, ms, "eom", dev, "cap")
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(torch.from_numpy(X).to(dev), 10, 303)


def test_bitwise_repeatable(dev, z):
    for c in "bf":
        X, mcs, ms, method = case(z, c)
        Xd = torch.from_numpy(X).to(dev)
        r0, r1 = hdbscan.hdbscan(Xd, mcs, ms, method), api.hdbscan(Xd, min_cluster_size=mcs, min_samples=ms, cluster_selection_method=method)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            r2 = hdbscan.hdbscan(Xd, mcs, ms, method)
        s.synchronize()
        for r in (r1, r2):
            assert r.labels.tobytes() == r0.labels.tobytes() and r.probabilities.tobytes() == r0.probabilities.tobytes()
            assert r.tie_mask.tobytes() == r0.tie_mask.tobytes() and r.n_rounds == r0.n_rounds
            assert r.core_distances.tobytes() == r0.core_distances.tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r.mst, r0.mst))


def test_entry_points_reject_and_launch_nothing(dev):
    L = api.load_library()
    x = torch.zeros((8, 4), device=dev)
    c2 = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
    comp = torch.arange(8, dtype=torch.int32, device=dev)
    w2 = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
    lo = torch.full((8,), 7, dtype=torch.int32, device=dev)
    hi = torch.full((8,), 7, dtype=torch.int32, device=dev)
    s = stream()
    core, rnd = L.ra_hdbscan_core, L.ra_hdbscan_round
    bad = [core(P(x), 1, 4, 1, P(c2), s), core(P(x), 262145, 4, 2, P(c2), s), core(P(x), 8, 0, 2, P(c2), s),
           core(P(x), 8, 2049, 2, P(c2), s), core(P(x), 8, 4, 0, P(c2), s), core(P(x), 8, 4, 9, P(c2), s),
           core(P(x), 1000, 4, 303, P(c2), s), core(None, 8, 4, 2, P(c2), s), core(P(x), 8, 4, 2, None, s),
           rnd(P(x), 1, 4, P(c2), P(comp), P(w2), P(lo), P(hi), s), rnd(P(x), 262145, 4, P(c2), P(comp), P(w2), P(lo), P(hi), s),
           rnd(P(x), 8, 0, P(c2), P(comp), P(w2), P(lo), P(hi), s), rnd(P(x), 8, 2049, P(c2), P(comp), P(w2), P(lo), P(hi), s),
           rnd(None, 8, 4, P(c2), P(comp), P(w2), P(lo), P(hi), s), rnd(P(x), 8, 4, None, P(comp), P(w2), P(lo), P(hi), s),
           rnd(P(x), 8, 4, P(c2), None, P(w2), P(lo), P(hi), s), rnd(P(x), 8, 4, P(c2), P(comp), None, P(lo), P(hi), s),
           rnd(P(x), 8, 4, P(c2), P(comp), P(w2), None, P(hi), s), rnd(P(x), 8, 4, P(c2), P(comp), P(w2), P(lo), None, s)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ra_hdbscan_round" in L.ra_last_error()
    torch.cuda.synchronize()
    assert torch.all(c2 == 7) and torch.all(w2 == 7) and torch.all(lo == 7) and torch.all(hi == 7)
    # the python layer: errors before a launch
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(torch.zeros((8, 4), device=dev, dtype=torch.float64))
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(torch.zeros((8, 4), device=dev).t())
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(x, 9)
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(x, 5, 0)
    bx = torch.zeros((8, 4), device=dev)
    bx[3, 1] = float("nan")
    with pytest.raises(hdbscan.HdbscanError):
        hdbscan.hdbscan(bx, 3)


def test_tool_end_to_end_with_averages(dev, z, tmp_path, capsys):
    """pin a through the tool with --averages on a small synthetic stack: noise particles are left out of the averages"""
    from cryo_ralib_amd import geometry, synth
    X, mcs, ms, method = case(z, "a")
    n, nx, ou = len(X), 32, 12
    refs = synth.make_references(3, nx, ou)
    parts, truth = synth.make_particles(refs, n, 2, 2, 0.3, ou=ou)
    inv = np.array([geometry.inverse_transform2(float(a), float(sx), float(sy), int(m))
                    for a, sx, sy, m in zip(truth["ang"], truth["sx"], truth["sy"], truth["mir"])], np.float64)
    np.savez(tmp_path / "x.npz", embedding=X)
    np.save(tmp_path / "stack.npy", parts)
    np.savetxt(tmp_path / "init.txt", inv)
    assert hdbscan.main([str(tmp_path / "x.npz"), str(tmp_path / "o.npz"), "--min_cluster_size", str(mcs), "--min_samples", str(ms),
                         "--method", method, "--min_proba", "0.25", "--stack", str(tmp_path / "stack.npy"),
                         "--params", str(tmp_path / "init.txt"), "--ou", str(ou), "--averages", str(tmp_path / "avg.npy")]) == 0
    o = np.load(tmp_path / "o.npz")
    lab, prob = z["labels_a"], z["probabilities_a"]
    assert str(o["backend"]) == "device" and np.array_equal(o["labels"], lab) and int(o["n_clusters"]) == lab.max() + 1
    assert np.array_equal(o["probabilities"], prob) and np.array_equal(o["tie_mask"], z["tie_mask_a"])
    assert np.array_equal(o["keep"], prob >= 0.25) and int(o["n_noise"]) == np.count_nonzero(lab < 0) > 0 and int(o["n_rounds"]) >= 1
    assert o["mst_distance"].shape == (n - 1,) and o["core_distances"].shape == (n,) and len(o["stabilities"]) == lab.max() + 1
    avg = np.load(tmp_path / "avg.npy")
    keep = lab >= 0
    want = kmeans.class_averages(parts[keep], inv[keep], lab[keep], int(lab.max()) + 1, ou)
    assert avg.shape == (lab.max() + 1, nx, nx) and np.array_equal(avg, want)
    withnoise = kmeans.class_averages(parts, inv, np.maximum(lab, 0), int(lab.max()) + 1, ou)
    assert not np.array_equal(avg[0], withnoise[0])
    lines = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("cluster") for ln in lines) == lab.max() + 1 and any(ln.startswith("noise: ") for ln in lines)
