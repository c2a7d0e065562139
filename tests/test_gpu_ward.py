"""Ward clustering on the device (ra_ward_nearest / ra_ward_merge behind ward.linkage): the two entries entry by entry against the
checker's functions on one state, at the edges of the row tile of 64, the column tile of 64, the lane groups of 16 and the
feature chunk of 32; whole trees on every pin of tests/golden/ward_ref.npz, on duplicates, identical rows and the adversarial
line; bitwise repeatability; sweep; the C entries' rejections.

The state (C, size) is built on the host and handed to both sides, so only the fusing differs: W2 within (d + 2) 2^-52 relative
(d + 1 roundings in the chain, one in the factor), centroids within 4 x 2^-53 max(|c_a|, |c_b|) per coordinate.  The builders keep
the row-wise margin >= 1e-9 (tests/test_ward_cpu.py asserts it), far above either bound, so nn is an equality."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ward_cases as wc  # noqa: E402
from cryo_ralib_amd import api, kmeans, ward  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ward_ref.npz")
EPS = 2.0 ** -52
N_ROWS = (1, 63, 64, 65)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def checker(z):
    return {c: ward.linkage(z["X_" + c], backend="numpy") for c in wc.PIN_NAMES}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_nearest(C, size, rows, dev):
    L = api.load_library()
    n, d = C.shape
    c, s, r = torch.from_numpy(C).to(dev), torch.from_numpy(size).to(dev), torch.from_numpy(np.asarray(rows, np.int32)).to(dev)
    nn = torch.full((len(rows),), -7, dtype=torch.int32, device=dev)
    w2 = torch.full((len(rows),), -7.0, dtype=torch.float64, device=dev)
    assert L.ra_ward_nearest(P(c), P(s), n, d, P(r), len(rows), P(nn), P(w2), stream()) == 0, L.ra_last_error()
    out = nn.cpu().numpy(), w2.cpu().numpy()
    assert np.array_equal(c.cpu().numpy(), C) and np.array_equal(s.cpu().numpy(), size)           # the state is read only
    return out


def check_nearest(C, size, rows, dev, what):
    nn, w = device_nearest(C, size, rows, dev)
    rn, rw = ward.rows_numpy(C, size, rows)
    has = rn >= 0
    err, bound = np.abs(w[has] - rw[has]), (C.shape[1] + 2) * EPS * rw[has]
    rel = float(np.max(err / np.where(rw[has] > 0, rw[has], 1.0))) if has.any() else 0.0
    print("%s: n = %d, d = %d, %d live, %d rows (%d without a neighbour): nn differ at %d, W2 within %.2e relative (bound %.2e)" % (
        what, C.shape[0], C.shape[1], np.count_nonzero(size), len(rows), np.count_nonzero(~has), np.count_nonzero(nn != rn), rel,
        (C.shape[1] + 2) * EPS))
    assert np.array_equal(nn, rn)
    assert np.all(np.isposinf(w[~has])) and np.all(nn[~has] == -1)
    assert np.all(err <= bound)
    return nn, w


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 193])
def test_nearest_entry_by_entry(dev, n):
    for d in (1, 31, 32, 33, 65):
        for p, dead in enumerate(wc.DEAD_PATTERNS):
            C, size = wc.table(n, d, dead, 1000 * n + d)
            check_nearest(C, size, np.arange(n, dtype=np.int32), dev, dead)                      # every slot, dead ones included
            rows = wc.row_list(n, N_ROWS[(p + d) % 4], n + d + p)                                 # unordered, with repeats
            nn, w = check_nearest(C, size, rows, dev, dead + ", listed")
            assert nn[-1] == nn[0] and w[-1] == w[0]


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_nearest_row_lists(dev, n_rows):
    """every length of the list against every table size: the tail of the last row tile, rows that are dead or out of range"""
    for n in (2, 65, 193):
        C, size = wc.table(n, 33, "alternate" if n > 2 else "none", 7 * n + n_rows)
        rows = wc.row_list(n, n_rows, 5 * n + n_rows)
        check_nearest(C, size, rows, dev, "rows")
        rows[::3] = (-1, n, n + 70, -2 ** 31, 2 ** 31 - 1)[n_rows % 5]
        nn, w = check_nearest(C, size, rows, dev, "rows out of range")
        assert np.all(nn[::3] == -1) and np.all(np.isposinf(w[::3]))


def test_nearest_ties_go_to_the_lower_slot(dev):
    """bitwise equal candidates: duplicates of one point among the columns, across lanes, threads and column tiles"""
    C = np.zeros((200, 3))
    C[:, 0] = 1.0
    C[7] = (0.0, 0.0, 0.0)
    size = np.ones(200, np.int32)
    size[:3] = 0
    nn, w = check_nearest(C, size, np.arange(200, dtype=np.int32), dev, "ties")
    want = np.where(np.arange(200) == 3, 4, 3)
    want[7] = 3
    want[:3] = -1
    assert np.array_equal(nn, want) and np.all(w[(np.arange(200) > 2) & (np.arange(200) != 7)] == 0)


def device_merge(C, size, a, b, dev):
    L = api.load_library()
    n, d = C.shape
    c, s = torch.from_numpy(C).to(dev), torch.from_numpy(size).to(dev)
    ta, tb = torch.from_numpy(np.asarray(a, np.int32)).to(dev), torch.from_numpy(np.asarray(b, np.int32)).to(dev)
    assert L.ra_ward_merge(P(c), P(s), n, d, P(ta), P(tb), len(a), stream()) == 0, L.ra_last_error()
    return c.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("d", [1, 33])
@pytest.mark.parametrize("n_pairs", [1, 255, 256, 257])
def test_merge_entry_by_entry(dev, n_pairs, d):
    n = 2 * n_pairs + 41
    rng = np.random.default_rng(10 * n_pairs + d)
    C, size = wc.table(n, d, "sizes", n + d)
    size[rng.choice(n, 20, replace=False)] = 0                     # dead slots that no pair names
    live = rng.permutation(np.nonzero(size)[0])[:2 * n_pairs].reshape(2, n_pairs)
    a, b = live.min(axis=0), live.max(axis=0)
    # all pairs good
    got_c, got_s = device_merge(C, size, a, b, dev)
    sa, sb = size[a].astype(np.float64)[:, None], size[b].astype(np.float64)[:, None]
    want = (sa * C[a] + sb * C[b]) / (sa + sb)
    bound = 4 * 2.0 ** -53 * np.maximum(np.abs(C[a]), np.abs(C[b]))
    err = np.abs(got_c[a] - want)
    print("merge: %d pairs, d = %d: centroids within %.2f of the bound at worst" % (n_pairs, d, float(np.max(err / bound))))
    assert np.all(err <= bound)
    ws = size.copy()
    ws[a] += size[b]
    ws[b] = 0
    assert np.array_equal(got_s, ws)
    rest = np.ones(n, bool)
    rest[a] = False
    assert np.array_equal(got_c[rest], C[rest])                     # b's row too: a dead slot keeps its last centroid
    # skipped pairs change nothing: a >= b, a dead member, out of range
    dead = np.nonzero(size == 0)[0]
    a2, b2 = a.copy(), b.copy()
    for p in range(0, n_pairs, 5):
        kind = (p // 5) % 5
        if kind == 0:
            a2[p], b2[p] = b[p], a[p]
        elif kind == 1:
            b2[p] = a[p]
        elif kind == 2:
            if dead[-1] > a[p]:
                b2[p] = dead[-1]                                    # a dead b above a live a
            else:
                a2[p] = dead[0]                                     # a dead a, below b or not
        elif kind == 3:
            b2[p] = n + (p % 3) * 1000
        else:
            a2[p] = -1 - p
    ok = (a2 >= 0) & (a2 < b2) & (b2 < n)
    ok &= (size[np.clip(a2, 0, n - 1)] > 0) & (size[np.clip(b2, 0, n - 1)] > 0)
    assert not ok[0] and np.count_nonzero(~ok) == len(range(0, n_pairs, 5))
    got_c, got_s = device_merge(C, size, a2, b2, dev)
    ws = size.copy()
    ws[a2[ok]] += size[b2[ok]]
    ws[b2[ok]] = 0
    assert np.array_equal(got_s, ws)
    rest[:] = True
    rest[a2[ok]] = False
    assert np.array_equal(got_c[rest], C[rest])
    assert np.all(np.abs(got_c[a2[ok]] - want[ok]) <= bound[ok])


def check_tree(T, ref, exact):
    assert np.array_equal(T.children, ref.children) and np.array_equal(T.Z[:, 3], ref.Z[:, 3]) and np.array_equal(T.merges, ref.merges)
    assert np.array_equal(T.merge_round, ref.merge_round) and T.n_rounds == ref.n_rounds and T.rows_evaluated == ref.rows_evaluated
    if exact:
        assert np.array_equal(T.Z, ref.Z) and np.array_equal(T.w2, ref.w2)


@pytest.mark.parametrize("c", wc.PIN_NAMES)
def test_pin_trees(dev, z, checker, c):
    X, Z, ref = z["X_" + c], z["Z_" + c], checker[c]
    T = ward.linkage(torch.from_numpy(X).to(dev))
    check_tree(T, ref, False)
    assert np.array_equal(T.Z[:, :2], Z[:, :2]) and np.array_equal(T.Z[:, 3], Z[:, 3])
    disc = float(np.max(np.abs(ref.heights - Z[:, 2])))
    err = float(np.max(np.abs(T.heights - Z[:, 2])))
    print("pin %s: %d rounds, %.2f n rows evaluated; heights vs scipy: checker %.3e, device %.3e (top height %.3e)" % (
        c, T.n_rounds, T.rows_evaluated / len(X), disc, err, Z[-1, 2]))
    assert err <= max(1000 * disc, 1e-12 * Z[-1, 2])
    for k, lab in zip(z["ks_" + c], z["labels_" + c]):
        assert wc.same_partition(ward.cut(T, n_clusters=int(k)), lab)
    for t, lab in zip(z["thresholds_" + c], z["tlabels_" + c]):
        assert wc.same_partition(ward.cut(T, distance_threshold=float(t)), lab)
    res = ward.ward(torch.from_numpy(X).to(dev), n_clusters=int(z["ks_" + c][0]))
    assert np.array_equal(res.labels, ward.cut(T, n_clusters=int(z["ks_" + c][0]))) and res.centers.shape == (res.n_clusters, X.shape[1])


def test_duplicates_and_identical_rows_equal_the_checker_exactly(dev):
    """margin = 0 here, so no margin protects the decisions: they are equal because every tie is between bitwise-equal operands.
    Identical rows: Z bit for bit.  Duplicates: every decision (children, sizes, slots, rounds) and the 50 merges of copies
    (W2 = 0, centroids bitwise the points) bit for bit; the 24 merges of the separated groups that follow run fused on the
    device and unfused in the checker (rule 8) on centroids that are no longer float32 values, so their heights are held to the
    pins' floor, 1e-12 of the top height (measured on an MI355X: 1 of the 24 differs, by 1.1e-16 of the top height)."""
    X, group = wc.duplicates()
    T, ref = ward.linkage(torch.from_numpy(X).to(dev)), ward.linkage(X, backend="numpy")
    check_tree(T, ref, False)
    assert np.array_equal(T.Z[:50], ref.Z[:50]) and np.all(T.w2[:50] == 0) and wc.same_partition(ward.cut(T, n_clusters=25), group)
    print("duplicates: %d of the 24 heights of separated groups differ, by at most %.3e of the top height" % (
        np.count_nonzero(T.heights[50:] != ref.heights[50:]), np.max(np.abs(T.heights - ref.heights)) / ref.heights[-1]))
    assert np.max(np.abs(T.heights - ref.heights)) <= 1e-12 * ref.heights[-1]
    X = wc.identical()
    T = ward.linkage(torch.from_numpy(X).to(dev))
    check_tree(T, ward.linkage(X, backend="numpy"), True)
    assert np.all(T.heights == 0)


def test_adversarial_line(dev):
    X = wc.line(600)
    ref = ward.linkage(X, backend="numpy")
    T = ward.linkage(torch.from_numpy(X).to(dev))
    print("line: n = 600, %d rounds, %.2f n rows evaluated" % (T.n_rounds, T.rows_evaluated / 600))
    check_tree(T, ref, False)
    assert np.allclose(T.heights, ref.heights, rtol=1e-12, atol=0) and T.n_rounds >= 290


def test_bitwise_repeatable_across_calls_and_streams(dev, z):
    x = torch.from_numpy(z["X_blobs50"]).to(dev)
    first = ward.linkage(x)
    again = ward.linkage(x)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = ward.linkage(x)
    side.synchronize()
    assert np.array_equal(first.Z, again.Z) and np.array_equal(first.Z, other.Z)
    assert np.array_equal(first.merges, other.merges) and first.n_rounds == other.n_rounds


def test_sweep_on_the_device(dev, z):
    x = torch.from_numpy(z["X_gauss5"]).to(dev)
    ks = [2, 3, 5, 9]
    sw = ward.sweep(x, ks)
    T = ward.linkage(x)
    assert np.array_equal(sw.tree.Z, T.Z) and [r.k for r in sw.rows] == ks
    for r in sw.rows:
        assert np.array_equal(r.labels, ward.cut(T, n_clusters=r.k)) and r.inertia == T.inertia(r.k)
        v = kmeans.validity(x, r.labels, r.k)
        assert (r.silhouette, r.calinski_harabasz, r.davies_bouldin) == (v.silhouette, v.calinski_harabasz, v.davies_bouldin)
        assert r.inertia == pytest.approx(wc.inertia_direct(z["X_gauss5"], r.labels), rel=1e-10)
    best = max(sw.rows, key=lambda r: (r.silhouette, -r.k))
    assert sw.best_k == best.k


def test_tool_on_sdr_output_with_sweep_truth_and_averages(dev, tmp_path, capsys):
    """stack -> sdr tool -> ward tool (--sweep, --truth, --averages) -> the multi-reference command line takes the averages"""
    from cryo_ralib_amd import cli, geometry, sdr, synth
    nx, ou, nref, n = 32, 12, 3, 240
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, 2, 2, 0.3, ou=ou)
    inv = np.array([geometry.inverse_transform2(float(a), float(sx), float(sy), int(m))
                    for a, sx, sy, m in zip(truth["ang"], truth["sx"], truth["sy"], truth["mir"])], np.float64)
    cls = np.asarray(truth["cls"])
    np.save(tmp_path / "stack.npy", parts)
    np.savetxt(tmp_path / "init.txt", inv)
    np.save(tmp_path / "truth.npy", cls.astype(np.int64))
    assert sdr.main([str(tmp_path / "stack.npy"), str(tmp_path / "f.npz"), "--p0", "8", "--q0", "8", "--r", "10",
                     "--params", str(tmp_path / "init.txt")]) == 0
    assert ward.main([str(tmp_path / "f.npz"), str(tmp_path / "o.npz"), "--sweep", "2:6", "--k", "3", "--truth", str(tmp_path / "truth.npy"),
                      "--stack", str(tmp_path / "stack.npy"), "--params", str(tmp_path / "init.txt"), "--ou", str(ou),
                      "--averages", str(tmp_path / "avg.npy")]) == 0
    o = np.load(tmp_path / "o.npz")
    k = 3
    print("tool: best_k = %d, at k = 3 purity %.4f, c_purity %.4f" % (int(o["best_k"]), float(o["purity"]), float(o["c_purity"])))
    assert str(o["backend"]) == "device" and o["labels"].shape == (n,) and o["linkage"].shape == (n - 1, 4) and o["sweep"].shape == (5, 5)
    assert int(o["n_clusters"]) == k == o["labels"].max() + 1 and 2 <= int(o["best_k"]) <= 6
    assert float(o["purity"]) >= 0.95 and float(o["c_purity"]) >= 0.95           # the bar the kmeans tool's test sets on this stack
    F = np.load(tmp_path / "f.npz")["factors"]
    T = ward.linkage(F, backend="numpy")
    assert np.array_equal(o["linkage"][:, :2], T.Z[:, :2]) and np.array_equal(o["labels"], ward.cut(T, n_clusters=k))
    avg = np.load(tmp_path / "avg.npy")
    assert avg.shape == (k, nx, nx) and np.array_equal(avg, kmeans.class_averages(parts, inv, o["labels"], k, ou))
    out = tmp_path / "mref"
    assert cli.main_mref([str(tmp_path / "stack.npy"), str(tmp_path / "avg.npy"), str(out), "--ou", str(ou), "--xr", "2",
                          "--yr", "2", "--maxit", "1", "--ext", "npy"]) == 0
    rows = np.loadtxt(out / "params.txt", ndmin=2)
    got = np.empty(n, np.int64)
    got[rows[:, 0].astype(np.int64)] = rows[:, 5].astype(np.int64)
    assert kmeans.purity_score(cls, got) >= 0.95
    capsys.readouterr()


def test_c_entries_reject(dev):
    L = api.load_library()
    c = torch.full((8, 4), 7.0, dtype=torch.float64, device=dev)
    size = torch.full((8,), 7, dtype=torch.int32, device=dev)
    rows = torch.arange(8, dtype=torch.int32, device=dev)
    nn = torch.full((8,), 7, dtype=torch.int32, device=dev)
    w2 = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
    a = torch.zeros(4, dtype=torch.int32, device=dev)
    b = torch.ones(4, dtype=torch.int32, device=dev)
    s = stream()
    near, merge = L.ra_ward_nearest, L.ra_ward_merge
    bad = [near(P(c), P(size), 1, 4, P(rows), 1, P(nn), P(w2), s), near(P(c), P(size), 262145, 4, P(rows), 8, P(nn), P(w2), s),
           near(P(c), P(size), 8, 0, P(rows), 8, P(nn), P(w2), s), near(P(c), P(size), 8, 2049, P(rows), 8, P(nn), P(w2), s),
           near(P(c), P(size), 8, 4, P(rows), 0, P(nn), P(w2), s), near(P(c), P(size), 8, 4, P(rows), 262145, P(nn), P(w2), s),
           near(None, P(size), 8, 4, P(rows), 8, P(nn), P(w2), s), near(P(c), None, 8, 4, P(rows), 8, P(nn), P(w2), s),
           near(P(c), P(size), 8, 4, None, 8, P(nn), P(w2), s), near(P(c), P(size), 8, 4, P(rows), 8, None, P(w2), s),
           near(P(c), P(size), 8, 4, P(rows), 8, P(nn), None, s)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ra_ward_nearest" in L.ra_last_error()
    bad = [merge(P(c), P(size), 1, 4, P(a), P(b), 1, s), merge(P(c), P(size), 262145, 4, P(a), P(b), 4, s),
           merge(P(c), P(size), 8, 0, P(a), P(b), 4, s), merge(P(c), P(size), 8, 2049, P(a), P(b), 4, s),
           merge(P(c), P(size), 8, 4, P(a), P(b), 0, s), merge(P(c), P(size), 8, 4, P(a), P(b), 5, s),
           merge(None, P(size), 8, 4, P(a), P(b), 4, s), merge(P(c), None, 8, 4, P(a), P(b), 4, s),
           merge(P(c), P(size), 8, 4, None, P(b), 4, s), merge(P(c), P(size), 8, 4, P(a), None, 4, s)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ra_ward_merge" in L.ra_last_error()
    torch.cuda.synchronize()
    assert torch.all(c == 7) and torch.all(size == 7) and torch.all(nn == 7) and torch.all(w2 == 7)
    # the python layer: errors before a launch
    with pytest.raises(ward.WardError):
        ward.linkage(torch.zeros((8, 4), device=dev, dtype=torch.float64))
    with pytest.raises(ward.WardError):
        ward.linkage(torch.zeros((8, 4), device=dev).t())
    with pytest.raises(ward.WardError):
        ward.linkage(torch.zeros((1, 4), device=dev))
    with pytest.raises(ward.WardError):
        ward.linkage(torch.zeros((8, 4), device=dev), details=True)
    with pytest.raises(ward.WardError):
        ward.ward(torch.zeros((8, 4), device=dev), n_clusters=9)
    bx = torch.zeros((8, 4), device=dev)
    bx[3, 1] = float("nan")
    with pytest.raises(ward.WardError):
        ward.linkage(bx)
