"""Out-of-sample t-SNE on the device (ra_tsne_knn_query, ra_tsne_affinity_rows, ra_tsne_place_gradient, ra_tsne_place behind
tsne.transform), on the inputs of tests/test_tsne_place_cpu.py (whose properties that file asserts without a GPU).  Integer
coordinates and counted embeddings make every value exact, so neighbour lists, distances, Z_i and the counted gradients are
compared for equality; the real-valued cases use the bounds that file derives from term counts and the float64 reference; rule 7 is
checked bit for bit.  Each toleranced test prints its largest error / bound ratio."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, tsne  # noqa: E402
from test_tsne_place_cpu import (COUNTED_CASES, FEATURE_D, GRAD_M, GRAD_N, GRAD_SCALES, LEARNING_RATE, LINE_CASES,  # noqa: E402
                                 MOMENTUM, PLACE_CASES, PLACE_ITERS, checker_margin, clusters, counted_case, duplicate_free,
                                 feature_case, gradient_case, grid_case, identical_case, line_case, place_case, random_lists)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on(dev, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


# ---- 1. kNN of query rows against base rows, exact

def check_query_exact(dev, Q, X, idx, d2):
    got_i, got_d = tsne.knn_query(on(dev, Q), on(dev, X), idx.shape[1])
    assert np.array_equal(got_i, idx), np.argwhere(got_i != idx)[:10]
    assert np.array_equal(got_d, d2), np.argwhere(got_d != d2)[:10]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("m,k,nq", LINE_CASES)
def test_query_line(dev, m, k, nq, reverse):
    check_query_exact(dev, *line_case(m, k, nq, reverse))


@pytest.mark.parametrize("d", FEATURE_D)
def test_query_feature_dimension(dev, d):
    check_query_exact(dev, *feature_case(d))


def test_query_identical_base_points(dev):
    check_query_exact(dev, *identical_case())


@pytest.mark.parametrize("k", [8, 91])
def test_query_grid_and_queries_on_base_points(dev, k):
    check_query_exact(dev, *grid_case(k))


@pytest.mark.parametrize("k", [10, 91])
def test_query_agrees_with_the_unchanged_kernel(dev, k):
    X = on(dev, duplicate_free())
    qi, qd = tsne.knn_query(X, X, k + 1)
    ki, kd = tsne.knn(X, k)
    assert np.array_equal(qi[:, 0], np.arange(X.shape[0])) and np.all(qd[:, 0] == 0.0)
    assert np.array_equal(qi[:, 1:], ki) and np.array_equal(qd[:, 1:], kd)


# ---- 2. repulsion and Z_i, counted

def run_gradient(dev, y, Y, idx, p, exaggeration=1.0):
    """ra_tsne_place_gradient: (gradient [n][2] float32, KL_i, Z_i) as numpy arrays"""
    with torch.cuda.device(dev):
        g, kl, z = tsne._Device(dev).place_gradient(on(dev, y, np.float32), on(dev, Y, np.float32), on(dev, idx, np.int32),
                                                    on(dev, p, np.float32), exaggeration)
        return g.cpu().numpy(), kl.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize("m,n,pair", COUNTED_CASES)
def test_counted_repulsion_and_z(dev, m, n, pair):
    Y, y, idx, p, Z, rep, grad = counted_case(m, n, pair)
    g, kl, z = run_gradient(dev, y, Y, idx, p)
    assert np.array_equal(z, Z), np.argwhere(z != Z)[:10]
    assert np.array_equal(g, grad), np.argwhere(g != grad)[:10]
    # the row repulsion itself: g = float32(-4 rep / Z) with rep a multiple of 1/4 and Z of 1/2, both exact
    assert np.all(kl == 0.0)


# ---- 3. gradient, KL_i and Z_i, real-valued

def check_gradient(dev, case, tag):
    Y, y, idx, p, exag, g, kl, Z, gb, klb, zb = case
    got, got_kl, got_z = run_gradient(dev, y, Y, idx, p, exag)
    err = np.abs(got - g)
    print("RATIO place gradient %s %.4f  kl %.4f  z %.4f" % (tag, float(np.max(err / gb)),
                                                             float(np.max(np.abs(got_kl - kl) / np.maximum(klb, 1e-300))),
                                                             float(np.max(np.abs(got_z - Z) / zb))))
    assert np.all(err <= gb), np.argwhere(err > gb)[:10]
    assert np.all(np.abs(got_kl - kl) <= klb)
    assert np.all(np.abs(got_z - Z) <= zb)
    assert np.max(np.abs(got)) <= 2.0 * (exag + 1.0)


@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("n", GRAD_N)
@pytest.mark.parametrize("m", GRAD_M)
def test_gradient_kl_and_z(dev, m, n, scale):
    check_gradient(dev, gradient_case(m, n, scale), "m=%d n=%d scale=%g" % (m, n, scale))


def test_gradient_hostile_lists(dev):
    case = gradient_case(1025, 257, 5.0, True)
    check_gradient(dev, case, "hostile")
    Y, y, idx, p = case[:4]
    got = run_gradient(dev, y, Y, idx, p, case[4])
    assert np.all(got[1][::9] == 0.0)                                    # rows of zero p: no attraction, KL_i = 0


def test_gradient_outputs_are_optional(dev):
    Y, y, idx, p, exag, g = gradient_case(257, 5, 5.0)[:6]
    full = run_gradient(dev, y, Y, idx, p, exag)
    L, s = api.load_library(), stream()
    a = [on(dev, y, np.float32), on(dev, Y, np.float32), on(dev, idx, np.int32), on(dev, p, np.float32)]
    for which in range(3):
        outs = [torch.full((5, 2), 7.0, device=dev), torch.full((5,), 7.0, dtype=torch.float64, device=dev),
                torch.full((5,), 7.0, dtype=torch.float64, device=dev)]
        ptrs = [P(o) if i == which else None for i, o in enumerate(outs)]
        assert L.ra_tsne_place_gradient(P(a[0]), 5, P(a[1]), 257, P(a[2]), P(a[3]), idx.shape[1], exag, *ptrs, s) == 0
        assert np.array_equal(outs[which].cpu().numpy(), full[which])


# ---- 4. one and five iterations of ra_tsne_place

@pytest.mark.parametrize("iters", PLACE_ITERS)
@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("m,n", PLACE_CASES)
def test_place_iterations(dev, m, n, scale, iters):
    """ra_tsne_place returns no gains, so they are read off a replay: the optimiser's rule applied on the host in float32 to the
    gradients ra_tsne_place_gradient returns at each y (the same pair loop, so the same bits as inside the launch) must give
    the launch's y bit for bit, and the replay's gains must equal the float64 reference's wherever the branch was decided"""
    Y, y0, idx, p, exag = gradient_case(m, n, scale)[:5]
    gains, decided, y_ref, yb = place_case(m, n, scale, iters)
    assert np.mean(decided) >= 0.95
    f32 = np.float32
    with torch.cuda.device(dev):
        D = tsne._Device(dev)
        y = on(dev, y0, np.float32)
        yf, ix, pv = on(dev, Y, np.float32), on(dev, idx, np.int32), on(dev, p, np.float32)
        kl = D.place(y, yf, ix, pv, exag, MOMENTUM, LEARNING_RATE, iters).cpu().numpy()
        got = y.cpu().numpy()
        want_kl = D.place_gradient(y, yf, ix, pv, 1.0)[1].cpu().numpy()
        ry, ru, rg = y0.astype(f32), np.zeros((n, 2), f32), np.ones((n, 2), f32)
        for _ in range(iters):
            g = D.place_gradient(on(dev, ry), yf, ix, pv, exag)[0].cpu().numpy()
            rg = np.maximum(np.where(ru * g < f32(0.0), rg + f32(0.2), rg * f32(0.8)), f32(0.01))
            ru = f32(MOMENTUM) * ru - f32(LEARNING_RATE) * (g * rg)
            ry = ry + ru
    assert ry.dtype == f32 and rg.dtype == f32
    assert np.array_equal(got, ry), np.argwhere(got != ry)[:10]
    assert np.array_equal(rg[decided], gains[decided]), np.argwhere((rg != gains) & decided)[:10]
    err = np.abs(got - y_ref)[decided]
    print("RATIO place m=%d n=%d scale=%g iters=%d y %.4f" % (m, n, scale, iters, float(np.max(err / yb[decided]))))
    assert np.all(err <= yb[decided]), np.argwhere((np.abs(got - y_ref) > yb) & decided)[:10]
    assert np.array_equal(kl, want_kl)                                   # KL_i at the final y, by the shared pair loop


# ---- 5. rule 7, bit for bit

@pytest.fixture(scope="module")
def rule7(dev):
    """1000 new rows against 1100 fitted rows under a random embedding, placed in one call"""
    Xf, _ = clusters(1100, 10, 21)
    Xn, _ = clusters(1000, 10, 22)
    Yf = (np.random.default_rng(23).normal(size=(1100, 2)) * 5.0).astype(np.float32)
    kw = dict(perplexity=10.0, n_iter=40)
    with torch.cuda.device(dev):
        xf, yf = on(dev, Xf), on(dev, Yf)
        one = tsne.transform(Xn, xf, yf, details=True, **kw)
    return Xn, xf, yf, kw, one


def same(a, b, rows=slice(None)):
    return all(np.array_equal(x[rows], y) for x, y in zip(a, b))


@pytest.mark.parametrize("batch,count", [(1, 12), (7, 70), (64, 1000), (929, 1000)])
def test_batches_do_not_change_a_bit(dev, rule7, batch, count):
    Xn, xf, yf, kw, one = rule7
    with torch.cuda.device(dev):
        got = tsne.transform(Xn[:count], xf, yf, batch=batch, details=True, **kw)
    assert same(one, got, slice(0, count))


def test_order_and_tensor_input_do_not_change_a_bit(dev, rule7):
    Xn, xf, yf, kw, one = rule7
    perm = np.random.default_rng(0).permutation(1000)
    with torch.cuda.device(dev):
        got = tsne.transform(on(dev, Xn[perm]), xf, yf, details=True, **kw)
    assert same(one, got, perm)


def test_one_point_alone_and_inside_4097(dev):
    rng = np.random.default_rng(4097)
    n, m, k = 4097, 1500, 31
    Y, y = (rng.normal(size=(m, 2)) * 5.0).astype(np.float32), (rng.normal(size=(n, 2)) * 5.0).astype(np.float32)
    idx, p = random_lists(rng, n, m, k)
    with torch.cuda.device(dev):
        D = tsne._Device(dev)
        yf, ya, ia, pa = on(dev, Y), on(dev, y), on(dev, idx, np.int32), on(dev, p, np.float32)
        kla = D.place(ya, yf, ia, pa, 1.0, MOMENTUM, LEARNING_RATE, 25).cpu().numpy()
        ga = [t.cpu().numpy() for t in D.place_gradient(ya, yf, ia, pa, 2.0)]
        ya = ya.cpu().numpy()
        for i in (0, 2500, 4096):
            y1, i1, p1 = on(dev, y[i:i + 1]), on(dev, idx[i:i + 1], np.int32), on(dev, p[i:i + 1], np.float32)
            kl1 = D.place(y1, yf, i1, p1, 1.0, MOMENTUM, LEARNING_RATE, 25).cpu().numpy()
            g1 = [t.cpu().numpy() for t in D.place_gradient(y1, yf, i1, p1, 2.0)]
            assert np.array_equal(y1.cpu().numpy(), ya[i:i + 1]) and np.array_equal(kl1, kla[i:i + 1])
            assert all(np.array_equal(a, b[i:i + 1]) for a, b in zip(g1, ga))


def test_two_streams(dev, rule7):
    Xn, xf, yf, kw, one = rule7
    got = []
    with torch.cuda.device(dev):
        for s in (torch.cuda.Stream(dev), torch.cuda.Stream(dev)):
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                got.append(tsne.transform(Xn[:300], xf, yf, details=True, **kw))
            torch.cuda.current_stream().wait_stream(s)
    assert same(one, got[0], slice(0, 300)) and same(one, got[1], slice(0, 300))


# ---- 6. full placement

@pytest.fixture(scope="module")
def full(dev):
    """1500 fitted rows of the clusters embedded by tsne.tsne (max_iter = 250), 1000 held-out draws placed by the device and by
    the numpy checker (float64, and float32 for the checker's own spread)"""
    Xf, lf = clusters(1500, 20, 1)
    Xn, ln = clusters(1000, 20, 2)
    with torch.cuda.device(dev):
        xf = on(dev, Xf)
        Yf = tsne.tsne(xf, max_iter=250, random_state=0).embedding
        got = tsne.transform(Xn, xf, on(dev, Yf), details=True)
    ref = tsne.transform(Xn, Xf, Yf, backend="numpy", details=True)
    y0 = tsne.initial_placement_numpy("weighted", Yf, ref.idx, ref.p)
    return Xf, lf, Yf, Xn, ln, got, ref, checker_margin(y0, Yf, ref.idx, ref.p, ref.kl)


def test_full_placement(dev, full):
    Xf, lf, Yf, Xn, ln, got, ref, margin = full
    diff = abs(float(np.mean(got.kl)) - float(np.mean(ref.kl)))
    worse, worse_ref = float(np.mean(got.kl > got.kl_init)), float(np.mean(ref.kl > ref.kl_init))
    print("FULL mean KL_i device %.9f checker %.9f  |diff| %.3e  margin (10 x float64 / float32 spread) %.3e  worse %.4f (checker %.4f)"
          % (np.mean(got.kl), np.mean(ref.kl), diff, margin, worse, worse_ref))
    assert worse_ref == 0.0                       # the checker on these inputs: no point ends above its start
    assert np.mean(ref.kl) < np.mean(ref.kl_init)
    assert diff <= margin
    assert worse <= 0.01
    assert np.array_equal(got.idx, ref.idx)
    lab, conf = tsne.vote_labels(got.idx, got.p, lf)
    rlab, rconf = tsne.vote_labels(ref.idx, ref.p, lf)
    sure = rconf > 0.5
    assert np.mean(sure) > 0.9 and np.array_equal(lab[sure], rlab[sure])
    assert np.mean(lab == ln) > 0.95


def test_fitted_rows_are_placed_on_themselves(dev):
    X = duplicate_free()
    Y = (np.random.default_rng(2).normal(size=(len(X), 2)) * 30.0).astype(np.float32)
    with torch.cuda.device(dev):
        got = tsne.transform(on(dev, X), on(dev, X), on(dev, Y), n_iter=0, init="nearest", details=True)
    assert np.array_equal(got.embedding, Y) and np.array_equal(got.kl, got.kl_init)
    assert np.array_equal(got.idx[:, 0], np.arange(len(X)))


# ---- 7. domain

def test_arg_errors_leave_the_outputs_untouched(dev):
    L, s = api.load_library(), stream()
    f32 = lambda *shape: torch.full(shape, 7.0, device=dev)                                           # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)                       # noqa: E731
    q, x, idx, d2, pc = f32(8, 4), f32(8, 4), torch.full((8, 4), 7, dtype=torch.int32, device=dev), f64(8, 4), f64(8, 4)
    y, yf, p, g, kl, z = f32(8, 2), f32(8, 2), f32(8, 4), f32(8, 2), f64(8), f64(8)
    big = 4194305
    bad = [
        L.ra_tsne_knn_query(P(q), 0, P(x), 8, 4, 4, P(idx), P(d2), s), L.ra_tsne_knn_query(P(q), big, P(x), 8, 4, 4, P(idx), P(d2), s),
        L.ra_tsne_knn_query(P(q), 8, P(x), 0, 4, 4, P(idx), P(d2), s), L.ra_tsne_knn_query(P(q), 8, P(x), 262145, 4, 4, P(idx), P(d2), s),
        L.ra_tsne_knn_query(P(q), 8, P(x), 8, 0, 4, P(idx), P(d2), s), L.ra_tsne_knn_query(P(q), 8, P(x), 8, 2049, 4, P(idx), P(d2), s),
        L.ra_tsne_knn_query(P(q), 8, P(x), 8, 4, 0, P(idx), P(d2), s), L.ra_tsne_knn_query(P(q), 8, P(x), 8, 4, 9, P(idx), P(d2), s),
        L.ra_tsne_knn_query(P(q), 8, P(x), 400, 4, 302, P(idx), P(d2), s), L.ra_tsne_knn_query(None, 8, P(x), 8, 4, 4, P(idx), P(d2), s),
        L.ra_tsne_knn_query(P(q), 8, None, 8, 4, 4, P(idx), P(d2), s), L.ra_tsne_knn_query(P(q), 8, P(x), 8, 4, 4, None, P(d2), s),
        L.ra_tsne_knn_query(P(q), 8, P(x), 8, 4, 4, P(idx), None, s),
        L.ra_tsne_affinity_rows(P(d2), 0, 4, 3.0, P(pc), s), L.ra_tsne_affinity_rows(P(d2), big, 4, 3.0, P(pc), s),
        L.ra_tsne_affinity_rows(P(d2), 8, 0, 3.0, P(pc), s), L.ra_tsne_affinity_rows(P(d2), 8, 302, 3.0, P(pc), s),
        L.ra_tsne_affinity_rows(P(d2), 8, 4, 0.0, P(pc), s), L.ra_tsne_affinity_rows(P(d2), 8, 4, 101.0, P(pc), s),
        L.ra_tsne_affinity_rows(P(d2), 8, 4, float("nan"), P(pc), s), L.ra_tsne_affinity_rows(None, 8, 4, 3.0, P(pc), s),
        L.ra_tsne_affinity_rows(P(d2), 8, 4, 3.0, None, s),
        L.ra_tsne_place_gradient(P(y), 0, P(yf), 8, P(idx), P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), big, P(yf), 8, P(idx), P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 0, P(idx), P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 262145, P(idx), P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), P(p), 0, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), P(p), 9, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 400, P(idx), P(p), 302, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), P(p), 4, 0.5, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), P(p), 4, float("inf"), P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), P(p), 4, float("nan"), P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, None, None, None, s),
        L.ra_tsne_place_gradient(None, 8, P(yf), 8, P(idx), P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, None, 8, P(idx), P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, None, P(p), 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place_gradient(P(y), 8, P(yf), 8, P(idx), None, 4, 1.0, P(g), P(kl), P(z), s),
        L.ra_tsne_place(P(y), 0, P(yf), 8, P(idx), P(p), 4, 1.0, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), big, P(yf), 8, P(idx), P(p), 4, 1.0, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 0, P(idx), P(p), 4, 1.0, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 262145, P(idx), P(p), 4, 1.0, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 9, 1.0, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 0.99, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, 1.0, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, -0.1, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, float("nan"), 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, 0.8, 0.0, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, 0.8, float("inf"), 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, P(yf), 8, P(idx), P(p), 4, 1.0, 0.8, 0.1, -1, P(kl), s),
        L.ra_tsne_place(None, 8, P(yf), 8, P(idx), P(p), 4, 1.0, 0.8, 0.1, 5, P(kl), s),
        L.ra_tsne_place(P(y), 8, None, 8, P(idx), P(p), 4, 1.0, 0.8, 0.1, 5, P(kl), s),
    ]
    assert all(rc == -1 for rc in bad), bad            # RA_ERR_ARG
    assert b"ra_tsne_place" in L.ra_last_error()
    torch.cuda.synchronize(dev)
    for t in (q, x, d2, pc, y, yf, p, g, kl, z):
        assert bool((t == 7.0).all())
    assert bool((idx == 7).all())
    # the existing entries keep their domain: ra_tsne_affinity still ties k to n
    assert L.ra_tsne_affinity(P(d2), 8, 8, 3.0, P(pc), s) == -1
    assert L.ra_tsne_affinity_rows(P(d2), 2, 4, 3.0, P(pc), s) == 0


def test_python_errors_come_before_a_launch(dev, monkeypatch):
    launched = []
    monkeypatch.setattr(tsne._Device, "__init__", lambda self, where: launched.append(where))
    Xf, Yf, Xn = torch.zeros((40, 3), device=dev), torch.zeros((40, 2), device=dev), torch.zeros((5, 3), device=dev)
    for bad in (dict(perplexity=50.0), dict(n_iter=-1), dict(batch=262145), dict(init="pca"), dict(momentum=1.0),
                dict(exaggeration=0.5), dict(learning_rate=0.0)):
        with pytest.raises(tsne.TsneError):
            tsne.transform(Xn, Xf, Yf, **dict(dict(perplexity=5.0), **bad))
    for a, b, c in ((Xn.double(), Xf, Yf), (Xn, Xf[:39], Yf), (Xn, Xf, Yf[:, :1]), (torch.zeros((5, 4), device=dev), Xf, Yf),
                    (Xn, Xf.cpu(), Yf), (torch.full((5, 3), float("nan"), device=dev), Xf, Yf)):
        with pytest.raises(tsne.TsneError):
            tsne.transform(a, b, c, perplexity=5.0)
    with pytest.raises(tsne.TsneError):
        tsne.tsne(torch.zeros((262145, 2), device=dev))                  # the fit keeps its limit
    with pytest.raises(tsne.TsneError):
        tsne.tsne_large(torch.zeros((100, 3), device=dev), 101)
    assert tsne.transform(Xn[:0], Xf, Yf, perplexity=5.0).shape == (0, 2)
    assert not launched


# ---- 8. the tool

def test_tool_modes(dev, tmp_path):
    X, lab = clusters(1000, 20, 9)
    np.save(tmp_path / "all.npy", X)
    assert tsne.main([str(tmp_path / "all.npy"), str(tmp_path / "large.npz"), "--fit_size", "600", "--seed", "4", "--max_iter", "250"]) == 0
    o = np.load(tmp_path / "large.npz")
    fit = tsne.draw_fit_rows(1000, 600, 4)
    rest = np.setdiff1d(np.arange(1000), fit)
    assert np.array_equal(o["fit_indices"], fit) and o["embedding"].shape == (1000, 2)
    assert np.all(np.isnan(o["kl_point"][fit])) and np.all(np.isfinite(o["kl_point"][rest]))

    # the device's mean KL_i against the numpy checker's on the same inputs, by test_full_placement's rule
    Yf = o["embedding"][fit]
    ref = tsne.transform(X[rest], X[fit], Yf, backend="numpy", details=True)
    margin = checker_margin(tsne.initial_placement_numpy("weighted", Yf, ref.idx, ref.p), Yf, ref.idx, ref.p, ref.kl)

    def held(kl_dev, tag):
        diff = abs(float(np.mean(kl_dev)) - float(np.mean(ref.kl)))
        print("TOOL %s mean KL_i device %.9f checker %.9f |diff| %.3e margin %.3e" % (tag, np.mean(kl_dev), np.mean(ref.kl), diff, margin))
        assert diff <= margin

    held(o["kl_point"][rest], "--fit_size")
    # --place_into: the stored fit, the 400 other rows, with labels; against the tool's own numpy backend
    np.savez(tmp_path / "fit_out.npz", embedding=Yf, perplexity=np.float64(30.0))
    np.save(tmp_path / "fit_in.npy", X[fit])
    np.save(tmp_path / "new.npy", X[rest])
    np.save(tmp_path / "labels.npy", lab[fit])
    common = ["--place_into", str(tmp_path / "fit_out.npz"), "--fit_input", str(tmp_path / "fit_in.npy"), "--fit_labels",
              str(tmp_path / "labels.npy")]
    assert tsne.main([str(tmp_path / "new.npy"), str(tmp_path / "placed.npz")] + common) == 0
    assert tsne.main([str(tmp_path / "new.npy"), str(tmp_path / "placed_np.npz"), "--backend", "numpy"] + common) == 0
    d, c = np.load(tmp_path / "placed.npz"), np.load(tmp_path / "placed_np.npz")
    held(d["kl_point"], "--place_into")
    assert np.array_equal(c["kl_point"], ref.kl) and np.array_equal(c["embedding"], ref.embedding)
    with torch.cuda.device(dev):
        got = tsne.transform(X[rest], X[fit], Yf, details=True)
    want = tsne.vote_labels(got.idx, got.p, lab[fit])
    assert np.array_equal(d["embedding"], got.embedding) and np.array_equal(d["kl_point"], got.kl)
    assert np.array_equal(d["labels"], want[0]) and np.array_equal(d["label_confidence"], want[1])
    assert np.mean(d["labels"] == lab[rest]) > 0.95
