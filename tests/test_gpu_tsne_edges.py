"""The t-SNE kernels entry by entry at their list, lane and segment edges, on the inputs of tests/test_tsne_edges_cpu.py (whose
properties that file asserts without a GPU).  Integer coordinates and counted embeddings make every value exact, so neighbour
sets, distances, Z and the counted gradients are compared for equality; the real-valued cases use the bounds that file derives
from term counts and the float64 reference.  Each toleranced test prints its largest error / bound ratio."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, tsne  # noqa: E402
from test_tsne_edges_cpu import (AFF_CASES, AFF_SCALES, COUNTED_N, COUNTED_PAIRS, FEATURE_D, GAP_D, GRAD_N,  # noqa: E402
                                 GRAD_SCALES, LEARNING_RATE, LINE_CASES, MOMENTUM, U53, affinity_blocks, affinity_case,
                                 affinity_pair, counted_case, entropy_bound, feature_case, gap_case, gradient_case, grid_case,
                                 identical_case, line_case, step_case)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on(dev, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def check_knn_exact(dev, X, idx, d2):
    got_i, got_d = tsne.knn(on(dev, X), idx.shape[1])
    assert np.array_equal(got_i, idx), np.argwhere(got_i != idx)[:10]
    assert np.array_equal(got_d, d2), np.argwhere(got_d != d2)[:10]


# ---- 1. kNN, exact

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n,k", LINE_CASES)
def test_knn_line(dev, n, k, reverse):
    check_knn_exact(dev, *line_case(n, k, reverse))


def test_knn_identical_points(dev):
    check_knn_exact(dev, *identical_case())


@pytest.mark.parametrize("k", [8, 91])
def test_knn_grid(dev, k):
    check_knn_exact(dev, *grid_case(k))


@pytest.mark.parametrize("d", FEATURE_D)
def test_knn_feature_dimension(dev, d):
    check_knn_exact(dev, *feature_case(d))


# ---- 2. kNN, real-valued with a planted gap

@pytest.mark.parametrize("shifted", [False, True])
def test_knn_planted_gap(dev, shifted):
    X, idx, d2, rk, rk1 = gap_case(shifted)
    got_i, got_d = tsne.knn(on(dev, X), idx.shape[1])
    assert np.array_equal(got_i, idx), np.argwhere(got_i != idx)[:10]
    bound = (GAP_D + 2) * U53 * d2
    ratio = float(np.max(np.abs(got_d - d2) / bound))
    print("RATIO knn dist2 shifted=%d %.3f" % (shifted, ratio))
    assert np.all(np.abs(got_d - d2) <= bound)


# ---- 3. perplexity search

def check_affinity(dev, perplexity, D, Pref, marginal, conv, rel, ab, a, s, tiny, tag):
    n, k = D.shape
    got = tsne._Device(dev).affinity(on(dev, D, np.float64), perplexity).cpu().numpy()
    ok = ~marginal
    err = np.abs(got - Pref)[ok]
    bound = (rel[:, None] * Pref + ab[:, None])[ok]
    ratio = float(np.max(err / bound))
    print("RATIO affinity %s %.3f (marginal %d, floor flag %d)" % (tag, ratio, int(marginal.sum()), int(tiny.sum())))
    assert np.all(err <= bound), np.argwhere(err > bound)[:10]
    rows = np.nonzero(ok & conv)[0]
    if rows.size:
        g = got[rows]
        sums = np.array([math.fsum(r) for r in g])
        assert np.all(np.abs(sums - 1.0) <= (k + 8) * 2.0 ** -52)
        with np.errstate(divide="ignore", invalid="ignore"):
            H = -np.sum(np.where(g > 0, g * np.log(g), 0.0), axis=1)
        hb = float(np.float32(1e-5)) + entropy_bound(rel, a, s)[rows]
        herr = np.abs(H - np.log(float(np.float32(perplexity))))
        print("RATIO entropy %s %.3f" % (tag, float(np.max(herr / hb))))
        assert np.all(herr <= hb), rows[herr > hb][:10]
    return got


@pytest.mark.parametrize("scale", AFF_SCALES)
@pytest.mark.parametrize("k,perplexity", AFF_CASES)
def test_affinity_lanes(dev, k, perplexity, scale):
    check_affinity(dev, perplexity, *affinity_case(k, perplexity, scale), tag="k=%d scale=%g" % (k, scale))


def test_affinity_equal_and_zero_rows(dev):
    got = check_affinity(dev, 20.0, *affinity_blocks(), tag="blocks")
    assert np.all(got[128:256] == 1.0 / 64)                                # exp(0) = 1, 64 / 64 of it: exact
    assert np.all(got[256:] == 0.0)                                        # the search ends on the sum_p == 0 floor


def test_affinity_two_points(dev):
    got = check_affinity(dev, 1.5, *affinity_pair(), tag="n=2")
    assert np.all(got == 1.0)


# ---- 4. repulsion and Z, counted

def run_error(dev, Y, csr, exaggeration):
    """ra_tsne_error: (gradient [n][2] float32, KL, squared gradient norm)"""
    n = Y.shape[0]
    lib = api.load_library()
    y = on(dev, Y, np.float32)
    ip, ix, pv = on(dev, csr[0], np.int32), on(dev, csr[1], np.int32), on(dev, csr[2], np.float32)
    g = torch.empty((n, 2), dtype=torch.float32, device=dev)
    st = torch.empty(2, dtype=torch.float64, device=dev)
    api._check(lib.ra_tsne_error(P(y), n, P(ip), P(ix), P(pv), int(ix.numel()), float(exaggeration), P(g), P(st), stream()),
               "ra_tsne_error")
    st = st.cpu().numpy()
    return g.cpu().numpy(), float(st[0]), float(st[1])


def empty_csr(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)


def test_rcp_of_two_is_one_half(dev):
    """the probe of the counted cases: two points at distance 1, Z = 2 v_rcp_f32(2) must be exactly 1"""
    Y, Z, grad, gn, counts = counted_case(2, 0)
    g, kl, got_gn = run_error(dev, Y, empty_csr(2), 1.0)
    assert Z == 1.0 and np.array_equal(g, grad) and np.array_equal(g, np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32))
    assert kl == 0.0 and got_gn == 2.0


@pytest.mark.parametrize("pair", range(len(COUNTED_PAIRS)))
@pytest.mark.parametrize("n", COUNTED_N)
def test_counted_repulsion_and_z(dev, n, pair):
    Y, Z, grad, gn, counts = counted_case(n, pair)
    g, kl, got_gn = run_error(dev, Y, empty_csr(n), 1.0)
    assert np.array_equal(g, grad), (np.argwhere(g != grad)[:10], counts)
    assert kl == 0.0
    assert abs(got_gn - gn) <= n * 2.0 ** -52 * gn


# ---- 5. gradient, statistics and one step, real-valued

def check_gradient(dev, case, tag):
    Y, csr, exag, kl, g, gb, klb, gn, gnb = case
    got, got_kl, got_gn = run_error(dev, Y, csr, exag)
    err = np.abs(got - g)
    print("RATIO gradient %s %.4f  kl %.4f  norm %.4f" % (tag, float(np.max(err / gb)), abs(got_kl - kl) / klb,
                                                            abs(got_gn - gn) / gnb))
    assert np.all(err <= gb), np.argwhere(err > gb)[:10]
    assert abs(got_kl - kl) <= klb
    assert abs(got_gn - gn) <= gnb


@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("n", GRAD_N)
def test_gradient_and_statistics(dev, n, scale):
    check_gradient(dev, gradient_case(n, scale), "n=%d scale=%g" % (n, scale))


def test_gradient_hostile_csr(dev):
    check_gradient(dev, gradient_case(1025, 5.0, True), "hostile")


@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("n", GRAD_N)
def test_one_step(dev, n, scale):
    Y, csr, exag, kl, g, gb, klb, gn, gnb = gradient_case(n, scale)
    upd, gains, new_gains, decided, new_upd, ub, new_y, yb = step_case(n, scale)
    with torch.cuda.device(dev):
        y1, u1, g1, got_kl, got_gn = tsne.step(Y, csr, upd, gains, exag, MOMENTUM, LEARNING_RATE)
    assert np.array_equal(g1[decided], new_gains[decided]), np.argwhere((g1 != new_gains) & decided)[:10]
    uerr, yerr = np.abs(u1 - new_upd)[decided], np.abs(y1 - new_y)[decided]
    print("RATIO step n=%d scale=%g update %.4f  y %.4f  kl %.4f" % (n, scale, float(np.max(uerr / ub[decided])),
                                                                     float(np.max(yerr / yb[decided])), abs(got_kl - kl) / klb))
    assert np.all(uerr <= ub[decided]) and np.all(yerr <= yb[decided])
    assert abs(got_kl - kl) <= klb
    # an undecided entry took one of the two branches
    other = np.maximum(np.where(upd.astype(np.float64) * g < 0.0, gains * np.float32(0.8), gains + np.float32(0.2)),
                       np.float32(0.01)).astype(np.float32)
    assert np.all((g1 == new_gains) | (g1 == other))
