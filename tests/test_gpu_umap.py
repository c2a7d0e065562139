"""UMAP on the device (csrc/ralign_umap.h behind cryo_ralib_amd.umap): the three entries entry by entry against the float64 checker
from states built on the host and handed to both sides (tests/umap_cases.py; tests/test_umap_cpu.py asserts what the builders
promise), then whole calls: bitwise repeatability call to call, stream to stream and in pieces, the device graph, and the scores of
the blob case next to the checker's.

The kernels' tile constants (ralign_umap.h): the calibration runs one wave per row, SK_ROWS = 4 rows a workgroup, lane l holding the
entries l, l + 64, ...; the epoch and the placement share a row among LANES = 16 lanes, ROWS = 16 rows a workgroup.  u = 2^-53.

ra_umap_smooth_knn.  rho is a selection and a square root: one ulp.  Every sigma must satisfy rule 2's stop condition evaluated by the
checker (slack 1e-9 for the different summation order), or be the floor bit for bit, or, on a row that ran into rule 2's limit of
64 trips above its floor (a row of duplicates only), be the checker's sigma bit for bit.  On the rows whose bisection stayed MARGIN = 1e-9 away from
every branch in the checker, the device took the same branches, so mid is the same number; the floor's mean is added in list order
on both sides, so sigma is the same too, and w differs by one exp and one division: inside the 4 (k + 2) u relative that the
different order of psum's k additions is given.

One ra_umap_epochs epoch.  Both sides form the same terms in double in the same order with unfused arithmetic; they differ in pow
alone, which OpenCL allows POW_ULPS = 16 ulps.  A term is at most 8 in magnitude (a clipped move of 4, doubled for the attraction)
and pow enters it through at most four operations, so the sums behind a coordinate differ by at most
    E_i = terms_i x 8 alpha_t x 4 (POW_ULPS + 8) u          (umap_cases.epoch_bound)
which the CPU file shows to be below half a float32 ulp of every result of these cases: the two roundings to float32 can differ only
when a rounding boundary lies between the two doubles, and then by one ulp.  Every coordinate is within one float32 ulp."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import umap_cases as uc  # noqa: E402
from cryo_ralib_amd import _graph, api, umap  # noqa: E402

RA_ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- ra_umap_smooth_knn

SMOOTH = uc.smooth_cases()


@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_smooth_knn_entries(dev, name):
    d2, nn = SMOOTH[name]
    rows, k = d2.shape
    sk = umap.smooth_knn_numpy(d2, nn)
    rho, sigma, w = (t.cpu().numpy() for t in umap._Device(dev).smooth_knn(up(d2, dev), nn))
    assert np.all(np.abs(rho - sk.rho) <= np.spacing(sk.rho))
    x = np.sqrt(d2) - sk.rho[:, None]
    mid_ok = np.abs(umap.psum_numpy(x, sigma) - np.log2(float(nn))) < 1e-5 + 1e-9
    on_floor = sigma == 1e-3 * (umap._list_sum(np.sqrt(d2)) / k)    # the mean in list order on both sides: the same bits
    # a row of duplicates only (rho = 0, psum = k at every sigma, floor 0) halves mid for 64 trips and ends at 2^-64 with neither
    # condition met: rule 2's trip limit, where the device must hold the checker's bits
    at_limit = ~sk.stopped & ~sk.floored & (sigma == sk.sigma)
    assert np.all(mid_ok | on_floor | at_limit)
    keep = sk.margin >= uc.MARGIN
    assert np.mean(~keep) <= uc.MAX_LEFT_OUT
    tol = 4 * (k + 2) * uc.U
    bad_s = np.nonzero(keep & ~(np.abs(sigma - sk.sigma) <= tol * sk.sigma))[0]
    assert not len(bad_s), (bad_s, sigma[bad_s], sk.sigma[bad_s])
    bad_w = np.argwhere(keep[:, None] & ~(np.abs(w - sk.w) <= tol * sk.w))
    assert not len(bad_w), (bad_w, [(w[i, j], sk.w[i, j]) for i, j in bad_w[:8]])
    assert np.all((w == 1.0) == (sk.w == 1.0))


def test_smooth_knn_rejections(dev, lib):
    d2 = up(uc.smooth_rows(4, 14, 1), dev)
    out = [torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev),
           torch.zeros((4, 14), dtype=torch.float64, device=dev)]
    for rows, k, nn in ((0, 14, 15), (4, 0, 15), (4, 302, 15), (4, 14, 1), (4, 14, 303)):
        assert lib.ra_umap_smooth_knn(P(d2), rows, k, nn, P(out[0]), P(out[1]), P(out[2]), stream()) == RA_ERR_ARG
    assert lib.ra_umap_smooth_knn(None, 4, 14, 15, P(out[0]), P(out[1]), P(out[2]), stream()) == RA_ERR_ARG
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in out)


# ---- one ra_umap_epochs epoch

EPOCH = uc.epoch_cases()


def run_epochs(lib, dev, case, Y, t0, count, seed=42, gamma=1.0, lr=1.0, indices=None):
    y, alt = up(Y, dev), torch.full((case.n, 2), 77.0, dtype=torch.float32, device=dev)
    before = y.clone()
    ix = case.indices if indices is None else indices
    ip, ixd, rt = up(case.indptr, dev), up(ix, dev), up(case.rate, dev)
    rc = lib.ra_umap_epochs(P(y), P(alt), case.n, P(ip), P(ixd), P(rt), len(ix), uc.A, uc.B, gamma, case.neg, lr, case.n_epochs, t0, count,
                            seed, stream())
    torch.cuda.synchronize()
    return rc, y, alt, before


@pytest.mark.parametrize("name", sorted(EPOCH))
def test_epoch_entries(dev, lib, name):
    case = EPOCH[name]
    differing = []
    for t in (1, 2, case.n_epochs):                                 # t = 1, epoch0 > 1, t = n_epochs
        rc, y, alt, before = run_epochs(lib, dev, case, case.Y, t, 1)
        assert rc == 0
        assert torch.equal(y, before)                               # the input buffer keeps its bits
        got, ref = alt.cpu().numpy(), case.reference(t)
        assert np.all(np.isfinite(got))
        assert np.all(np.abs(got.astype(np.float64) - ref) <= uc.ulp32(ref)), (name, t)
        differing.append(float(np.mean(got != ref)))
    print("%s: share of coordinates that differ from the checker by one ulp: %s" % (name, differing))


def test_epoch_seeds_and_strengths(dev, lib):
    case = EPOCH["n33"]
    a = run_epochs(lib, dev, case, case.Y, 1, 1, seed=1)[2].cpu().numpy()
    b = run_epochs(lib, dev, case, case.Y, 1, 1, seed=2)[2].cpu().numpy()
    assert not np.array_equal(a, b)
    for seed, got in ((1, a), (2, b)):
        ref = case.reference(1, seed=seed)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= uc.ulp32(ref))
    got = run_epochs(lib, dev, case, case.Y, 3, 1, gamma=0.5, lr=0.25)[2].cpu().numpy()
    ref = case.reference(3, gamma=0.5, lr=0.25)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= uc.ulp32(ref))


def test_epochs_ping_pong(dev, lib):
    """count epochs in one call equal the same epochs one call at a time; the parity of count names the buffer"""
    case = EPOCH["n33"]
    rc, y, alt, _ = run_epochs(lib, dev, case, case.Y, 2, 5)
    assert rc == 0
    Y = case.Y
    for t in range(2, 7):
        Y = run_epochs(lib, dev, case, Y, t, 1)[2].cpu().numpy()
    assert np.array_equal(alt.cpu().numpy(), Y)                     # five epochs: the result is in d_y_alt
    rc, y, alt, _ = run_epochs(lib, dev, case, case.Y, 2, 4)
    Y4 = case.Y
    for t in range(2, 6):
        Y4 = run_epochs(lib, dev, case, Y4, t, 1)[2].cpu().numpy()
    assert np.array_equal(y.cpu().numpy(), Y4)                      # four: in d_y


def test_epochs_rejections(dev, lib):
    case = EPOCH["n33"]
    bad = case.indices.copy()
    bad[len(bad) // 2] = case.n                                     # a column index >= n
    rc, y, alt, before = run_epochs(lib, dev, case, case.Y, 1, 1, indices=bad)
    assert rc == RA_ERR_ARG
    assert torch.equal(y, before) and bool((alt == 77.0).all())     # nothing is written
    y, alt = up(case.Y, dev), torch.full((case.n, 2), 77.0, dtype=torch.float32, device=dev)
    ip, ix, rt = up(case.indptr, dev), up(case.indices, dev), up(case.rate, dev)
    nnz = len(case.indices)

    def call(n=case.n, a=uc.A, gamma=1.0, neg=5, lr=1.0, n_epochs=20, t0=1, count=1, y2=alt):
        return lib.ra_umap_epochs(P(y), P(y2), n, P(ip), P(ix), P(rt), nnz, a, uc.B, gamma, neg, lr, n_epochs, t0, count, 42, stream())
    for kw in (dict(n=3), dict(n=262145), dict(a=0.0), dict(gamma=-1.0), dict(neg=17), dict(neg=-1), dict(lr=0.0), dict(n_epochs=0),
               dict(n_epochs=10001), dict(t0=0), dict(count=0), dict(t0=20, count=2), dict(y2=y)):
        assert call(**kw) == RA_ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((alt == 77.0).all()) and np.array_equal(y.cpu().numpy(), case.Y)


# ---- ra_umap_place

PLACE = uc.place_cases()


def run_place(lib, dev, case, n_epochs, rows=None, row0=0, seed=42):
    rows = slice(None) if rows is None else rows
    y = up(case.y0[rows], dev)
    idx, rate, yf = up(case.idx[rows], dev), up(case.rate[rows], dev), up(case.Yfit, dev)
    rc = lib.ra_umap_place(P(y), int(y.shape[0]), row0, P(yf), case.m, P(idx), P(rate), case.k, uc.A, uc.B, 1.0, case.neg, 1.0, n_epochs,
                           seed, stream())
    torch.cuda.synchronize()
    assert rc == 0
    return y.cpu().numpy()


@pytest.mark.parametrize("name", sorted(PLACE))
def test_place_entries(dev, lib, name):
    case = PLACE[name]
    got, ref = run_place(lib, dev, case, 1), case.reference(1)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= uc.ulp32(ref))    # one epoch: the epoch kernel's bound
    # the same after three epochs: a coordinate whose rounding differed in an earlier epoch (a share of about E / ulp, 1e-5, of
    # them) would feed a different position to the next one and could show here as more than one ulp
    got3, ref3 = run_place(lib, dev, case, 3), case.reference(3)
    assert np.all(np.abs(got3.astype(np.float64) - ref3) <= uc.ulp32(ref3))


def test_place_is_batch_independent(dev, lib):
    big = uc.PlaceCase(257, 80, 15, 90)
    whole = run_place(lib, dev, big, 4)
    alone = run_place(lib, dev, big, 4, rows=slice(200, 201), row0=200)
    assert np.array_equal(alone[0], whole[200])
    part = run_place(lib, dev, big, 4, rows=slice(100, 257), row0=100)
    assert np.array_equal(part, whole[100:])
    shifted = run_place(lib, dev, big, 4, rows=slice(200, 201), row0=0)         # another key index: other samples
    assert not np.array_equal(shifted[0], whole[200])


def test_place_far_rows(dev, lib):
    """the key index is formed in 64 bits: a batch past 4 194 304 rows, and the last rows the domain takes, against the checker"""
    case = PLACE["k15"]
    for row0 in (5000000, 2 ** 48 - case.n):
        got, ref = run_place(lib, dev, case, 2, row0=row0), case.reference(2, row0=row0)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= uc.ulp32(ref))
        assert not np.array_equal(got, run_place(lib, dev, case, 2))


def test_place_rejections(dev, lib):
    case = PLACE["k15"]
    y, yf = up(case.y0, dev), up(case.Yfit, dev)
    idx, rate = up(case.idx, dev), up(case.rate, dev)

    def call(n=case.n, row0=0, m=case.m, k=case.k, neg=5, n_epochs=3):
        return lib.ra_umap_place(P(y), n, row0, P(yf), m, P(idx), P(rate), k, uc.A, uc.B, 1.0, neg, 1.0, n_epochs, 42, stream())
    for kw in (dict(n=0), dict(row0=-1), dict(row0=2 ** 48 - case.n + 1), dict(m=1), dict(k=0), dict(k=case.m + 1), dict(neg=17), dict(n_epochs=0)):
        assert call(**kw) == RA_ERR_ARG, kw
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), case.y0)


# ---- whole calls

@pytest.fixture(scope="module")
def blob():
    X, truth = uc.blobs()
    return X, truth


@pytest.fixture(scope="module")
def fits(blob, dev):
    X, truth = blob
    ref = umap.umap(X, n_epochs=200, init="pca", backend="numpy")
    got = umap.umap(up(X, dev), n_epochs=200, init="pca")
    return ref, got


def test_calls_and_streams_give_the_same_bits(blob, fits, dev):
    X, _ = blob
    again = umap.umap(up(X, dev), n_epochs=200, init="pca")
    assert np.array_equal(again.embedding, fits[1].embedding)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        other = umap.umap(up(X, dev), n_epochs=200, init="pca")
    side.synchronize()
    assert np.array_equal(other.embedding, fits[1].embedding)


def test_one_call_equals_eight(blob, fits, dev):
    X, _ = blob
    res = fits[1]
    indptr, indices, s = res.graph
    kw = dict(a=res.a, b=res.b, n_epochs=200)
    with torch.cuda.device(dev):
        Y = umap.pca_start(X)
        for e0 in range(1, 200, 25):
            Y = umap.layout(indptr, indices, s, Y, epoch0=e0, count=25, **kw)
    assert np.array_equal(Y, res.embedding)


def test_device_graph(blob, fits, dev):
    """indptr and indices equal the checker's.  s is compared at the calibration's bound eps = 4 (k + 2) u, relative, with the
    checker's rules 2 and 3 applied to the device's own lists.  The calibration's bound is one for equal inputs, and the two kNNs
    add the squares of a distance in different orders (ra_tsne_knn the features in order, tsne.knn_numpy as numpy.sum does); rule 2
    magnifies a relative d u of d_ij by d_ij / sigma in the exponent.  Against the checker's own graph the same bound is asserted
    on the entries both of whose rows got bitwise equal distances from the two kNNs; over all entries the worst relative difference
    is printed (observed 7.2e-15 = 65 u against eps = 64 u).  Why eps carries over from w to s: with w' = w (1 + e), |e| <= eps, the first-order
    change of s = w1 + w2 - w1 w2 is w1 e1 (1 - w2) + w2 e2 (1 - w1) <= eps (w1 + w2 - 2 w1 w2) <= eps s."""
    from cryo_ralib_amd import tsne
    ref, got = fits
    assert np.array_equal(got.graph[0], ref.graph[0]) and np.array_equal(got.graph[1], ref.graph[1])
    idx, d2 = tsne.knn(up(blob[0], dev), 14)
    sk = umap.smooth_knn_numpy(d2, 15)
    indptr, indices, s = umap._union_numpy(idx, sk.w)
    assert np.array_equal(indptr, got.graph[0]) and np.array_equal(indices, got.graph[1])
    keep = sk.margin >= uc.MARGIN
    assert np.mean(~keep) <= uc.MAX_LEFT_OUT
    both = keep[_graph.row_ids_numpy(indptr.astype(np.int64))] & keep[indices]
    tol = 4 * (14 + 2) * uc.U
    rel = np.abs(got.graph[2] - s)[both] / s[both]
    print("s against rules 2 - 3 on the device's lists: worst %.3g of the bound; against the checker's own graph: worst relative %.3g"
          % (rel.max() / tol, (np.abs(got.graph[2] - ref.graph[2]) / ref.graph[2]).max()))
    assert np.all(rel <= tol)
    assert np.all(np.abs(got.rho - sk.rho) <= np.spacing(sk.rho))
    same = np.all(tsne.knn_numpy(blob[0], 14)[1] == d2, axis=1) & keep
    same2 = same[_graph.row_ids_numpy(indptr.astype(np.int64))] & same[indices]
    print("rows with bitwise equal distances from the two kNNs: %.3f; entries between two such rows: %.3f" % (same.mean(), same2.mean()))
    assert np.all(np.abs(got.graph[2] - ref.graph[2])[same2] <= tol * ref.graph[2][same2])
    rows = _graph.row_ids_numpy(got.graph[0].astype(np.int64))
    S = np.zeros((1500, 1500))
    S[rows, got.graph[1]] = got.graph[2]
    assert np.array_equal(S, S.T)


def test_scores_next_to_the_checker(blob, fits):
    """trajectories of the two backends may part after many epochs (a one-ulp difference feeds the next epoch), so the scores are
    compared, not the points.  The margin is three times the spread of the checker's own scores over its seeds."""
    from sklearn.manifold import trustworthiness
    from sklearn.metrics import silhouette_score
    X, truth = blob
    ref, got = fits

    def scores(Y):
        return trustworthiness(X, Y, n_neighbors=15), silhouette_score(Y, truth)
    own = np.array([scores(umap.umap(X, n_epochs=200, init="pca", random_state=seed, backend="numpy").embedding) for seed in (1, 2)]
                   + [scores(ref.embedding)])
    margin = 3.0 * (own.max(axis=0) - own.min(axis=0))
    dev_scores = np.array(scores(got.embedding))
    print("checker scores over seeds:", own.tolist(), "device:", dev_scores.tolist(), "margin:", margin.tolist())
    assert np.all(np.isfinite(got.embedding))
    assert np.all(np.abs(dev_scores - own[-1]) <= margin)


def test_transform_on_the_device(blob, fits, dev):
    from cryo_ralib_amd import tsne
    X, truth = blob
    res = fits[1]
    fit, held = np.arange(100, 1500), np.arange(0, 100)
    Xf, Yf = up(X[fit], dev), up(res.embedding[fit], dev)
    kw = dict(a=res.a, b=res.b, n_epochs=30)
    det = umap.transform(X[held], Xf, Yf, details=True, **kw)
    for batch in (1, 33):
        assert np.array_equal(umap.transform(X[held], Xf, Yf, batch=batch, **kw), det.embedding)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        other = umap.transform(up(X[held], dev), Xf, Yf, **kw)
    side.synchronize()
    assert np.array_equal(other, det.embedding)
    chk = umap.transform(X[held], X[fit], res.embedding[fit], details=True, backend="numpy", **kw)
    assert np.array_equal(det.idx, chk.idx)
    assert np.all(np.abs(det.start.astype(np.float64) - chk.start) <= uc.ulp32(chk.start))
    assert np.array_equal(tsne.vote_labels(det.idx, det.w, truth[fit])[0], truth[held])
    # the placed rows land in their blob: nearer to its fitted rows' centre than to any other's
    cent = np.stack([res.embedding[fit][truth[fit] == c].mean(axis=0) for c in range(6)])
    assert np.array_equal(np.argmin(np.linalg.norm(det.embedding[:, None] - cent[None], axis=2), axis=1), truth[held])
    assert umap.transform(np.zeros((0, 10), np.float32), Xf, Yf, **kw).shape == (0, 2)
