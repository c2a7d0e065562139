"""Trustworthiness and continuity on the device (ra_tsne_knn and ra_embed_ranks behind cryo_ralib_amd.quality): the scikit-learn
1.7.2 pins of tests/golden/quality_ref.npz, the shapes around the kernel's tiles and list chunks entry by entry against the float64
numpy backend, unquantised data, the penalties, bitwise repeatability, sampling, the C entry's rejections, both tools and the
recovery of misplaced points.

Every rank comparison is an equality.  The pins sit on a 1/1024 grid and the generated cases on a 1/64 grid: every term of D2 is
exact in double, so the device's fused multiply-adds and numpy's unfused ones give the same bits and ties are ties on both sides.
The unquantised case first asserts, on the CPU, that no column lies within d 2^-50 thr of a listed entry's threshold (the two
chains differ by at most d 2^-52 D2), and then asks for equality everywhere."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, quality, tsne  # noqa: E402
from cryo_ralib_amd._common import d2_rows  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_ref.npz")
KC = 24             # list entries per pass of emb_rank_kernel (csrc/ralign_quality.h)
KS = [1, KC - 1, KC, KC + 1, 2 * KC + 1]


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


def c_ranks(dev, X, idx, want_rank=True, want_pen=True):
    """ra_embed_ranks through the C entry: (rc, rank or None, pen or None) as numpy arrays"""
    lib = api.load_library()
    n, d = X.shape
    k = idx.shape[1]
    x = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(dev)
    ix = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    rank = torch.full((n, k), -7, dtype=torch.int32, device=dev) if want_rank else None
    pen = torch.full((n,), -7, dtype=torch.int64, device=dev) if want_pen else None
    rc = lib.ra_embed_ranks(P(x), n, d, P(ix), k, P(rank), P(pen), stream())
    torch.cuda.synchronize()
    return rc, None if rank is None else rank.cpu().numpy(), None if pen is None else pen.cpu().numpy()


@pytest.mark.parametrize("c", "abcd")
def test_device_equals_the_pins(dev, z, c):
    X, Y, k = z["X_" + c], z["Y_" + c], int(z["k_" + c])
    t = quality.trustworthiness(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), k, details=True)
    cc = quality.continuity(X, Y, k, details=True)                  # numpy arrays are copied to the device
    print("pin %s: T %.15f (sklearn %+.1e), C %.15f (%+.1e), ranks differ at %d and %d" % (
        c, t.score, t.score - float(z["T_" + c]), cc.score, cc.score - float(z["C_" + c]),
        np.count_nonzero(t.ranks != z["rank_t_" + c]), np.count_nonzero(cc.ranks != z["rank_c_" + c])))
    assert t.ranks.dtype == np.int32 and np.array_equal(t.ranks, z["rank_t_" + c]) and np.array_equal(cc.ranks, z["rank_c_" + c])
    assert abs(t.score - float(z["T_" + c])) <= 1e-12 and abs(cc.score - float(z["C_" + c])) <= 1e-12
    assert abs(t.score - t.point.mean()) <= 1e-14 and abs(cc.score - cc.point.mean()) <= 1e-14
    r = quality.embedding_quality(X, Y, k)
    assert r.trustworthiness == t.score and r.continuity == cc.score and np.array_equal(r.trust_point, t.point)
    ref = quality.embedding_quality(X, Y, k, backend="numpy")
    assert np.array_equal(r.qnx, ref.qnx) and np.array_equal(r.lcmc, ref.lcmc) and r.k_best == ref.k_best


def tie_case(n, d, k, seed):
    """points on a coarse 1/64 grid with duplicate rows, and lists [n][k] that hold for every row, rotating through the
    positions: the farthest column (no column's D2 exceeds its threshold), the nearest, a duplicate of the row where there is
    one, the invalid entries -1, n and i, and a repeated entry"""
    rng = np.random.default_rng(seed)
    X = (rng.integers(-5, 6, size=(n, d)) / 64.0).astype(np.float32)
    X[n // 2] = X[0]
    X[n - 1] = X[0]
    D = d2_rows(X.astype(np.float64), 0, n)
    np.fill_diagonal(D, np.inf)
    near = np.argmin(D, axis=1)
    np.fill_diagonal(D, -np.inf)
    far = np.argmax(D, axis=1)
    idx = rng.integers(0, n, size=(n, k))
    dup = {0: n // 2, n // 2: n - 1, n - 1: 0}
    for i in range(n):
        special = [far[i], near[i], dup.get(i, near[i]), -1, n, i]
        for s, v in enumerate(special):
            if s < k or (i + s) % 6 == 0:
                idx[i, (i + s) % k] = v
        if k >= 8:
            idx[i, (i + 7) % k] = idx[i, (i + 1) % k]               # the nearest column again
    return X, idx, near, far


@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 65])
@pytest.mark.parametrize("n", [3, 63, 64, 65, 127, 129, 257])
def test_shapes_entry_by_entry(dev, n, d):
    for k in KS:
        X, idx, near, far = tie_case(n, d, k, 1000 * n + 10 * d + k)
        ref = quality.neighbor_ranks(X, idx, backend="numpy")
        got = quality.neighbor_ranks(torch.from_numpy(X).to(dev), idx)
        bad = np.argwhere(got != ref)
        print("n = %d, d = %d, k = %d: %d of %d ranks differ%s" % (n, d, k, len(bad), ref.size, "" if not len(bad) else
              ", first at %s: %d for %d" % (bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])))
        assert got.dtype == np.int32 and got.shape == (n, k)
        assert np.array_equal(got, ref)
        rows = np.arange(n)[:, None]
        invalid = (idx < 0) | (idx >= n) | (idx == rows)
        assert np.all(got[invalid] == 0) and np.all((got[~invalid] >= 1) & (got[~invalid] <= n - 1))
        for i in range(n):                                          # a repeated entry has one rank
            _, first, inv = np.unique(idx[i], return_index=True, return_inverse=True)
            assert np.array_equal(got[i], got[i][first][inv])
        if k >= 8:
            # the farthest column under rule 2 has rank n - 1; the nearest has rank 1 unless a lower index ties with it
            Dn = d2_rows(X.astype(np.float64), 0, n)
            for i in range(n):
                t = (i + 0) % k
                if idx[i, t] == far[i] and far[i] != i:
                    later = np.count_nonzero((Dn[i] == Dn[i, far[i]]) & (np.arange(n) > far[i]) & (np.arange(n) != i))
                    assert got[i, t] == n - 1 - later


def test_longest_list_through_the_c_entry(dev):
    """k = 301 at n = 302: 13 chunks, the last of 13 entries; lists of a row hold every other column once, shuffled"""
    n, k, d = 302, 301, 3
    rng = np.random.default_rng(301)
    X = (rng.integers(-20, 21, size=(n, d)) / 64.0).astype(np.float32)
    idx = np.stack([rng.permutation(np.delete(np.arange(n), i)) for i in range(n)])
    rc, rank, pen = c_ranks(dev, X, idx)
    ref = quality.ranks_numpy(X, idx)
    print("k = 301: rc %d, %d ranks differ" % (rc, np.count_nonzero(rank != ref)))
    assert rc == 0 and np.array_equal(rank, ref)
    assert np.array_equal(np.sort(rank, axis=1), np.tile(np.arange(1, n), (n, 1)))        # every rank once: a permutation
    assert np.array_equal(pen, np.maximum(rank.astype(np.int64) - k, 0).sum(axis=1)) and np.all(pen == 0)


def test_penalties_are_the_row_sums_and_outputs_do_not_depend_on_each_other(dev):
    n, d, k = 257, 5, 2 * KC + 1
    X, idx, _, _ = tie_case(n, d, k, 99)
    rc, rank, pen = c_ranks(dev, X, idx)
    rc1, rank1, none1 = c_ranks(dev, X, idx, want_pen=False)
    rc2, none2, pen2 = c_ranks(dev, X, idx, want_rank=False)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and none1 is None and none2 is None
    assert np.array_equal(rank, quality.ranks_numpy(X, idx))
    assert np.array_equal(pen, quality.penalties(rank, k)) and pen.max() > 0
    assert rank1.tobytes() == rank.tobytes() and pen2.tobytes() == pen.tobytes()


def unquantised_case():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(2000, 50)).astype(np.float32)
    return X, (X[:, :2] + 0.5 * rng.normal(size=(2000, 2))).astype(np.float32)


def test_unquantised_data(dev):
    X, Y = unquantised_case()
    n, d, k = 2000, 50, 30
    idx = quality.knn_numpy(Y, k)
    D = d2_rows(X.astype(np.float64), 0, n)
    thr = np.take_along_axis(D, idx, axis=1)
    amb = np.zeros(idx.shape, bool)
    for t in range(k):
        close = np.abs(D - thr[:, t, None]) <= d * 2.0 ** -50 * thr[:, t, None]
        close[np.arange(n), idx[:, t]] = False
        close[np.arange(n), np.arange(n)] = False
        amb[:, t] = close.any(axis=1)
    assert amb.sum() == 0                       # the seed was chosen so: the ambiguous set is empty (the bound is 0.1 %)
    t = quality.trustworthiness(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), k, details=True)
    ref = quality.trustworthiness(X, Y, k, backend="numpy", details=True)
    print("unquantised: neighbours differ at %d, ranks at %d of %d, T %.15f against %.15f" % (
        np.count_nonzero(t.neighbors != ref.neighbors), np.count_nonzero(t.ranks != ref.ranks), ref.ranks.size, t.score, ref.score))
    assert np.array_equal(t.neighbors, idx) and np.array_equal(ref.neighbors, idx)
    assert np.array_equal(t.ranks[~amb], ref.ranks[~amb])
    assert t.score == ref.score and np.array_equal(t.point, ref.point)


def test_repeatable_across_calls_and_streams_and_sampling(dev):
    X, Y = unquantised_case()
    X, Y = X[:700], Y[:700]
    xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    a = quality.embedding_quality(xd, yd, 12)
    b = quality.embedding_quality(xd, yd, 12)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        c = quality.embedding_quality(xd, yd, 12)
    side.synchronize()
    for o in (b, c):
        assert o.trustworthiness == a.trustworthiness and o.continuity == a.continuity and o.k_best == a.k_best
        for f in ("trust_point", "cont_point", "qnx", "lcmc"):
            assert getattr(o, f).tobytes() == getattr(a, f).tobytes()
    s = quality.embedding_quality(xd, yd, 12, sample_size=300, random_state=5)
    assert np.array_equal(s.sample_indices, quality.draw_sample(700, 300, 5)) and s.trust_point.shape == (700,)
    g = quality.embedding_quality(X[s.sample_indices], Y[s.sample_indices], 12)
    assert s.trustworthiness == g.trustworthiness and s.continuity == g.continuity
    assert np.array_equal(s.trust_point[s.sample_indices], g.trust_point) and np.array_equal(s.cont_point[s.sample_indices], g.cont_point)
    out = np.setdiff1d(np.arange(700), s.sample_indices)
    assert np.all(np.isnan(s.trust_point[out])) and np.all(np.isnan(s.cont_point[out]))
    assert np.array_equal(s.qnx, g.qnx)


def test_c_entry_rejects_the_domain_violations(dev):
    lib = api.load_library()
    x = torch.zeros((8, 4), dtype=torch.float32, device=dev)
    ix = torch.zeros((8, 302), dtype=torch.int32, device=dev)
    rank = torch.full((8, 302), -7, dtype=torch.int32, device=dev)
    pen = torch.full((8,), -7, dtype=torch.int64, device=dev)
    bad = [lib.ra_embed_ranks(P(x), 1, 4, P(ix), 2, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 262145, 4, P(ix), 2, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 8, 0, P(ix), 2, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 8, 2049, P(ix), 2, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 8, 4, P(ix), 0, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 8, 4, P(ix), 302, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(None, 8, 4, P(ix), 2, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 8, 4, None, 2, P(rank), P(pen), stream()),
           lib.ra_embed_ranks(P(x), 8, 4, P(ix), 2, None, None, stream())]
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in bad), bad                          # RA_ERR_ARG
    assert bool((rank == -7).all()) and bool((pen == -7).all())
    assert lib.ra_embed_ranks(P(x), 8, 4, P(ix), 2, P(rank), P(pen), stream()) == 0
    torch.cuda.synchronize()
    assert bool((rank[:1, :2] == 0).all()) and bool((pen == 0).all())         # row 0 lists itself: invalid; all points equal


def blobs():
    """600 points in three separated, equidistant Gaussian blobs in d = 10, Y = X[:, :2] with 30 points moved into another blob"""
    rng = np.random.default_rng(600)
    centres = np.zeros((3, 10))
    centres[:, :2] = 40.0 * np.array([[1.0, 0.0], [-0.5, 0.75 ** 0.5], [-0.5, -0.75 ** 0.5]])
    lab = np.repeat(np.arange(3), 200)
    X = (centres[lab] + rng.normal(size=(600, 10))).astype(np.float32)
    Y = X[:, :2].copy()
    moved = np.sort(rng.permutation(600)[:30])
    Y[moved] = (centres[(lab[moved] + 1) % 3, :2] + rng.normal(size=(30, 2))).astype(np.float32)
    return X, Y, moved


def test_recovery_of_misplaced_points(dev):
    X, Y, moved = blobs()
    r = quality.embedding_quality(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), 10)
    worst = np.sort(np.argsort(r.trust_point, kind="stable")[:30])
    print("recovery: T %.6f, C %.6f, the 30 lowest trust_point hold %d of the 30 moved rows" % (
        r.trustworthiness, r.continuity, np.intersect1d(worst, moved).size))
    assert np.array_equal(worst, moved)
    assert r.trust_point[moved].max() < np.delete(r.trust_point, moved).min()


def test_tools_end_to_end(dev, tmp_path, capsys):
    X, Y, moved = blobs()
    X, Y = X[:400], Y[:400]
    np.save(tmp_path / "x.npy", X)
    np.save(tmp_path / "y.npy", Y)
    assert quality.main([str(tmp_path / "x.npy"), str(tmp_path / "y.npy"), str(tmp_path / "q.npz"), "--k", "8", "--worst", "3"]) == 0
    text = capsys.readouterr().out
    o = np.load(tmp_path / "q.npz")
    ref = quality.embedding_quality(X, Y, 8, backend="numpy")
    assert float(o["trustworthiness"]) == ref.trustworthiness and float(o["continuity"]) == ref.continuity
    assert np.array_equal(o["trust_point"], ref.trust_point) and np.array_equal(o["qnx"], ref.qnx) and int(o["k_best"]) == ref.k_best
    assert int(o["k"]) == 8 and np.array_equal(o["sample_indices"], np.arange(400))
    assert "trustworthiness" in text and text.count("row ") == 3
    plain = ["embedding", "kl_divergence", "n_iter", "errors", "perplexity", "early_exaggeration", "learning_rate", "max_iter", "init",
             "seed", "backend"]
    common = [str(tmp_path / "x.npy"), "--max_iter", "250", "--perplexity", "20"]
    assert tsne.main(common[:1] + [str(tmp_path / "t0.npz")] + common[1:]) == 0
    assert tsne.main(common[:1] + [str(tmp_path / "t1.npz")] + common[1:] + ["--quality"]) == 0
    assert tsne.main(common[:1] + [str(tmp_path / "t2.npz")] + common[1:] + ["--quality", "6", "--fit_size", "300", "--seed", "1"]) == 0
    t0, t1, t2 = (np.load(tmp_path / ("t%d.npz" % i)) for i in range(3))
    assert sorted(t0.files) == sorted(plain)
    assert sorted(t1.files) == sorted(plain + ["trustworthiness", "continuity", "trust_point", "cont_point"])
    assert np.array_equal(t0["embedding"], t1["embedding"])
    q = quality.embedding_quality(X, t1["embedding"], 10)
    assert float(t1["trustworthiness"]) == q.trustworthiness and np.array_equal(t1["cont_point"], q.cont_point)
    assert 0.5 < float(t1["trustworthiness"]) <= 1.0
    assert {"trustworthiness", "continuity", "trust_point", "cont_point", "fit_indices"} <= set(t2.files)
    assert t2["trust_point"].shape == (400,) and float(t2["trustworthiness"]) == quality.trustworthiness(X, t2["embedding"], 6)
