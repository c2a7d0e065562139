"""Gaussian mixtures on the device: every case of tests/golden/gmm_ref.npz against scikit-learn 1.7's values (the stored bars) and
the numpy backend; single E- and M-steps through ctypes against float64 numpy at the shapes where the MFMA tiling and the
fixed-order sums can go wrong, with exact ties and the integer-exact lane-map check; bitwise reproducibility; the domain errors;
aligned stack -> 2SDR -> gmm -> class averages -> one multi-reference pass; and one case k-means cannot separate."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, gmm, kmeans  # noqa: E402
from test_gmm_cpu import CASES, GOLDEN, case, check_against_pins, fit  # noqa: E402

U = 2.0 ** -53
FULL_D, FULL_N = (1, 3, 16, 17, 33, 128, 256), (17, 1000, 4097)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a, dev, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


@pytest.mark.parametrize("c", CASES)
def test_device_matches_sklearn_pins_and_numpy(dev, z, c):
    X, k, kw = case(z, c)
    r = fit(torch.from_numpy(X).to(dev), k, kw, "device", not bool(z[c + "_converged"]))
    check_against_pins(z, c, r, torch.from_numpy(X).to(dev), "device")
    rn = fit(X, k, kw, "numpy", not bool(z[c + "_converged"]))
    assert np.array_equal(r.labels, rn.labels) and r.n_iter == rn.n_iter and r.converged == rn.converged
    assert np.abs(r.means - rn.means).max() <= 2 * float(z[c + "_tol_means"])          # each within the bar of the same pin


# ---- single steps

def mixture(n, d, k, cov, seed, spread=2.0):
    """X float32 [n][d] around k centres, and a plausible model: means, PC, offset (float64)"""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((k, d)) * spread
    X = (means[rng.integers(0, k, n)] + rng.standard_normal((n, d))).astype(np.float32)
    if cov == "full":
        A = rng.standard_normal((k, d, 2 * d))
        C = A @ np.transpose(A, (0, 2, 1)) / (2 * d) + 0.25 * np.eye(d)
    else:
        C = rng.uniform(0.3, 3.0, (k, d))
    pc = gmm.precision_cholesky(C, cov)
    w = rng.uniform(0.5, 1.5, k)
    return X, means, pc, gmm.offsets(w / w.sum(), pc, cov)


def estep_numpy(X, means, pc, off, cov):
    """(log p [n][k], log_prob_norm [n], the bound per entry [n][k]) in float64"""
    X = X.astype(np.float64)
    n, d = X.shape
    k = means.shape[0]
    lp, bound = np.empty((n, k)), np.empty((n, k))
    for c in range(k):
        diff = X - means[c]
        if cov == "full":
            y = diff @ pc[c]
            A = np.sum(((np.abs(X) + np.abs(means[c])) @ np.abs(pc[c])) ** 2, axis=1)
        else:
            y = diff * pc[c]
            A = np.sum(((np.abs(X) + np.abs(means[c])) * np.abs(pc[c])) ** 2, axis=1)
        lp[:, c] = off[c] - 0.5 * np.sum(y * y, axis=1)
        bound[:, c] = 4 * (d + 4) * U * A + 8 * U * np.maximum(1.0, np.abs(lp[:, c]))
    mx = lp.max(axis=1)
    return lp, mx + np.log(np.sum(np.exp(lp - mx[:, None]), axis=1)), bound


def estep_device(dev, X, means, pc, off, cov, want_resp=True, want_labels=True):
    L = api.load_library()
    n, d = X.shape
    k = means.shape[0]
    x = torch.from_numpy(X).to(dev)
    lr = torch.full((n, k), 7.0, dtype=torch.float64, device=dev) if want_resp else None
    lpn = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    lab = torch.full((n,), -7, dtype=torch.int32, device=dev) if want_labels else None
    s = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    mu_d, pc_d, off_d = up(means, dev), up(pc, dev), up(off, dev)          # named: they must outlive the call
    rc = L.ra_gmm_estep(P(x), n, d, k, gmm.COV_TYPES[cov], P(mu_d), P(pc_d), P(off_d), P(lr), P(lpn), P(lab), P(s), stream())
    assert rc == 0, L.ra_last_error()
    torch.cuda.synchronize()
    return (lr.cpu().numpy() if want_resp else None, lpn.cpu().numpy(), lab.cpu().numpy() if want_labels else None, float(s.item()))


def check_estep(dev, X, means, pc, off, cov, tag):
    lp, lpn, bound = estep_numpy(X, means, pc, off, cov)
    lr, got_lpn, lab, total = estep_device(dev, X, means, pc, off, cov)
    # the entry returns log_resp = log p - log_prob_norm, not log p: adding log_prob_norm back costs the two roundings of the
    # subtraction and the addition, at most 2^-53 (|log_resp| + |log p|) <= 2 * 2^-53 (|log p| + |log_prob_norm|), on top of the bound
    e_lp = np.abs((lr + got_lpn[:, None]) - lp)
    slack = 2 * U * (np.abs(lp) + np.abs(lpn)[:, None])
    e_n = np.abs(got_lpn - lpn)
    b_n = bound.max(axis=1)
    print("estep %s: max |d log p| / bound %.3f, max |d log_prob_norm| / bound %.3f" % (tag, (e_lp / (bound + slack)).max(),
                                                                                      (e_n / b_n).max()))
    assert np.all(e_n <= b_n), (tag, float((e_n / b_n).max()))
    assert np.all(e_lp <= bound + slack), (tag, float((e_lp / (bound + slack)).max()))
    srt = np.sort(lp, axis=1)
    clear = np.ones(len(lp), bool) if lp.shape[1] == 1 else (srt[:, -1] - srt[:, -2]) > 2 * b_n
    assert np.array_equal(lab[clear], np.argmax(lp, axis=1)[clear].astype(np.int32)), tag
    # d_sum: runs of 64 values in order, then at most n / 16384 + 1 runs per thread and 256 thread shares in order
    assert abs(total - float(np.sum(got_lpn))) <= (64 + 256 + len(lpn) / 16384 + 4) * U * np.sum(np.abs(got_lpn))
    # the optional outputs change nothing
    _, lpn2, _, total2 = estep_device(dev, X, means, pc, off, cov, want_resp=False, want_labels=False)
    assert np.array_equal(lpn2, got_lpn) and total2 == total


@pytest.mark.parametrize("d", FULL_D)
def test_full_estep_against_float64_numpy(dev, d):
    for n in FULL_N:
        check_estep(dev, *mixture(n, d, 3, "full", 100 * d + n % 7), "full", "full n=%d d=%d k=3" % (n, d))


@pytest.mark.parametrize("k", [1, 2, 256])
def test_full_estep_component_counts(dev, k):
    check_estep(dev, *mixture(600, 17, k, "full", k), "full", "full n=600 d=17 k=%d" % k)


@pytest.mark.parametrize("d", [1, 50, 2048])
def test_diag_estep_against_float64_numpy(dev, d):
    for n, k in ((17, 3), (1000, 33), (4097, 2)):
        check_estep(dev, *mixture(n, d, k, "diag", d + n), "diag", "diag n=%d d=%d k=%d" % (n, d, k))


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_estep_exact_ties_take_the_first_index(dev, cov):
    X, means, pc, off = mixture(500, 19, 4, cov, 3)
    means[3], pc[3], off[3] = means[1], pc[1], off[1]          # components 1 and 3 are the same
    means[2], pc[2], off[2] = means[0], pc[0], off[0]          # and so are 0 and 2
    lr, lpn, lab, _ = estep_device(dev, X, means, pc, off, cov)
    assert np.array_equal(lr[:, 1], lr[:, 3]) and np.array_equal(lr[:, 0], lr[:, 2])
    assert set(np.unique(lab)) == {0, 1}
    assert np.array_equal(lab, np.argmax(lr, axis=1).astype(np.int32))


@pytest.mark.parametrize("d", FULL_D)
def test_full_estep_is_exact_on_small_integers(dev, d):
    """integer-valued X, mu, PC and offset: every product and sum is exact in double, so with one component log_prob_norm is
    log p bit for bit -- a wrong MFMA lane map (the f32 C/D rows) cannot pass"""
    rng = np.random.default_rng(d)
    n = 100
    X = rng.integers(-4, 5, (n, d)).astype(np.float32)
    for seed in range(2):
        mu = rng.integers(-2, 3, (1, d)).astype(np.float64)
        pc = np.triu(rng.integers(-2, 3, (1, d, d))).astype(np.float64)
        off = np.array([float(3 - seed)])
        y = (X.astype(np.float64) - mu[0]) @ pc[0]
        want = off[0] - 0.5 * np.sum(y * y, axis=1)
        lr, lpn, lab, total = estep_device(dev, X, mu, pc, off, "full")
        assert np.array_equal(lpn, want) and np.all(lr == 0.0) and np.all(lab == 0) and total == float(np.sum(want))


def mstep_numpy(X, r, reg, cov):
    """(nk, means, covariances, and the sums of absolute values behind the means and the covariances).  Up to d = 64, where the
    bound 8 (d + 4) 2^-53 is of the size of float64 numpy's own error over n terms (np.sum down a column adds the n rows one after
    the other), the sums run in numpy's extended precision, so that the comparison measures the device and not the reference"""
    ft = np.longdouble if X.shape[1] <= 64 else np.float64
    X, r = X.astype(ft), r.astype(ft)
    n, d = X.shape
    k = r.shape[1]
    nk = r.sum(axis=0) + 10 * np.finfo(np.float64).eps
    means = r.T @ X / nk[:, None]
    a_means = r.T @ np.abs(X) / nk[:, None]
    f = lambda *a: tuple(np.asarray(v, np.float64) for v in a)          # noqa: E731
    if cov == "diag":
        return f(nk, means, r.T @ (X * X) / nk[:, None] - means ** 2 + reg, a_means, r.T @ (X * X) / nk[:, None] + means ** 2 + reg)
    C, A = np.empty((k, d, d), ft), np.empty((k, d, d), ft)
    for c in range(k):
        diff = X - means[c]
        C[c] = (r[:, c] * diff.T) @ diff / nk[c]
        C[c].flat[::d + 1] += reg
        A[c] = (r[:, c] * np.abs(diff).T) @ np.abs(diff) / nk[c] + reg
    return f(nk, means, C, a_means, A)


def mstep_device(dev, X, resp, log_domain, reg, cov):
    L = api.load_library()
    n, d = X.shape
    k = resp.shape[1]
    nk = torch.empty(k, dtype=torch.float64, device=dev)
    means = torch.empty((k, d), dtype=torch.float64, device=dev)
    C = torch.empty((k, d, d) if cov == "full" else (k, d), dtype=torch.float64, device=dev)
    x, r = torch.from_numpy(X).to(dev), up(resp, dev)                      # named: they must outlive the call
    rc = L.ra_gmm_mstep(P(x), n, d, k, gmm.COV_TYPES[cov], P(r), int(log_domain), float(reg), P(nk), P(means), P(C), stream())
    assert rc == 0, L.ra_last_error()
    torch.cuda.synchronize()
    return nk.cpu().numpy(), means.cpu().numpy(), C.cpu().numpy()


def check_mstep(dev, n, d, k, cov, seed):
    X, means, pc, off = mixture(n, d, k, cov, seed)
    logit = np.random.default_rng(seed).standard_normal((n, k)) * 2.0
    log_r = logit - np.log(np.sum(np.exp(logit), axis=1))[:, None]
    reg = 1e-6
    nk, mu, C, a_mu, a_C = mstep_numpy(X, np.exp(log_r), reg, cov)
    g_nk, g_mu, g_C = mstep_device(dev, X, log_r, 1, reg, cov)
    b = 8 * (d + 4) * U
    e = (np.abs(g_nk - nk) / nk).max() / b, (np.abs(g_mu - mu) / a_mu).max() / b, (np.abs(g_C - C) / a_C).max() / b
    print("mstep %s n=%d d=%d k=%d: errors / bound: nk %.3f means %.3f covariances %.3f" % (cov, n, d, k, e[0], e[1], e[2]))
    assert max(e) <= 1.0, e
    if cov == "full":
        assert np.array_equal(g_C, np.transpose(g_C, (0, 2, 1)))
    lab = np.random.default_rng(seed + 1).integers(0, k, n)
    lab[:k] = np.arange(k)
    hot = np.zeros((n, k))
    hot[np.arange(n), lab] = 1.0
    with np.errstate(divide="ignore"):
        a, b2 = mstep_device(dev, X, hot, 0, reg, cov), mstep_device(dev, X, np.log(hot), 1, reg, cov)
    for u, v in zip(a, b2):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("d", FULL_D)
def test_full_mstep_against_float64_numpy(dev, d):
    for n in FULL_N:
        check_mstep(dev, n, d, 3, "full", 7 * d + n % 5)


@pytest.mark.parametrize("k", [1, 2, 256])
def test_full_mstep_component_counts(dev, k):
    check_mstep(dev, 600, 17, k, "full", k)


@pytest.mark.parametrize("d", [1, 50, 2048])
def test_diag_mstep_against_float64_numpy(dev, d):
    for n, k in ((17, 3), (1000, 33), (4097, 2)):
        check_mstep(dev, n, d, k, "diag", d + n)


# ---- whole fits

def test_bitwise_reproducible_across_calls_and_streams(dev):
    rng = np.random.default_rng(8)
    X = torch.from_numpy((rng.normal(size=(20000, 16)) * rng.uniform(0.5, 2.0, 16) + rng.integers(0, 5, 20000)[:, None] * 3.0)
                         .astype(np.float32)).to(dev)
    for cov in ("full", "diag"):
        a = gmm.gmm(X, 5, covariance_type=cov, random_state=4, max_iter=20)
        b = gmm.gmm(X, 5, covariance_type=cov, random_state=4, max_iter=20)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            c = gmm.gmm(X, 5, covariance_type=cov, random_state=4, max_iter=20)
        s.synchronize()
        for r in (b, c):
            assert np.array_equal(a.labels, r.labels) and np.array_equal(a.means, r.means) and np.array_equal(a.covariances, r.covariances)
            assert np.array_equal(a.lower_bounds, r.lower_bounds) and a.n_iter == r.n_iter and np.array_equal(a.log_prob, r.log_prob)


def test_domain_errors_return_codes(dev):
    L = api.load_library()
    f64 = dict(dtype=torch.float64, device=dev)
    x = torch.zeros((300, 4), device=dev)
    mu, pc, off = torch.zeros((2, 4), **f64), torch.zeros((2, 4, 4), **f64), torch.zeros(2, **f64)
    lr, lpn, s = torch.full((300, 2), 7.0, **f64), torch.full((300,), 7.0, **f64), torch.full((1,), 7.0, **f64)
    lab = torch.full((300,), 7, dtype=torch.int32, device=dev)
    nk, mo, co = torch.full((2,), 7.0, **f64), torch.full((2, 4), 7.0, **f64), torch.full((2, 4, 4), 7.0, **f64)
    st = stream()

    def E(n=300, d=4, k=2, ct=0, x=x, mu=mu, pc=pc, off=off, lpn=lpn, s=s):
        return L.ra_gmm_estep(P(x), n, d, k, ct, P(mu), P(pc), P(off), P(lr), P(lpn), P(lab), P(s), st)

    def M(n=300, d=4, k=2, ct=0, x=x, r=lr, reg=1e-6, nk=nk, mo=mo, co=co):
        return L.ra_gmm_mstep(P(x), n, d, k, ct, P(r), 0, reg, P(nk), P(mo), P(co), st)

    bad = [E(d=257), E(d=2049, ct=1), E(k=257), E(k=0), E(n=1), E(n=0), E(n=4194305), E(n=1 << 21, k=256), E(d=0), E(ct=2), E(x=None),
           E(mu=None), E(pc=None), E(off=None), E(lpn=None), E(s=None),
           M(d=257), M(d=2049, ct=1), M(k=257), M(k=0), M(n=1), M(n=0), M(ct=-1), M(reg=-1.0), M(reg=float("nan")), M(x=None), M(r=None),
           M(nk=None), M(mo=None), M(co=None)]
    assert all(rc == -1 for rc in bad), bad
    torch.cuda.synchronize()
    for t in (lr, lpn, s, nk, mo, co):
        assert torch.all(t == 7.0)
    assert torch.all(lab == 7)
    with pytest.raises(gmm.GmmError):
        gmm.gmm(torch.zeros((40, 3), device=dev, dtype=torch.float64), 2)
    with pytest.raises(gmm.GmmError):
        gmm.gmm(torch.zeros((3, 40), device=dev).t(), 2)
    with pytest.raises(gmm.GmmError):
        gmm.gmm(torch.zeros((300, 257), device=dev), 2)
    bx = torch.zeros((40, 3), device=dev)
    bx[5, 1] = float("nan")
    with pytest.raises(gmm.GmmError):
        gmm.gmm(bx, 2)
    X = torch.from_numpy(np.repeat(np.array([[0.0, 0.0], [4.0, 4.0]], np.float32), 10, axis=0)).to(dev)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        gmm.gmm(X, 2, reg_covar=0.0, init_params=np.repeat(np.array([0, 1]), 10))


def test_references_from_an_aligned_stack(dev, tmp_path):
    """aligned stack -> 2SDR -> gmm -> class averages -> one multi-reference pass, and the tool on the same factors"""
    from cryo_ralib_amd import mref, sdr
    from test_gpu_kmeans import aligned_stack
    nx, ou, nref, n = 32, 12, 3, 240
    refs, parts, cls, inv = aligned_stack(nref, n, nx, ou, 0.3)
    with torch.cuda.device(dev):
        al = api.rot_shift2d(torch.from_numpy(parts).to(dev), inv)
        F = np.ascontiguousarray(sdr.two_sdr(al, 8, 8, 10).factors, np.float32)
    r = gmm.gmm(torch.from_numpy(F).to(dev), 3, random_state=0)
    assert kmeans.purity_score(cls, r.labels) >= 0.95 and kmeans.c_purity_score(cls, r.labels) >= 0.95
    proba = gmm.predict_proba(torch.from_numpy(F).to(dev), r)
    assert proba.shape == (n, 3) and np.allclose(proba.sum(axis=1), 1.0, atol=1e-12) and np.array_equal(proba.max(axis=1), r.proba_max)
    avg = kmeans.class_averages(parts, inv, r.labels, 3, ou)
    assert avg.shape == (3, nx, nx) and np.all(np.isfinite(avg))
    a = mref.MrefAligner(parts, avg, ou, 2, 2)
    a.iterate()
    got = a.params()["ref_id"]
    a.close()
    assert kmeans.purity_score(cls, got) >= 0.95
    np.save(tmp_path / "f.npy", F)
    assert gmm.main([str(tmp_path / "f.npy"), str(tmp_path / "o.npz"), "--sweep", "2:4", "--seed", "0", "--min_proba", "0.8"]) == 0
    o = np.load(tmp_path / "o.npz")
    assert str(o["backend"]) == "device" and o["sweep"].shape == (3, 6) and o["keep"].shape == (n,)


def stretched_case():
    """two large classes, one of them stretched along factor 0, and a class 20 times smaller"""
    rng = np.random.default_rng(0)
    d, n_big, n_small = 4, 1000, 50
    A = rng.standard_normal((n_big, d)) * np.array([6.0, 0.5, 0.5, 0.5])
    B = rng.standard_normal((n_big, d)) * 0.7 + np.array([0, 3.0, 0, 0])
    C = rng.standard_normal((n_small, d)) * 0.5 + np.array([0, -3.0, 2.0, 0])
    X, y = np.concatenate([A, B, C]), np.repeat([0, 1, 2], [n_big, n_big, n_small])
    p = rng.permutation(len(X))
    return (np.round(X[p] * 64) / 64).astype(np.float32), y[p]


def test_mixture_separates_what_kmeans_splits(dev):
    """with the numpy backends and random_state=0 k-means reaches purity 0.8010 (it cuts the stretched class in two and swallows
    the small one), the full-covariance mixture 0.9546"""
    X, y = stretched_case()
    Xd = torch.from_numpy(X).to(dev)
    pk = kmeans.purity_score(y, kmeans.kmeans(Xd, 3, random_state=0).labels)
    r = gmm.gmm(Xd, 3, random_state=0)
    pg = kmeans.purity_score(y, r.labels)
    print("purity: k-means %.4f, mixture %.4f" % (pk, pg))
    assert pg > pk and pg >= 0.94
    rn = gmm.gmm(X, 3, random_state=0, backend="numpy")
    assert np.array_equal(r.labels, rn.labels) and r.n_iter == rn.n_iter
