"""The 2SDR kernels (csrc/ralign_sdr.h) entry by entry at their tile, run and rank edges, on the inputs of
tests/test_sdr_edges_cpu.py (whose properties that file asserts without a GPU).  Integer-valued images, means and projectors make
every f32 product and partial sum an exact integer below 2^24, so means, Grams, U and F are compared for equality with the numpy
result; the real-valued cases use the entry-wise bounds that file derives from term counts, and print their largest
error / bound ratio.  Every output is the interior of a larger buffer filled with a sentinel: every entry inside must have
been overwritten and every guard element on both sides must be untouched.

Edge                                                          integer case
------------------------------------------------------------  --------------------------------------------------------------
mean: runs of 64 (n = 63, 64, 65)                             test_mean_exact[63|64|65-*]
mean: 16 / 17 partials against the 16 shares (C 1 -> 2)       test_mean_exact[1024|1025-*]
mean: npix 1, 63 .. 65, 255 .. 257 (blocks of 64 / 256), p=1  test_mean_exact[65|1025-p-q] over MEAN_PQ
form 0: ns steps d = 1, 15 .. 17, 112, 113, 128               test_gram0_tiles[7-p-d]
form 0: nb 1 -> 2 at d = 129 (TD = 80, 49 of 80 columns),     test_gram0_tiles[7-5-129], [7-3-130], [7-5-160], [7-3-161],
        130, 160, 161, 255, 256                               [7-5-255], [7-3-256]
form 0: 16-row steps across image boundaries, last step of    test_gram0_tiles (21 or 35 stack rows, p = 3 or 5);
        a run partly filled (p = 33: 2046 rows, 14 left)      test_gram0_runs[61|62|63-33-17]
form 0: p = 256, runs of 8 images: 1, 2, 16, 17, 17, 18 runs  test_gram0_runs[8|9|128|129|136|137-256-17]
second stage: q = 1, 127 .. 129, 2047, 2048 (136 tiles)       test_second_stage_gram[*-1-q]
second stage: run of 2048 rows (n = 1, 2047, 2048, 2049)      test_second_stage_gram[n-1-129], [n-1-2048]
second stage: 17 runs                                         test_second_stage_gram[32769-1-5]
forms 1, 2: (k + 3) & ~3 and kt, k = 1 .. 64                  test_gram12_ranks[form-k-L-d] over GRAM12_KLD
forms 1, 2: contracted length k, 17, 33, 47, 90, 255, 256     test_gram12_ranks[form-k-L-d]
forms 1, 2: d = 16, 17, 128, 129, 256                         test_gram12_ranks[form-k-L-d]
forms 1, 2: 1, 2, 16, 17, 18, 33 runs of 32 images            test_gram12_runs[form-n]; null mean at n = 33, 545
forms 1, 2: d differs between the forms                       test_gram12_rectangular[form-33-130], [form-130-33]
project: wave exit at wave * 16 >= p0, partly filled last     test_project_exact[n-p-q-p0-q0] over project_cases()
        16-tile in a and in b, the a q0 + b layout            (every (p0, q0) of the grid, the named pairs)
project: image i's row independent of the others              test_project_exact with n = 3: batch == single-image calls
factors: row blocks n = 1, 15 .. 17, 63 .. 65, 129            test_factors_exact[n-625-17], [n-2048-65]
factors: contracted length m = 1, 3, 4, 5, 625, 2047, 2048    test_factors_exact[17|65-m-*]
factors: column blocks r = 1, 15 .. 17, 63 .. 65, 255, 256    test_factors_exact[17-625-r], [129-2048-r]
the accepted corner p0 q0 = 2048, r = 256                     test_accepted_corner_end_to_end (real-valued)
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, sdr  # noqa: E402
from test_sdr_edges_cpu import (GRAM0_RUNS, GRAM0_TILE, GRAM12_KLD, GRAM12_NULL_MEAN_N, GRAM12_RECT, GRAM12_RUN_N,  # noqa: E402
                                STAGE2, centred, chained_factors_bound, factors_bound, factors_case, factors_cases,
                                factors_ref, gram_case, int_stack, mean_cases, mean_ref, project_bound, project_case,
                                project_cases, project_ref, real_factors_case, real_gram_case, real_mean_case,
                                real_project_case)

GUARD = 1024                 # sentinel elements before and after every output
SENTINEL = -7.5e30           # no integer case and no bounded real value comes near it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) if a is not None else None


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """an output of the given shape inside a sentinel-filled buffer"""

    def __init__(self, dev, shape, dtype=torch.float32):
        self.shape, self.size = shape, int(np.prod(shape))
        self.buf = torch.full((self.size + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def result(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        fill = b.dtype.type(SENTINEL)
        assert np.all(b[:GUARD] == fill), "written before the output: %s" % (np.nonzero(b[:GUARD] != fill)[0][:10] - GUARD)
        assert np.all(b[GUARD + self.size:] == fill), "written past the output: +%s" % np.nonzero(b[GUARD + self.size:] != fill)[0][:10]
        inner = b[GUARD:GUARD + self.size].reshape(self.shape)
        assert not np.any(inner == fill), "never written: %s" % np.argwhere(inner == fill)[:10]
        return inner


def check(rc):
    assert rc == 0, api.load_library().ra_last_error()


def mean_dev(dev, x, n, p, q):
    out = Guarded(dev, (p, q))
    check(api.load_library().ra_sdr_mean(P(x), n, p, q, out.ptr, stream()))
    return out.result()


def gram_dev(dev, x, n, p, q, mean, form, Pm=None):
    d = p if form == 1 else q
    out = Guarded(dev, (d, d), torch.float64)
    md, Pd = on(dev, mean), on(dev, Pm)
    check(api.load_library().ra_sdr_gram(P(x), n, p, q, P(md), form, P(Pd), 0 if Pm is None else Pm.shape[1], out.ptr, stream()))
    return out.result()


def project_dev(dev, x, n, p, q, mean, A, B):
    out = Guarded(dev, (n, A.shape[1] * B.shape[1]))
    md, Ad, Bd = on(dev, mean), on(dev, A), on(dev, B)
    check(api.load_library().ra_sdr_project(P(x), n, p, q, P(md), P(Ad), A.shape[1], P(Bd), B.shape[1], out.ptr, stream()))
    return out.result()


def factors_dev(dev, U, G):
    out = Guarded(dev, (U.shape[0], G.shape[1]))
    Ud, Gd = on(dev, U), on(dev, G)
    check(api.load_library().ra_sdr_factors(P(Ud), U.shape[0], U.shape[1], P(Gd), G.shape[1], out.ptr, stream()))
    return out.result()


def assert_equal(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got, want), "first differing indices %s" % np.argwhere(got != want)[:10].tolist()


def check_gram_exact(dev, n, p, q, form, k=0, null=False):
    X, mean, Pm, ref = gram_case(n, p, q, form, k, null)
    g = gram_dev(dev, on(dev, X), n, p, q, mean, form, Pm)
    assert_equal(g, ref)
    assert np.array_equal(g, g.T)


def within(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    print("RATIO %s %.4f (max error %.3e)" % (name, float(np.max(err / bound)), float(err.max())))
    assert np.all(err <= bound), "first entries outside the bound %s" % np.argwhere(err > bound)[:10].tolist()


# ---- 1. mean

@pytest.mark.parametrize("n,p,q", mean_cases())
def test_mean_exact(dev, n, p, q):
    X = int_stack(n, p, q, 7)
    got = mean_dev(dev, on(dev, X), n, p, q)
    assert_equal(got, mean_ref(X))


# ---- 2. Gram, form 0

@pytest.mark.parametrize("n,p,q", GRAM0_TILE)
def test_gram0_tiles(dev, n, p, q):
    check_gram_exact(dev, n, p, q, 0)


@pytest.mark.parametrize("n,p,q", GRAM0_RUNS)
def test_gram0_runs(dev, n, p, q):
    check_gram_exact(dev, n, p, q, 0)


@pytest.mark.parametrize("n,p,q", STAGE2)
def test_second_stage_gram(dev, n, p, q):
    check_gram_exact(dev, n, p, q, 0, 0, True)


# ---- 3. Gram, forms 1 and 2

@pytest.mark.parametrize("k,L,d", GRAM12_KLD)
@pytest.mark.parametrize("form", [1, 2])
def test_gram12_ranks(dev, form, k, L, d):
    p, q = (d, L) if form == 1 else (L, d)
    check_gram_exact(dev, 3, p, q, form, k)


@pytest.mark.parametrize("n", GRAM12_RUN_N)
@pytest.mark.parametrize("form", [1, 2])
def test_gram12_runs(dev, form, n):
    check_gram_exact(dev, n, 20, 24, form, 5, n in GRAM12_NULL_MEAN_N)


@pytest.mark.parametrize("p,q", GRAM12_RECT)
@pytest.mark.parametrize("form", [1, 2])
def test_gram12_rectangular(dev, form, p, q):
    check_gram_exact(dev, 3, p, q, form, 5)


# ---- 4. project

@pytest.mark.parametrize("n,p,q,p0,q0", project_cases())
def test_project_exact(dev, n, p, q, p0, q0):
    X, mean, A, B, ref = project_case(n, p, q, p0, q0)
    x = on(dev, X)
    U = project_dev(dev, x, n, p, q, mean, A, B)
    assert_equal(U, ref)
    U3, R3 = U.reshape(n, p0, q0), ref.reshape(n, p0, q0)
    assert np.array_equal(U3[:, p0 - 1, :], R3[:, p0 - 1, :]) and np.array_equal(U3[:, :, q0 - 1], R3[:, :, q0 - 1])
    for i in range(n if n > 1 else 0):
        assert_equal(project_dev(dev, x[i:i + 1].contiguous(), 1, p, q, mean, A, B)[0], U[i])


# ---- 5. factors

@pytest.mark.parametrize("n,m,r", factors_cases())
def test_factors_exact(dev, n, m, r):
    U, G, ref = factors_case(n, m, r)
    assert_equal(factors_dev(dev, U, G), ref)


# ---- 6. real-valued, against the derived bounds

def test_mean_real_within_bound(dev):
    X, ref, bound = real_mean_case()
    within("mean", mean_dev(dev, on(dev, X), *X.shape), ref, bound)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_gram_real_within_bound(dev, form):
    """form 3 is the second stage: form 0 with p = 1 and a null mean"""
    X, mean, Pm, ref, bound = real_gram_case(form)
    n, p, q = X.shape
    g = gram_dev(dev, on(dev, X), n, p, q, mean, form % 3, Pm)
    within("gram form %d" % form, g, ref, bound)
    assert np.array_equal(g, g.T)


def test_project_real_within_bound(dev):
    X, mean, A, B, ref, bound = real_project_case()
    n, p, q = X.shape
    within("project", project_dev(dev, on(dev, X), n, p, q, mean, A, B), ref, bound)


def test_factors_real_within_bound(dev):
    U, G, ref, bound = real_factors_case()
    within("factors", factors_dev(dev, U, G), ref, bound)


# ---- 7. the accepted corner, end to end

def test_accepted_corner_end_to_end(dev, monkeypatch):
    """n = 300, 64 x 64, p0 = 32, q0 = 64 (p0 q0 = 2048), r = 256: the corner check_domain admits.  No subspace is compared (the
    eigen-gaps of such data are not controlled): shapes, finiteness, the factors against the float64 recomputation from the
    returned A, B, G and mean, and the second-stage Gram against a direct call on the same U."""
    n, p, q, p0, q0, r = 300, 64, 64, 32, 64, 256
    rng = np.random.default_rng(300)
    a = (rng.standard_normal((n, p, q)) + 0.3 * rng.standard_normal((1, p, q)) + 1.0).astype(np.float32)
    x = torch.from_numpy(a).to(dev)
    seen = {"grams": []}
    top_eig, project = sdr.top_eig, sdr._Device.project

    def spy_eig(S, k):
        seen["grams"].append(np.array(S, copy=True))
        return top_eig(S, k)

    def spy_project(self, mean, A, B):
        seen["U"] = project(self, mean, A, B)
        return seen["U"]
    monkeypatch.setattr(sdr, "top_eig", spy_eig)
    monkeypatch.setattr(sdr._Device, "project", spy_project)
    res = sdr.two_sdr(x, p0, q0, r, max_iter=2, tol=-np.inf)
    assert res.iterations == 2 and len(seen["grams"]) == 5
    assert res.factors.shape == (n, r) and res.G.shape == (p0 * q0, r) and res.A.shape == (p, p0) and res.B.shape == (q, q0)
    assert res.mean.shape == (p, q) and res.factors.dtype == np.float32
    for M in (res.factors, res.G, res.A, res.B, res.mean):
        assert np.all(np.isfinite(M))
    A, B, G = (np.ascontiguousarray(M, np.float32) for M in (res.A, res.B, res.G))        # as _Device._f32 rounds them
    Xc = centred(a, res.mean)
    Ud = seen["U"].cpu().numpy()
    assert Ud.shape == (n, p0 * q0)
    within("corner project", Ud, project_ref(Xc, A, B), project_bound(Xc, A, B))
    within("corner factors from the device's U", res.factors, factors_ref(Ud, G), factors_bound(Ud, G))
    F = factors_ref(project_ref(Xc, A, B).astype(np.float32), G)
    within("corner factors recomputed", res.factors, F, chained_factors_bound(Xc, A, B, G))
    C = seen["grams"][-1]
    assert C.shape == (p0 * q0, p0 * q0)
    direct = gram_dev(dev, seen["U"], n, 1, p0 * q0, None, 0)
    assert np.array_equal(direct, C), np.argwhere(direct != C)[:10].tolist()
    assert np.array_equal(C, C.T)
