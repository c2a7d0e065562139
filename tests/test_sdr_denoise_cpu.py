"""2SDR denoising without a GPU: the numpy backend of sdr.transform / reconstruct / denoise / eigenimages against the reference's
pinned outputs (tests/golden/sdr_ref.npz), the identities of the model, denoising quality and junk detection on planted stacks,
the model file, the tool's usage errors -- and the input builders of tests/test_gpu_sdr_denoise.py with the checks of the
builders themselves.

Integer builders.  Factors are integers in -2 .. 2, G, A and B have entries in {-1, 0, 1}, the mean is an integer pattern in
-1 .. 1.  The entry-wise majorant |A| reshape(|G| |f|) |B|^T + |mean| bounds the absolute terms of every f32 accumulator of the
three chained products (c = G f, T = C B^T, x^ = A T) and of the mean's add; below 2^24 every partial is an exact integer in
any order, so the device must equal the float64 product bit for bit.

Real-valued bound (u = 2^-24; each product is an f32 fma chain, one rounding per term): c is a chain of r terms, T of q0, x^ of
p0, each carrying the error of the one before through non-negative majorants, + 8 for the second-order terms and the mean's add,
and the result is rounded once more:   (r + p0 + q0 + 8) u |A| reshape(|G| |f|) |B|^T + u |x^|   (r = 0 without G)."""
import functools
import os

import numpy as np
import pytest

from cryo_ralib_amd import api, sdr
from test_sdr_edges_cpu import LIMIT, U24, cut10, int_mean, int_proj, is_integer_f32, real_proj

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdr_ref.npz")
RUN = 8                      # SDR_REC_RUN: images per workgroup of ra_sdr_reconstruct
OLD_KEYS = {"factors", "G", "A", "B", "mean", "iterations", "energies", "p0", "q0", "r"}


# ---- builders (shared with the GPU file)

# (n, p, q, p0, q0, r, with G, with mean): n at 1 and RUN - 1, RUN, RUN + 1; p, q in 1, 15, 16, 17, 90, 255, 256; p0, q0 in
# 1, 16, 17, 49, 64; m = 2048 as 64 x 32 on 64 x 64; r in 1, 64, 65, 256; no G; no mean; several runs; p0, q0 in 33 .. 48 and
# p, q in 129 .. 192 for the kernel's register plans
INT_CASES = [(1, 1, 1, 1, 1, 1, True, True), (7, 15, 17, 1, 16, 1, True, True), (8, 16, 15, 1, 1, 1, True, True),
             (8, 17, 16, 17, 16, 64, True, False), (9, 16, 90, 16, 49, 65, True, True), (9, 90, 255, 49, 17, 256, True, True),
             (3, 255, 256, 64, 17, 65, True, True), (2, 256, 90, 17, 64, 64, True, True), (9, 64, 64, 64, 32, 256, True, True),
             (9, 64, 64, 64, 32, 2048, False, True), (7, 90, 90, 25, 25, 625, False, False), (17, 20, 24, 3, 4, 5, True, True),
             (9, 130, 47, 40, 33, 65, True, True), (2, 47, 192, 33, 5, 7, True, True)]


def rec_ref(F, G, A, B, mean, p0, q0):
    """mean + A reshape(G f) B^T in float64, (a, b) -> a q0 + b"""
    c = np.asarray(F, np.float64) if G is None else np.asarray(F, np.float64) @ np.asarray(G, np.float64).T
    xh = np.matmul(np.matmul(np.asarray(A, np.float64), c.reshape(-1, p0, q0)), np.asarray(B, np.float64).T)
    return xh if mean is None else xh + np.asarray(mean, np.float64)


def rec_majorant(F, G, A, B, mean, p0, q0):
    return rec_ref(np.abs(F), None if G is None else np.abs(G), np.abs(A), np.abs(B), None if mean is None else np.abs(mean), p0, q0)


def rec_bound(F, G, A, B, mean, p0, q0):
    r = 0 if G is None else G.shape[1]
    return (r + p0 + q0 + 8) * U24 * rec_majorant(F, G, A, B, None, p0, q0) + U24 * np.abs(rec_ref(F, G, A, B, mean, p0, q0))


def drops(F, G, A, B, p0, q0):
    """the operands with one edge contribution removed each: the last image of the first run and of the stack, factor column
    r - 1, row p0 - 1 and column q0 - 1 of C, pixel row p - 1 and column q - 1"""
    def without(M, rows=None, cols=None):
        M = M.copy()
        M[rows if rows is not None else slice(None), cols if cols is not None else slice(None)] = 0
        return M
    n = F.shape[0]
    out = {"image %d" % i: (without(F, rows=i), G, A, B) for i in {min(n, RUN) - 1, n - 1}}
    out["factor column r - 1"] = (without(F, cols=F.shape[1] - 1), G, A, B) if G is not None else None
    out["row p0 - 1"] = (F, G, without(A, cols=p0 - 1), B)
    out["column q0 - 1"] = (F, G, A, without(B, cols=q0 - 1))
    out["pixel row p - 1"] = (F, G, without(A, rows=A.shape[0] - 1), B)
    out["pixel column q - 1"] = (F, G, A, without(B, rows=B.shape[0] - 1))
    return {k: v for k, v in out.items() if v is not None}


@functools.lru_cache(maxsize=None)
def int_case(n, p, q, p0, q0, r, with_g, with_mean):
    """F, G, A, B, mean, expected x^.  The seeds advance until every edge contribution of drops() shows in the expected output"""
    m = p0 * q0
    mean = int_mean(p, q, 5) if with_mean else None
    for seed in range(0, 60, 3):
        rng = np.random.default_rng([n, p, q, p0, q0, r, seed])
        F = rng.integers(-2, 3, (n, r)).astype(np.float32)
        F[:, r - 1][F[:, r - 1] == 0] = 1.0
        G, A, B = int_proj(m, r, seed) if with_g else None, int_proj(p, p0, seed + 1), int_proj(q, q0, seed + 2)
        ref = rec_ref(F, G, A, B, mean, p0, q0)
        if all(not np.array_equal(rec_ref(f, g, a, b, mean, p0, q0), ref) for f, g, a, b in drops(F, G, A, B, p0, q0).values()):
            break
    return F, G, A, B, mean, ref


@functools.lru_cache(maxsize=None)
def real_case(n, p, q, p0, q0, r, with_g, seed):
    """F, G, A, B, mean (float32, orthonormal bases), the float64 x^ of these float32 operands, the bound"""
    rng = np.random.default_rng(seed)
    F = (rng.standard_normal((n, r)) * np.linspace(3.0, 0.3, r)).astype(np.float32)
    G, A, B = real_proj(p0 * q0, r, seed + 1) if with_g else None, real_proj(p, p0, seed + 2), real_proj(q, q0, seed + 3)
    mean = (0.5 + 0.2 * rng.standard_normal((p, q))).astype(np.float32)
    return F, G, A, B, mean, rec_ref(F, G, A, B, mean, p0, q0), rec_bound(F, G, A, B, mean, p0, q0)


REAL_CASES = [(9, 33, 47, 5, 4, 7, True, 70), (9, 33, 47, 5, 4, 20, False, 71), (10, 90, 90, 25, 25, 50, True, 72)]


def f32_reconstruct(F, G, A, B, mean, p0, q0, cut=lambda a: a):
    """the device's three products and the add in float32 numpy; cut is applied to every operand of every product"""
    c = cut(F) if G is None else cut(F) @ cut(G).T
    T = np.matmul(cut(c).reshape(-1, p0, q0), cut(B).T)
    xh = np.matmul(cut(A), cut(T)) + mean
    assert xh.dtype == np.float32
    return xh.astype(np.float64)


def planted(sigma, n=160, seed=11, junk=()):
    """make_sdr_pins.low_rank's construction (U0 C_i V0^T + 0.5, rank 3 x 4, distinct coefficient scales) under white noise of
    deviation sigma; the images listed in junk are replaced by white noise of their own mean and variance.  Returns the noisy
    float32 stack and the clean float64 one"""
    rng = np.random.default_rng(seed)
    p, q = 20, 24
    U0 = np.linalg.qr(rng.standard_normal((p, 3)))[0]
    V0 = np.linalg.qr(rng.standard_normal((q, 4)))[0]
    s, t = np.array([8.0, 3.0, 1.0]), np.array([5.0, 2.2, 1.3, 0.6])
    C = rng.standard_normal((n, 3, 4)) * s[:, None] * t[None, :]
    clean = np.einsum("pa,iab,qb->ipq", U0, C, V0) + 0.5
    arr = clean + sigma * rng.standard_normal((n, p, q))
    for i in junk:
        arr[i] = arr[i].mean() + arr[i].std() * rng.standard_normal((p, q))
    return arr.astype(np.float32), clean


# ---- the builders' own properties

@pytest.mark.parametrize("case", INT_CASES)
def test_integer_cases_are_exact_and_sensitive(case):
    n, p, q, p0, q0, r, with_g, with_mean = case
    F, G, A, B, mean, ref = int_case(*case)
    assert is_integer_f32(F, G, A, B, mean) and np.abs(F).max() <= 2 and ref.shape == (n, p, q)
    assert rec_majorant(F, G, A, B, mean, p0, q0).max() < LIMIT
    assert np.array_equal(ref, np.rint(ref)) and (G is None) == (not with_g) and (mean is None) == (not with_mean)
    for name, (f, g, a, b) in drops(F, G, A, B, p0, q0).items():
        assert not np.array_equal(rec_ref(f, g, a, b, mean, p0, q0), ref), name
    # image i's x^ depends on row i of F alone
    assert np.array_equal(rec_ref(F[n - 1:], G, A, B, mean, p0, q0)[0], ref[n - 1])


def test_integer_cases_cover_the_edges():
    col = lambda i: {c[i] for c in INT_CASES}
    assert col(0) >= {1, RUN - 1, RUN, RUN + 1} and col(1) >= {1, 15, 16, 17, 90, 255, 256} <= col(2)
    assert col(3) >= {1, 16, 17, 49, 64} <= col(4) and {c[5] for c in INT_CASES if c[6]} >= {1, 64, 65, 256}
    assert (9, 64, 64, 64, 32, 256, True, True) in INT_CASES and any(not c[6] for c in INT_CASES) and any(not c[7] for c in INT_CASES)
    assert all(p0 <= min(p, 64) and q0 <= min(q, 64) and p0 * q0 <= 2048 and r == (r if g else p0 * q0) and r <= max(256 * g, p0 * q0)
               for n, p, q, p0, q0, r, g, mu in INT_CASES)
    # every register plan of the kernel: steps 4 ceil(max(p0, q0) / 16), tiles ceil(max(p, q) / 64), and both at their largest
    assert {-(-max(c[3], c[4]) // 16) for c in INT_CASES} == {1, 2, 3, 4} == {-(-max(c[1], c[2]) // 64) for c in INT_CASES}
    assert any(max(c[3], c[4]) > 48 and max(c[1], c[2]) > 192 for c in INT_CASES)


@pytest.mark.parametrize("case", REAL_CASES)
def test_bound_separates_float32_from_a_10_bit_mantissa(case):
    n, p, q, p0, q0, r, with_g, seed = case
    F, G, A, B, mean, ref, bound = real_case(*case)
    assert np.all(bound > 0) and bound.shape == ref.shape == (n, p, q)
    inside = float(np.max(np.abs(f32_reconstruct(F, G, A, B, mean, p0, q0) - ref) / bound))
    outside = float(np.max(np.abs(f32_reconstruct(F, G, A, B, mean, p0, q0, cut10) - ref) / bound))
    print("RATIO float32 numpy reconstruct %.4f, 10-bit %.4f" % (inside, outside))
    assert inside <= 1.0 < outside


# ---- 1. the reference's pinned outputs

def golden(k):
    z = np.load(GOLDEN)
    return {key[:-len("_%d" % k)]: z[key] for key in z.files if key.endswith("_%d" % k)}


def reference_reconstruction(c, two_stage):
    """the reference's own outputs through the contract: mean + A reshape(G f) B^T in float64"""
    pre = "" if two_stage else "m"
    p, q = c["arr"].shape[1:]
    model = sdr.SdrModel(c[pre + "mean"].reshape(p, q), c[pre + "A"], c[pre + "B"], c["G"] if two_stage else None)
    return sdr.reconstruct(c[pre + "factors"], model, backend="numpy")


@functools.lru_cache(maxsize=None)
def fitted(k, two_stage):
    c = golden(k)
    p0, q0, r = int(c["p0"]), int(c["q0"]), int(c["r"])
    res = sdr.two_sdr(c["arr"], p0, q0, r, backend="numpy") if two_stage else sdr.mpca(c["arr"], p0, q0, backend="numpy")
    return c["arr"], res, sdr.SdrModel.from_result(res)


@pytest.mark.parametrize("two_stage", [True, False])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_denoise_matches_the_reference_reconstruction(k, two_stage):
    arr, res, model = fitted(k, two_stage)
    ref = reference_reconstruction(golden(k), two_stage)
    got = sdr.denoise(arr, model, backend="numpy")
    scale = np.abs(arr - model.mean).max()
    err = np.abs(got.astype(np.float64) - ref).max() / scale
    print("case %d %s: max |x^ - reference| / scale = %.2e" % (k, "2SDR" if two_stage else "MPCA", err))
    assert got.shape == arr.shape and got.dtype == np.float32 and err < 1e-4


# ---- 2. identities

@pytest.mark.parametrize("two_stage", [True, False])
def test_identities(two_stage):
    arr, res, model = fitted(2, two_stage)
    x = arr.astype(np.float64)
    scale = np.abs(arr - model.mean).max()
    f = sdr.transform(arr, model, backend="numpy")
    assert f.shape == res.factors.shape and np.abs(f - res.factors).max() <= 1e-12 * scale
    f64 = sdr.transform(x, model, backend="numpy")
    rng = np.random.default_rng(3)
    f1, f2 = rng.standard_normal(f.shape), rng.standard_normal(f.shape)
    R = lambda v: sdr.reconstruct(v, model, add_mean=False, backend="numpy")
    assert np.abs(R(2.0 * f1 - 3.0 * f2) - (2.0 * R(f1) - 3.0 * R(f2))).max() <= 1e-12 * np.abs(R(f1)).max()
    assert np.abs(sdr.reconstruct(f1, model, backend="numpy") - (R(f1) + model.mean)).max() <= 1e-12 * scale
    d1, resid = sdr.denoise(x, model, residuals=True, backend="numpy")
    assert d1.dtype == np.float64 and np.abs(sdr.denoise(d1, model, backend="numpy") - d1).max() <= 1e-12 * scale
    E = sdr.eigenimages(model, backend="numpy")
    assert E.shape == (model.width,) + arr.shape[1:]
    assert np.abs(E.reshape(model.width, -1) @ E.reshape(model.width, -1).T - np.eye(model.width)).max() <= 1e-12
    assert np.array_equal(sdr.eigenimages(model, 3, backend="numpy"), E[:3])
    # resid = sum (x - mean)^2 - |f|^2, up to the float32 rounding of x^ that the contract puts into resid
    xc = x - model.mean
    slack = 4 * U24 * (np.abs(x - d1) * np.abs(d1)).sum(axis=(1, 2)) + 1e-12 * (xc ** 2).sum(axis=(1, 2))
    assert resid.shape == (arr.shape[0],) and resid.dtype == np.float64
    assert np.all(np.abs(resid - ((xc ** 2).sum(axis=(1, 2)) - (f64 ** 2).sum(axis=1))) <= slack)


def test_numpy_backend_copies_its_input_and_fills_out():
    arr, res, model = fitted(0, True)
    keep = arr.copy()
    out = np.empty_like(arr)
    got = sdr.denoise(arr, model, out=out, backend="numpy")
    assert got is out and np.array_equal(arr, keep) and np.array_equal(out, sdr.denoise(arr, model, backend="numpy"))
    assert sdr.transform(arr[:0], model, backend="numpy").shape == (0, model.width)
    assert sdr.denoise(arr[:0], model, backend="numpy").shape == (0,) + arr.shape[1:]
    for bad in (lambda: sdr.transform(arr[:, :-1], model, backend="numpy"), lambda: sdr.reconstruct(res.factors[:, :-1], model, backend="numpy"),
                lambda: sdr.denoise(arr, model, out=out[:-1], backend="numpy"), lambda: sdr.eigenimages(model, model.width + 1, backend="numpy"),
                lambda: sdr.eigenimages(model, 0, backend="numpy"), lambda: sdr.transform(arr, model, backend="eager"),
                lambda: sdr.transform(arr, model)):
        with pytest.raises(sdr.SdrError):
            bad()
    assert api.sdr_denoise(arr, model, backend="numpy").shape == arr.shape
    assert api.sdr_transform(arr, model, backend="numpy").shape == res.factors.shape
    assert api.sdr_reconstruct(res.factors, model, backend="numpy").shape == arr.shape


# ---- 3. quality, 4. junk

SIGMA, GAIN = 2.0, 8.0       # noise deviation against coefficient scales of 0.6 .. 40; the least factor by which the MSE falls


def test_denoising_lowers_the_error_to_the_clean_images():
    """At sigma = 2 the noisy stack is off the clean one by sigma^2 = 4 per pixel.  Rank (3, 4, 5) keeps about 5 / 480 of the
    noise (0.04) and drops the 7 weakest of the 12 planted coefficients (73 / 480 = 0.15 per pixel): about 0.2, a factor near
    20 with the subspace's own error; the test asks for 8."""
    arr, clean = planted(SIGMA)
    model = sdr.SdrModel.from_result(sdr.two_sdr(arr, 3, 4, 5, backend="numpy"))
    before = ((arr - clean) ** 2).mean()
    after = ((sdr.denoise(arr, model, backend="numpy") - clean) ** 2).mean()
    print("MSE to the clean images: %.4f -> %.4f, a factor of %.1f" % (before, after, before / after))
    assert before > 0.95 * SIGMA ** 2 and before / after >= GAIN


def test_junk_images_have_the_largest_relative_residuals():
    """sigma = 0.5: a member keeps its planted part (resid_rel well below 1), white noise keeps about r / (p q) of its energy"""
    junk = (3, 77, 78, 159)
    arr, _ = planted(0.5, junk=junk)
    model = sdr.SdrModel.from_result(sdr.two_sdr(arr, 3, 4, 5, backend="numpy"))
    _, resid = sdr.denoise(arr, model, residuals=True, backend="numpy")
    rel = resid / ((arr - model.mean).astype(np.float64) ** 2).sum(axis=(1, 2))
    members = np.delete(rel, junk)
    print("resid_rel: junk %s, members' largest %.4f" % (np.round(rel[list(junk)], 4), members.max()))
    assert rel[list(junk)].min() > members.max() and rel[list(junk)].min() > 0.9


# ---- 5. model file and tool

@pytest.mark.parametrize("two_stage", [True, False])
def test_model_file_round_trip_and_tool_output(tmp_path, two_stage):
    arr, res, model = fitted(0, two_stage)
    model.save(str(tmp_path / "m.npz"))
    back = sdr.SdrModel.load(str(tmp_path / "m.npz"))
    for a, b in ((back.mean, model.mean), (back.A, model.A), (back.B, model.B)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert (back.G is None) == (not two_stage) and (two_stage is False or np.array_equal(back.G, model.G))
    assert (back.p, back.q, back.p0, back.q0, back.m, back.width) == (20, 24, 3, 4, 12, 5 if two_stage else 12)
    # the tool's OUT.npz, as it has always written it: a G of zero columns means MPCA
    np.savez(str(tmp_path / "out.npz"), factors=res.factors, G=res.G if res.G is not None else np.zeros((12, 0)), A=res.A, B=res.B,
             mean=res.mean, iterations=np.int64(res.iterations), energies=np.asarray(res.energies), p0=np.int64(3), q0=np.int64(4),
             r=np.int64(5 if two_stage else 0))
    tool = sdr.SdrModel.load(str(tmp_path / "out.npz"))
    assert (tool.G is None) == (not two_stage)
    assert np.array_equal(sdr.denoise(arr, tool, backend="numpy"), sdr.denoise(arr, model, backend="numpy"))
    assert set(model.arrays()) | {"factors", "iterations", "energies"} == OLD_KEYS
    z = dict(np.load(str(tmp_path / "m.npz")))
    assert z["G"].shape == ((12, 5) if two_stage else (12, 0)) and int(z["r"]) == (5 if two_stage else 0)


def test_model_shape_checks(tmp_path):
    arr, res, model = fitted(0, True)
    for bad in (lambda: sdr.SdrModel(model.mean, model.A[:-1], model.B, model.G), lambda: sdr.SdrModel(model.mean, model.A, model.B[:-1]),
                lambda: sdr.SdrModel(model.mean, model.A, model.B, model.G[:-1]), lambda: sdr.SdrModel(model.mean.ravel(), model.A, model.B),
                lambda: sdr.SdrModel(model.mean, model.A, model.B, np.zeros((12, 13))),
                lambda: sdr.SdrModel(np.zeros((300, 24), np.float32), np.zeros((300, 3)), model.B)):
        with pytest.raises(sdr.SdrError):
            bad()
    np.savez(str(tmp_path / "no.npz"), A=model.A)
    with pytest.raises(sdr.SdrError):
        sdr.SdrModel.load(str(tmp_path / "no.npz"))


def test_tool_usage_errors_exit_with_status_2(tmp_path, capsys):
    arr, res, model = fitted(0, True)
    stack, mfile, out = str(tmp_path / "s.npy"), str(tmp_path / "m.npz"), str(tmp_path / "o.npz")
    np.save(stack, arr)
    model.save(mfile)
    np.save(str(tmp_path / "other.npy"), arr[:, :, :-1])
    cases = [[stack, out, "--model", mfile, "--" + o, v] for o, v in (("p0", "3"), ("q0", "4"), ("r", "5"), ("max_iter", "3"), ("tol", "0"))]
    cases += [[stack, out, "--model", mfile, "--mpca"], [stack, out, "--n_eig", "2"], [stack, out, "--batch", "7"],
              [stack, out, "--model", mfile, "--batch", "0"], [str(tmp_path / "other.npy"), out, "--model", mfile]]
    for argv in cases:
        with pytest.raises(SystemExit) as e:
            sdr.main(argv)
        assert e.value.code == 2, argv
        assert not os.path.exists(out)
    capsys.readouterr()
