"""2SDR / MPCA without a GPU: the numpy backend against the reference's own MPCA / TwoSDR (tests/golden/sdr_ref.npz, written
by make_sdr_pins.py), the loop rules, the sign convention, the domain and the tool's params-file parser."""
import os

import numpy as np
import pytest

from cryo_ralib_amd import sdr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdr_ref.npz")
LOW_RANK, NOISY, SYNTH = 0, 1, 2


def case(k):
    z = np.load(GOLDEN)
    return {key[:-len("_%d" % k)]: z[key] for key in z.files if key.endswith("_%d" % k)}


def proj(M):
    return M @ M.T


def energy(arr, A, B, mean=None):
    """sum_i ||A^T X_i B||_F^2, X_i centred by `mean` in fp32 (as the backends do) or by the float64 mean"""
    X = (arr - mean.reshape(arr.shape[1:])).astype(np.float64) if mean is not None else arr.astype(np.float64) - arr.astype(np.float64).mean(0)
    return float((np.einsum("ra,irc,cb->iab", A, X, B) ** 2).sum())


def check_against_reference(res, c, two_stage):
    pre = "" if two_stage else "m"
    A, B = c[pre + "A"], c[pre + "B"]
    assert np.abs(proj(res.A) - proj(A)).max() < 1e-4
    assert np.abs(proj(res.B) - proj(B)).max() < 1e-4
    assert np.abs(res.mean.ravel() - c[pre + "mean"].ravel()).max() < 1e-6
    if two_stage:
        # G lives in the coordinates of kron(A, B): align the signs of A and B first
        d = np.kron(np.sign((res.A * A).sum(0)), np.sign((res.B * B).sum(0)))
        assert np.abs(proj(res.G * d[:, None]) - proj(c["G"])).max() < 1e-4
    F, Fr = res.factors, c[pre + "factors"]
    assert F.shape == Fr.shape
    s = np.sign((F * Fr).sum(0))
    err = np.abs(F * s - Fr).max(0) / np.linalg.norm(Fr, axis=0)
    assert err.max() < 1e-3, err


@pytest.mark.parametrize("k", [LOW_RANK, SYNTH])
def test_numpy_two_sdr_matches_reference(k):
    c = case(k)
    res = sdr.two_sdr(c["arr"], int(c["p0"]), int(c["q0"]), int(c["r"]), backend="numpy")
    check_against_reference(res, c, True)


@pytest.mark.parametrize("k", [LOW_RANK, SYNTH])
def test_numpy_mpca_matches_reference(k):
    c = case(k)
    res = sdr.mpca(c["arr"], int(c["p0"]), int(c["q0"]), backend="numpy")
    assert res.G is None
    check_against_reference(res, c, False)


def test_numpy_noise_dominated_captures_reference_energy():
    c = case(NOISY)
    res = sdr.two_sdr(c["arr"], int(c["p0"]), int(c["q0"]), int(c["r"]), backend="numpy")
    assert res.iterations == 30
    e_ref, e = energy(c["arr"], c["A"], c["B"]), energy(c["arr"], res.A, res.B)
    assert abs(e - e_ref) / e_ref < 1e-4
    e = energy(c["arr"], res.A, res.B, res.mean)
    assert abs(res.energies[-1] - e) / e < 1e-10


def test_low_rank_case_converges_early():
    c = case(LOW_RANK)
    assert sdr.mpca(c["arr"], 3, 4, backend="numpy").iterations < 30


def test_max_iter_caps_the_loop():
    c = case(NOISY)
    for it in (1, 2, 5):
        res = sdr.mpca(c["arr"], 8, 6, max_iter=it, backend="numpy")
        assert res.iterations == it and len(res.energies) == it


def test_tolerance_is_a_signed_test():
    c = case(NOISY)
    full = sdr.mpca(c["arr"], 8, 6, backend="numpy")
    d = np.diff(full.energies) / c["arr"].shape[0]
    # with tol below every step the loop runs to the cap; a tol just above step k stops right there
    assert sdr.mpca(c["arr"], 8, 6, tol=-np.inf, backend="numpy").iterations == 30
    k = int(np.argmax(d > 0)) if (d > 0).any() else 0
    res = sdr.mpca(c["arr"], 8, 6, tol=d[k] * (1 + 1e-6) if d[k] > 0 else d[k] + 1e-12, backend="numpy")
    assert res.iterations == k + 2
    # a negative change always stops (signed, not absolute)
    res = sdr.mpca(c["arr"], 8, 6, tol=1e-300, backend="numpy")
    assert res.iterations == (int(np.argmax(d < 1e-300)) + 2 if (d < 1e-300).any() else 30)


def test_energy_equals_eigenvalue_sum():
    for k in (LOW_RANK, NOISY, SYNTH):
        c = case(k)
        res = sdr.mpca(c["arr"], int(c["p0"]), int(c["q0"]), max_iter=3, backend="numpy")
        e = energy(c["arr"], res.A, res.B, res.mean)
        assert abs(res.energies[-1] - e) / e < 1e-10


def test_sign_convention():
    V = np.array([[0.1, -0.7, 0.5], [-0.9, 0.7, -0.5], [0.3, 0.1, 0.0]])
    W = sdr.fix_signs(V)
    assert np.array_equal(W[:, 0], -V[:, 0])          # -0.9 is the largest entry
    assert np.array_equal(W[:, 1], -V[:, 1])          # tie: the first of |-0.7| = |0.7| decides
    assert np.array_equal(W[:, 2], V[:, 2])
    rng = np.random.default_rng(0)
    S = rng.standard_normal((7, 7)); S = S + S.T
    w, E = sdr.top_eig(S, 4)
    assert np.all(np.diff(w) <= 0)
    assert np.all(E[np.argmax(np.abs(E), axis=0), np.arange(4)] > 0)
    assert np.allclose(S @ E, E * w)


@pytest.mark.parametrize("shape,p0,q0,r", [
    ((10, 0, 8), 1, 1, 1), ((10, 257, 8), 1, 1, 1), ((10, 8, 300), 1, 1, 1),
    ((10, 8, 8), 0, 2, 1), ((10, 8, 8), 9, 2, 1), ((10, 80, 80), 65, 2, 1),
    ((10, 8, 8), 2, 0, 1), ((10, 8, 8), 2, 9, 1), ((10, 80, 80), 2, 65, 1),
    ((10, 64, 64), 64, 64, 1),                                      # p0 q0 = 4096 > 2048
    ((10, 8, 8), 2, 2, 0), ((10, 8, 8), 2, 2, 4), ((3, 8, 8), 2, 2, 3), ((400, 64, 64), 32, 32, 257),
    ((0, 8, 8), 1, 1, None),
])
def test_domain_checks(shape, p0, q0, r):
    with pytest.raises(sdr.SdrError):
        sdr.check_domain(shape[0], shape[1], shape[2], p0, q0, r)
    if shape[0] >= 1 and min(shape[1:]) >= 1 and max(shape[1:]) <= 12:
        with pytest.raises(sdr.SdrError):
            if r is None:
                sdr.mpca(np.zeros(shape, np.float32), p0, q0, backend="numpy")
            else:
                sdr.two_sdr(np.zeros(shape, np.float32), p0, q0, r, backend="numpy")


def test_domain_edges_accepted():
    sdr.check_domain(1, 1, 1, 1, 1, None)
    sdr.check_domain(2, 1, 2, 1, 2, 1)
    sdr.check_domain(300, 256, 256, 32, 64, 256)
    sdr.check_domain(300, 40, 256, 40, 51, 256)
    with pytest.raises(sdr.SdrError):
        sdr.check_domain(10, 8, 8, 2, 2, 1, max_iter=0)
    with pytest.raises(sdr.SdrError):
        sdr.two_sdr(np.zeros((4, 8, 8), np.float32), 2, 2, 1, backend="cpu")


def test_params_file_layouts(tmp_path):
    from cryo_ralib_amd import stackio
    rng = np.random.default_rng(3)
    prm = np.column_stack([rng.uniform(0, 360, 5), rng.uniform(-2, 2, 5), rng.uniform(-2, 2, 5), rng.integers(0, 2, 5)])
    p6 = tmp_path / "params.txt"
    order = [3, 0, 4, 1, 2]
    stackio.write_text_rows(str(p6), [(i, float(prm[i, 0]), float(prm[i, 1]), float(prm[i, 2]), int(prm[i, 3]), 7) for i in order])
    got = sdr.read_params(str(p6), 5)
    assert np.allclose(got, prm, atol=1e-5)
    p4 = tmp_path / "initial2Dparams.txt"
    stackio.write_text_rows(str(p4), [(float(a), float(b), float(c), int(d)) for a, b, c, d in prm])
    assert np.allclose(sdr.read_params(str(p4), 5), prm, atol=1e-5)
    with pytest.raises(sdr.SdrError, match="rows"):
        sdr.read_params(str(p6), 6)
    with pytest.raises(sdr.SdrError, match="rows"):
        sdr.read_params(str(p4), 4)
    bad = tmp_path / "bad.txt"
    bad.write_text("1 2 3\n4 5 6\n")
    with pytest.raises(sdr.SdrError, match="columns"):
        sdr.read_params(str(bad), 2)
    dup = tmp_path / "dup.txt"
    stackio.write_text_rows(str(dup), [(0, 1.0, 0.0, 0.0, 0, 0), (0, 1.0, 0.0, 0.0, 0, 0)])
    with pytest.raises(sdr.SdrError, match="permutation"):
        sdr.read_params(str(dup), 2)
