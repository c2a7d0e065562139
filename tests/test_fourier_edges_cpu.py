"""Everything tests/test_gpu_fourier_edges.py relies on, asserted without a GPU on the cases of tests/fourier_edge_cases.py:

  * the coverage claim: the restated rs_make_plan sends the resize cases through resize_kernel<1> .. <8> and nt = 1, 2, 3, and
    every case has the edges it is named for; the filter boxes have the radices, batch and route they are named for;
  * the references: resize.operator agrees with a direct long-double cosine sum to 2^-45 (largest: 1.9e-14 = 2^-45.6 at
    24 -> 330, where the closed form divides by the smallest sine; every other shape stays below 2^-46).  The 2^-40 floor of the
    impulse bound stays as it is: it covers the resulting error of a product of two entries, 2 delta max|A| + delta^2, 16 times
    over, which is asserted.  operator(nx, nx) is the identity to 2^-50 off the diagonal and exactly 1 on it;
  * a float32 replay of the kernel's arithmetic (numpy, the kernel's k order) meets every bound the device is held to: the
    identity bit for bit (R1), the impulse stack within 3 u |y| + 2^-40 (R2), noise with a bright pixel within
    (K1 + K2 + 3) u |A| |x| |A|^T (R3); the single-precision CPU filter defines the F1 bar, which is at most 1e-5;
  * every applicable mutant of the operator, the output, or the gain table exceeds those bounds, and the faintest of them (one
    far operator entry times 1.01, one stop-band gain doubled) passes the norm bars of tests/test_gpu_resize.py (2e-5 max|x|)
    and tests/test_gpu_prep.py (1e-5 max|ref|) at the shapes those tests use -- the gap the entry-wise tests close."""
import numpy as np
import pytest

import fourier_edge_cases as fc
from cryo_ralib_amd import prep

OLD_RESIZE_BAR, OLD_FILTER_BAR = 2e-5, 1e-5
OLD_FILTER_BOXES = (45, 64, 90)      # the pad=False boxes of test_filter_matches_the_checker among FILTER_BOXES


# ---- coverage

def test_resize_cases_reach_every_instantiation_and_tile_count():
    plans = [fc.rs_plan(nx, m) for nx, m in fc.RESIZE_SHAPES]
    ident = [fc.rs_plan(nx, nx) for nx in fc.IDENTITY]
    assert {p["nct"] for p in plans + ident} == set(range(1, 9))
    assert {p["nct"] for p in plans} == {1, 2, 3, 5, 6, 7, 8}       # NCT 4 runs through the identity at 63 and 64
    assert {p["nt"] for p in plans} == {1, 2, 3}
    assert {p["nct"] for p in ident} >= {1, 4, 5, 7} and {p["nt"] for p in ident} == {1, 2}
    assert any(p["nct"] == 7 and p["nt"] > 1 for p in plans)
    for nx, m in fc.RESIZE_SHAPES:                               # tiny: at most 130 images of 130^2 in, 330^2 out
        assert 1 <= nx <= 130 and 1 <= m <= 330 and fc.rs_plan(nx, m)["bt"] <= 128
    assert max(fc.IDENTITY) <= 200


@pytest.mark.parametrize("nx,m,edges", fc.RESIZE_CASES)
def test_resize_case_has_its_named_edges(nx, m, edges):
    p = fc.rs_plan(nx, m)
    assert p["mp"] >= m and p["mp"] - m < 16 * p["nt"] and p["nxp"] >= nx and p["nxp"] % 64 == 0
    for e in edges:
        assert fc.EDGES[e](nx, m, p), e


def test_named_shapes_of_the_plan():
    assert fc.rs_plan(24, 330) == dict(nt=3, bt=112, mp=336, nxp=64, nct=7)
    assert fc.rs_plan(64, 129) == dict(nt=2, bt=80, mp=160, nxp=64, nct=5)
    assert fc.rs_plan(100, 112)["mp"] == 112 and fc.rs_plan(65, 16)["mp"] == 16
    assert fc.rs_plan(360, 90)["nct"] == 6 and fc.rs_plan(1024, 256) == dict(nt=2, bt=128, mp=256, nxp=1024, nct=8)
    for nx, m in fc.UNALIGNED:
        assert nx % 4 == 0 and (nx, m) in fc.RESIZE_SHAPES


@pytest.mark.parametrize("nx", sorted({nx for nx, _ in fc.RESIZE_SHAPES}))
def test_impulse_columns_are_a_permutation(nx):
    c = fc.impulse_columns(nx)
    assert sorted(c.tolist()) == list(range(nx))
    x = fc.impulse_stack(nx)
    assert x.sum() == nx and np.all(x.sum(axis=(1, 2)) == 1)
    if nx > 4:
        assert not np.array_equal(x, x.transpose(0, 2, 1))


def test_filter_boxes_have_their_radices_and_routes():
    for nx, rad in fc.FILTER_BOXES.items():
        assert fc.pf_radices(nx) == rad and int(np.prod(rad)) == nx
        nb, in_lds = fc.pf_batch(nx)
        assert in_lds and nb >= 1
    assert (45 // 2 + 1) % fc.pf_batch(45)[0] != 0        # H % nb != 0: the last column batch is partly filled
    assert 90 in fc.PF_FIXED_NOPAD and 90 in fc.FILTER_BOXES
    assert fc.FILTERS == [tuple(f) for f in fc.FILTERS] and len(fc.FILTERS) == 4
    for nx in fc.FILTER_BOXES:
        for r, c in fc.IMPULSES:
            assert r < nx and c < nx


# ---- the references

@pytest.mark.parametrize("nx,m", fc.RESIZE_SHAPES)
def test_operator_matches_the_direct_cosine_sum(nx, m):
    A = fc.operator64(nx, m)
    delta = float(np.abs(A.astype(np.longdouble) - fc.operator_direct(nx, m)).max())
    print("%d -> %d: max |closed form - cosine sum| = %.3g = 2^%.1f" % (nx, m, delta, np.log2(max(delta, 1e-300))))
    assert delta <= 2.0 ** -45
    amax = float(np.abs(A).max())
    assert 16.0 * (2.0 * delta * amax + delta * delta) <= 2.0 ** -40


@pytest.mark.parametrize("nx", fc.IDENTITY)
def test_identity_operator_and_replay(nx):
    A = fc.operator64(nx, nx)
    assert np.all(np.diag(A) == 1.0)
    assert np.abs(A - np.eye(nx)).max() <= 2.0 ** -50
    x = fc.identity_stack(nx)
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 8
    if nx >= 7:
        assert 0.25 <= (x == 0).mean() <= 0.45 and (x != 0).any()
    y = fc.replay(x, A.astype(np.float32))
    assert np.array_equal(y[x != 0], x[x != 0])
    assert np.all(np.abs(y[x == 0]) <= 2.0 ** -36)
    # 2 nx off-diagonal terms of at most 8 x 2^-50 stay below the 2^-36 allowed at a zero, and far below half an ulp (2^-25) of
    # the smallest non-zero |x|, where they vanish in the float32 sum
    assert 2 * nx * 8 * 2.0 ** -50 <= 2.0 ** -36 < 2.0 ** -25


# ---- the replay within the bounds, the mutants outside them

def ratios(y, ref, bound):
    return float((np.abs(y.astype(np.float64) - ref) / bound).max())


@pytest.mark.parametrize("nx,m", fc.RESIZE_SHAPES)
def test_resize_replay_meets_the_bounds_and_mutants_do_not(nx, m):
    A32 = fc.operator64(nx, m).astype(np.float32)
    # R2
    ref2, y2 = fc.impulse_reference(nx, m), fc.impulse_replay(nx, A32)
    b2 = fc.impulse_bound(ref2)
    sub = sorted({0, 1, nx // 2, nx - 1})
    assert np.array_equal(fc.replay(fc.impulse_stack(nx)[sub], A32), y2[sub])       # one rounded product per entry
    r2 = ratios(y2, ref2, b2)
    # R3
    x = fc.bright_stack(nx)
    assert x.shape == (3, nx, nx) and np.all((x == 1e4).sum(axis=(1, 2)) == 1)
    ref3, b3 = fc.reference(x, nx, m), fc.general_bound(x, nx, m)
    assert np.all(b3 > 0)
    r3 = ratios(fc.replay(x, A32), ref3, b3)
    print("%d -> %d: replay error / bound: impulses %.2f, general %.3f" % (nx, m, r2, r3))
    assert r2 <= 1.0 and r3 <= 1.0
    # mutants
    muts = fc.operator_mutants(nx, m)
    assert "last source column zeroed" in muts
    assert ("Nyquist weight 1" in muts) == fc.has_half(nx, m)
    for name, Am in muts.items():
        q2, q3 = ratios(fc.impulse_replay(nx, Am), ref2, b2), ratios(fc.replay(x, Am), ref3, b3)
        print("    %s: impulses %.3g, general %.3g" % (name, q2, q3))
        assert q2 > 1.0, name
        if name != "far entry times 1.01":
            assert q3 > 1.0, name
    assert ratios(fc.swap_rows(y2), ref2, b2) > 1.0
    if m > 4:
        assert ratios(fc.swap_rows(fc.replay(x, A32)), ref3, b3) > 1.0
    # the faintest mutant against the norm bar of tests/test_gpu_resize.py
    if "far entry times 1.01" in muts:
        j, i = fc.far_entry(nx, m)
        assert 1e-6 < abs(fc.operator64(nx, m)[j, i]) < 1e-3
        xw = fc.white_stack(nx, m)
        err = np.abs(fc.replay(xw, muts["far entry times 1.01"]) - fc.reference(xw, nx, m)).reshape(5, -1).max(1)
        assert np.all(err <= OLD_RESIZE_BAR * np.abs(xw).reshape(5, -1).max(1))


def test_the_far_entry_mutant_applies_to_most_shapes():
    have = [s for s in fc.RESIZE_SHAPES if fc.far_entry(*s) is not None]
    assert len(have) >= len(fc.RESIZE_SHAPES) - 2, have       # 33 -> 17 and 9 -> 90 have no entry in (1e-6, 1e-3)


# ---- filter

@pytest.mark.parametrize("nx", list(fc.FILTER_BOXES))
def test_filter_bar_and_mutants(nx):
    iy = np.fft.fftfreq(nx, 1.0 / nx).round().astype(np.int64)[:, None]
    ix = np.arange(nx // 2 + 1, dtype=np.int64)[None, :]
    x = fc.impulse_images(nx)
    assert np.all(np.abs(np.abs(np.fft.rfft2(x.astype(np.float64))) - 1.0) <= 1e-14)          # every frequency is read
    doubled = 0
    for f, (lp, hp) in enumerate(fc.FILTERS):
        assert np.array_equal(fc.gain(nx, f, iy, ix), prep.filter_multiplier(nx, nx, lp, hp))   # the restated profile
        bar = fc.filter_bar(nx, f)
        print("nx=%d filter %d: E32 %s, bar %s" % (nx, f, fc.e32(nx, f), bar))
        assert bar.shape == (len(fc.IMPULSES),) and np.all(bar >= 16 * fc.U) and np.all(bar <= 1e-5)
        # the double-precision checker sits far inside the bar
        assert np.all(fc.spectrum_error(prep.fourier_filter(x, lp, hp, pad=False, backend="numpy"), nx, f) <= 1e-3 * bar)
        em = fc.spectrum_error(fc.filter32(x, fc.table_unmirrored(nx, f)), nx, f)
        assert np.all(em > bar), (f, em / bar)
        gd = fc.table_stop_band_doubled(nx, f)
        if gd is None:
            continue
        doubled += 1
        ay, kx = fc.stop_band_entry(nx, f)
        assert fc.STOP_BAND[0] <= fc.gain32(nx, f)[ay, kx] < fc.STOP_BAND[1]
        ed = fc.spectrum_error(fc.filter32(x, gd), nx, f)
        assert np.all(ed > bar), (f, ed / bar)
        if nx in OLD_FILTER_BOXES:
            # a pixel moves by about 2 dg / nx: the norm bar of tests/test_gpu_prep.py lets this through at its own boxes (at
            # boxes below 45, which that test does not have, the same bar is sharp enough to see it)
            xw = fc.white_images(nx)
            ref = prep.fourier_filter(xw, lp, hp, pad=False, backend="numpy")
            yw = fc.filter32(xw, gd)
            assert max(np.abs(yw[i] - ref[i]).max() / np.abs(ref[i]).max() for i in range(3)) <= OLD_FILTER_BAR
    assert doubled == 3                       # the high-pass alone has no gain below 1e-3: its stop band is 1 - tanh(pi) at DC
