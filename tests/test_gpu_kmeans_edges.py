"""The k-means kernels entry by entry at their tile, run and screen edges, on the inputs of tests/test_kmeans_edges_cpu.py (whose
properties that file asserts without a GPU).  Integer-valued data make every float64 distance, sum and potential exact, so labels,
inertia, centres, potentials and indices are compared for equality; the one real-valued case uses a bound derived from the
kernel's stated order of summation, and the centre shift (a sum of squares of non-integers) a bound from its term count."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api, kmeans  # noqa: E402
from test_kmeans_edges_cpu import (MULTS, MULTS_LONG_RUN, MULTS_SHORT, RELOCATION_CASES, SEARCH_N, SEED_SHAPES,  # noqa: E402
                                   copies_case, counted_case, crowded_case, expected_update, overflow_case,
                                   plusplus_case, real_case, real_centre_reference, relocation_case, search_case, seed_case,
                                   seed_reference, ties_case, tiling_cases)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on(dev, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


# ---- 1. E-step tiling

@pytest.mark.parametrize("d,k,n", tiling_cases())
def test_estep_tiling_exact_labels_and_inertia(dev, d, k, n):
    X, C, lab, dmin = ties_case(d, k, n)
    got, inertia = kmeans.labels_for(on(dev, X), C)
    assert np.array_equal(got, lab), np.nonzero(got != lab)[0][:10]
    assert inertia == float(np.sum(dmin))


# ---- 2. crowded screen

@pytest.mark.parametrize("d", [9, 35, 128])
@pytest.mark.parametrize("m", [16, 17, 20])
def test_crowded_screen(dev, d, m):
    X, C, lab, dmin, D = crowded_case(d, m)
    got, inertia = kmeans.labels_for(on(dev, X), C)
    assert np.array_equal(got, lab), np.nonzero(got != lab)[0][:10]
    assert inertia == float(np.sum(dmin))


@pytest.mark.parametrize("d", [9, 35, 128])
def test_identical_copies_lowest_wins(dev, d):
    X, C, lab, dmin, D, pos = copies_case(d)
    got, inertia = kmeans.labels_for(on(dev, X), C)
    assert np.array_equal(got, lab), np.nonzero(got != lab)[0][:10]
    assert not np.any(np.isin(got, pos[1:]))
    assert inertia == float(np.sum(dmin))


# ---- 3. overflowing norms

@pytest.mark.parametrize("d", [12, 40])
def test_overflowing_norms(dev, d):
    X, C, ordinary, lab, dmin = overflow_case(d)
    got, inertia = kmeans.labels_for(on(dev, X), C)
    assert np.array_equal(got, lab), np.nonzero(got != lab)[0][:10]
    assert math.isfinite(inertia)
    # the distances are visible through the inertia: exact where every row's distance is a small integer.  The batch without the
    # rows at 2^140 from their centre, and the ordinary rows alone
    small = dmin < 2.0 ** 52
    assert np.all(ordinary <= small) and np.sum(small & ~ordinary) >= 8
    got_s, inertia_s = kmeans.labels_for(on(dev, X[small]), C)
    got_o, inertia_o = kmeans.labels_for(on(dev, X[ordinary]), C)
    assert np.array_equal(got_s, lab[small]) and np.array_equal(got_o, lab[ordinary])
    assert np.array_equal(got_o, got[ordinary]) and np.array_equal(got_o, got_s[ordinary[small]])
    assert inertia_s == float(np.sum(dmin[small])) and inertia_o == float(np.sum(dmin[ordinary]))
    assert inertia_s - float(np.sum(dmin[small & ~ordinary])) == inertia_o
    # the input is finite: the fit accepts it
    r = kmeans.kmeans(on(dev, X), C.shape[0], init=C, max_iter=1)
    rn = kmeans.kmeans(X, C.shape[0], init=C, max_iter=1, backend="numpy")
    assert np.array_equal(r.labels, rn.labels) and r.n_iter == rn.n_iter and math.isfinite(r.inertia)


# ---- 4. one Lloyd step: sums and centres

def shift_bound(Cn, C):
    """(reference, bound) of sum |c_new - c_old|^2: each term carries two roundings (the difference, the square), the sum of the
    N = k d non-negative terms at most N - 1 more in any order: below (N + 2) 2^-53 of the sum"""
    t = (np.asarray(Cn, np.float64) - C) ** 2
    ref = math.fsum(t.ravel())
    return ref, (t.size + 2) * 2.0 ** -53 * ref


def lloyd_both(dev, X, C):
    B = kmeans._Device(on(dev, X))
    Ct = B.centers_from(C)
    Cn, shift, changed = B.lloyd(Ct)
    stats = B.stats.cpu().numpy().copy()
    N = kmeans._Numpy(X)
    Nn, nshift, nchanged = N.lloyd(np.asarray(C, np.float64))
    return B, Ct, Cn, stats, N, Nn


def check_step(dev, X, C, lab):
    n = len(lab)
    B, Ct, Cn, stats, N, Nn = lloyd_both(dev, X, C)
    got = Cn.cpu().numpy()
    assert np.array_equal(B.labels_numpy(), lab)
    assert np.array_equal(got, Nn), np.argwhere(got != Nn)[:10]
    ref, bound = shift_bound(Nn, C)
    assert abs(stats[0] - ref) <= bound and stats[1] == n and stats[2] == 0
    Cn2, shift2, changed2 = B.lloyd(Ct)                      # the labels kept: nothing changes
    assert changed2 == 0 and np.array_equal(Cn2.cpu().numpy(), got) and shift2 == stats[0]


@pytest.mark.parametrize("d,mults", [(9, MULTS), (255, MULTS), (256, MULTS), (257, MULTS), (513, MULTS), (2048, MULTS_SHORT)])
def test_lloyd_step_sums_and_centres(dev, d, mults):
    X, C, lab = counted_case(d, mults)
    check_step(dev, X, C, lab)


def test_lloyd_step_long_runs(dev):
    X, C, lab = counted_case(9, MULTS_LONG_RUN)
    check_step(dev, X, C, lab)


def test_lloyd_step_real_valued_within_the_derived_bound(dev):
    """Measured on an MI355X: the largest error / bound ratio over the 514 centre entries is printed by the test."""
    X, C, lab = real_case()
    B = kmeans._Device(on(dev, X))
    Cn, shift, changed = B.lloyd(B.centers_from(C))
    assert np.array_equal(B.labels_numpy(), lab) and changed == len(lab)
    ref, bound = real_centre_reference(X, lab, 2)
    err = np.abs(Cn.cpu().numpy().astype(np.longdouble) - ref).astype(np.float64)
    print("real-valued centres: max error %.3e, max error / bound %.4f" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)


# ---- 5. relocation

@pytest.mark.parametrize("d", [3, 40])
@pytest.mark.parametrize("variant,e,heavy_low", RELOCATION_CASES)
def test_relocation(dev, d, variant, e, heavy_low):
    r = relocation_case(d, e, variant, heavy_low)
    B, Ct, Cn, stats, N, Nn = lloyd_both(dev, r.X, r.C)
    got = Cn.cpu().numpy()
    assert np.array_equal(B.labels_numpy(), r.labels)
    assert np.array_equal(Nn, expected_update(r))
    assert np.array_equal(got, Nn), np.argwhere(got != Nn)[:10]
    # stats[2] is the number of clusters found empty (include/ralign.h), also when nothing is moved
    assert stats[1] == len(r.labels) and stats[2] == e
    ref, bound = shift_bound(Nn, r.C)
    assert abs(stats[0] - ref) <= bound
    B.finish(Cn, True)
    N.finish(Nn, True)
    assert np.array_equal(B.labels_numpy(), N.labels_numpy())


# ---- 6. search

def device_search(L, w, vals, dev):
    v = on(dev, vals, np.float64)
    idx = torch.full((len(vals),), -7, dtype=torch.int32, device=dev)
    assert L.ra_kmeans_search(P(w), int(w.numel()), P(v), len(vals), P(idx), stream()) == 0
    return idx.cpu().numpy()


@pytest.mark.parametrize("n", SEARCH_N)
def test_search_matches_searchsorted(dev, n):
    L = api.load_library()
    w, vals, ref, placed = search_case(n)
    wd = on(dev, w, np.float64)
    assert np.array_equal(device_search(L, wd, vals, dev), ref)                       # m = 16
    one = np.array([device_search(L, wd, vals[j:j + 1], dev)[0] for j in range(len(vals))])
    assert np.array_equal(one, ref)                                                   # m = 1


# ---- 7. seed

@pytest.mark.parametrize("n,d", SEED_SHAPES)
def test_seed_steps_exact(dev, n, d):
    L = api.load_library()
    X, first, lists = seed_case(n, d)
    steps = seed_reference(X, first, lists)
    Xd = on(dev, X)
    closest = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    for step, cand in enumerate([np.array([first], np.int32)] + lists):
        m = len(cand)
        out = torch.full((m + 2,), -7.0, dtype=torch.float64, device=dev)
        assert L.ra_kmeans_seed(P(Xd), n, d, P(on(dev, cand, np.int32)), m, P(closest), int(step == 0), P(out), stream()) == 0
        chosen, pot, pots, want = steps[step]
        o = out.cpu().numpy()
        assert o[0] == chosen and o[1] == pot and np.array_equal(o[2:], pots), (step, o, chosen, pots)
        assert np.array_equal(closest.cpu().numpy(), want)


def test_plusplus_init_indices_match_numpy(dev):
    X = plusplus_case()
    with torch.cuda.device(dev):
        got = kmeans._plusplus(kmeans._Device(on(dev, X)), 8, np.random.RandomState(11))
    want = kmeans._plusplus(kmeans._Numpy(X), 8, np.random.RandomState(11))
    assert np.array_equal(got, want)
