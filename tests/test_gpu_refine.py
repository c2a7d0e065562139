"""The reference-update kernels (csrc/ralign_refine.h) and their entries at the end of csrc/ralign_engine.hip, entry by entry at
box and curve edges, against the float64 references and on the cases of tests/test_refine_cpu.py (which asserts, without a GPU,
every property of the inputs that a test here relies on).  One engine per box size, nothing searched: the sums are uploaded.

Edge                                                              test
----------------------------------------------------------------  ------------------------------------------------------------
odd boxes (33, 131): kys, inc = nx / 2, no Nyquist weight,        every test at 33; test_per_class_fsc, test_filter_centre_shift,
    the frequency axis i / (2 (nx / 2)), phase_cog's nx / 2       test_normalize_mask at 131
second trip of the 64-thread DFT loops (nxh = 66) and of the      test_per_class_fsc[130|131], test_filter_centre_shift[130|131]
    128-thread inverse rows (nx > 128)
fsc_kernel's thread count min(1024, 4 len): 4 len = 1024, 1028    test_per_class_fsc[254|256]
fsc_fit_kernel: one point per lane full (len 64), the second      test_fit_at_the_lane_edges[126|128|254|256-*]; [32|33-*] with
    chunk's first lane (65), two per lane full (128), the         most lanes idle
    n > 128 branch (129)
fit branches: ordinary, never below 0.5, f0 = 0, fsc[0] < 0       test_fit_at_the_lane_edges[*-signal|same|uncorrelated|signal_negdc]
clamps biting from below and from above                           test_fit_at_the_lane_edges (two clamp sets per case)
live and dead classes, `last` != nref - 1, total == 0,            test_live_class_average[32|33]
    every class dead
class averages with counts around min_count                       test_class_averages_bit_for_bit
ra_filter_references_dev: d_flaa null / set, center = -1 from     test_filter_centre_shift
    device memory, d_cs_out
ensure_refine_ws regrowth (1, 2 nref, 2 nref + 3 images)          test_filter_centre_shift (a fresh engine per box size),
                                                                  test_class_curves_survive_workspace_growth
normalize_mask_kernel, update_refs_kernel                         test_normalize_mask
ra_state_from_params_dev, blocks of 256 (n = 1, 255, 256, 257)    test_state_from_params_dev
fixed summation orders                                            test_repeatability

Every bounded comparison prints its largest error / bound ratio (pytest -s shows them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cryo_ralib_amd import api  # noqa: E402
from oracle import refine_oracle as ro  # noqa: E402
from test_refine_cpu import (DEAD_COUNTS, DEAD_MIN_COUNT, FILTER_FLAA, FILTER_NIMG, FILTER_NX, FIT_KINDS, FIT_NREF, FIT_NX,  # noqa: E402
                             FSC_NX, HOST_FIT_TOL, SMALL_NX, STATE_CS, STATE_N, averaged_curve, centre_bound, circle_mask,
                             class_average_ref, class_fsc_ref, dead_class_sums, engine_geometry, filter_bound, filter_images,
                             filter_shifts, fit_case, freq_axis, fsc_bound, halves, normalize_bound, normalize_kernel_steps,
                             normalize_mask_ref, refine_ref, shell_points, state_check, state_params, state_ref)

SENTINEL = -7.5e30


def make_engine(nx, nref, mode=api.RA_MODE_MREF):
    ou, xr = engine_geometry(nx)
    eng = api.Engine(nx, ou, xr, xr, 1.0, nref, mode)
    eng.use_current_stream()
    return eng


@pytest.fixture(scope="module")
def engines():
    """engines by (nx, nref, mode), created on first use and closed with the module"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cache = {}

    def get(nx, nref, mode=api.RA_MODE_MREF):
        if (nx, nref, mode) not in cache:
            cache[nx, nref, mode] = make_engine(nx, nref, mode)
        return cache[nx, nref, mode]
    yield get
    for e in cache.values():
        e.close()


def on(eng, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(eng.dev)


def host(eng, t):
    eng.sync()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def report(name, ratio):
    print("%-58s largest error / bound = %.3g" % (name, ratio))


def device_fit(eng, sums, counts, min_count=4, masked=False, **clamps):
    fit = torch.full((8,), SENTINEL, device=eng.dev)
    curve = torch.full((3 * eng.fsc_len,), SENTINEL, device=eng.dev)
    eng.class_fsc_fit(sums, counts, fit, curve, min_count, masked=masked, **clamps)
    return host(eng, fit), host(eng, curve).reshape(3, -1)


# ---- 1. class averages

def test_class_averages_bit_for_bit(engines):
    """class_average_kernel: refs == (ev + od) * float32(1 / float32(cnt)), an add and then a multiply (nothing to fuse), bit for
    bit; classes below min_count keep the sentinel.  Counts straddle min_count: min_count - 1, min_count, 0, large"""
    for nx in SMALL_NX:
        eng = engines(nx, 4)
        s = halves(nx, 4, "signal", 5)
        for min_count, counts in ((4, (3, 4, 0, 100003)), (7, (7, 6, 16777217, 0)), (1, (0, 1, 3, 2))):
            refs = torch.full((4, nx, nx), SENTINEL, device=eng.dev)
            eng.class_averages(on(eng, s), on(eng, counts, np.int32), refs, min_count)
            got = host(eng, refs)
            want = class_average_ref(s, counts, min_count, np.full((4, nx, nx), SENTINEL, np.float32))
            assert np.array_equal(bits(got), bits(want)), (nx, counts)
            for j, c in enumerate(counts):
                assert np.all(got[j] == np.float32(SENTINEL)) == (c < min_count)


# ---- 2. per-class FSC

@pytest.mark.parametrize("masked", (False, True), ids=("plain", "masked"))
@pytest.mark.parametrize("nx", FSC_NX)
def test_per_class_fsc(engines, nx, masked):
    """fsc_kernel behind class_fsc + last_class_fsc on "signal" halves: points per shell equal the integer-exact count for every
    class, and every FSC value lies within the bound below of the float64 reference (masked: of the transform of the float32
    image (img - mean) * mask with mean = float32 of the float64 mean, which test_refine_cpu shows the device must form too).

    Bound.  The device transforms v in two passes of nx-term double sums with table twiddles: each coefficient is off by at most
    eps_F = 4 nx 2^-53 sum |v| (per pass (nx + 3) 2^-53 times an abs-sum of at most sum |v|, the two components combined).  With
    ret = sum Re(F conj G), n1 = sum |F|^2, n2 = sum |G|^2 over the cnt coefficients of a shell, to first order
        d ret <= eps_F(a) sum |G| + eps_F(b) sum |F| + (cnt + 4) 2^-53 sum |F| |G|      (carried in; the shell sum and its products)
        d n1  <= 2 eps_F(a) sum |F| + (cnt + 4) 2^-53 n1,    d n2 likewise
        d fsc <= d ret / sqrt(n1 n2) + |fsc| / 2 (d n1 / n1 + d n2 / n2) + 4 2^-53 |fsc|    (product, square root, division)
    plus 2^-24 for the rounding to float32.  A shell with no points or n1 n2 == 0 is exactly 0."""
    eng = engines(nx, FIT_NREF)
    s = halves(nx, FIT_NREF, "signal")
    counts = on(eng, [9] * FIT_NREF, np.int32)
    curve = eng.class_fsc(on(eng, s), counts, 4, masked=masked)
    per, pts = eng.last_class_fsc()
    ref = class_fsc_ref(s, circle_mask(nx) if masked else None)
    worst = 0.0
    for j, p in enumerate(ref):
        np.testing.assert_array_equal(pts[j], shell_points(nx))
        b = fsc_bound(p)
        err = np.abs(per[j].astype(np.float64) - p["val"])
        assert np.all(per[j][b == 0] == 0)
        worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    report("fsc nx=%d %s" % (nx, "masked" if masked else "plain"), worst)
    assert worst <= 1.0
    # the averaged curve of the host entry is the mean of exactly these curves, its axis i / (2 (nx // 2)) in float32
    want, last = averaged_curve(per, [9] * FIT_NREF, 4)
    assert np.array_equal(bits(curve[1]), bits(want)) and last == FIT_NREF - 1
    assert np.array_equal(bits(curve[0]), bits(freq_axis(nx)))
    np.testing.assert_array_equal(curve[2], shell_points(nx))


# ---- 3. live and dead classes

@pytest.mark.parametrize("nx", SMALL_NX)
def test_live_class_average(engines, nx):
    """counts (10, 3, 4, 0) with min_count 4: the average runs over classes 0 and 2, the last live class is 2, not nref - 1.
    The host entry (class_fsc) and the device entry (class_fsc_fit) restate this separately; both are held against the numpy
    restatement on the device's own per-class curves bit for bit, and those curves against the float64 reference.

    The points row is the last live class's by the code, but points per shell depend on the box alone (two per counted
    coefficient, whatever the data), so no input can tell one class's row from another's; what tells the classes apart is the
    curve: the dead classes hold FSC 1 (class 1) and noise (class 3), and in the "cancel" case the total is exactly 0 with class 0
    at +1 and class 2 at -1, so the fall-back curve must be class 2's -1 -- not class 0's, not a dead class's.
    "odd_zero": n2 == 0 in every shell of the live classes, every value 0, the total 0, the curve the last live class's zeros."""
    eng = engines(nx, 4)
    counts = on(eng, DEAD_COUNTS, np.int32)
    for variant in ("mixed", "odd_zero", "cancel"):
        s = dead_class_sums(nx, variant)
        ds = on(eng, s)
        curve = np.array(eng.class_fsc(ds, counts, DEAD_MIN_COUNT, masked=False), np.float32)
        per, pts = eng.last_class_fsc()
        ref = class_fsc_ref(s)
        worst = 0.0
        for j, p in enumerate(ref):
            b = fsc_bound(p)
            assert np.all(per[j][b == 0] == 0)
            if np.any(b > 0):
                worst = max(worst, float((np.abs(per[j] - p["val"])[b > 0] / b[b > 0]).max()))
            np.testing.assert_array_equal(pts[j], shell_points(nx))
        report("fsc nx=%d dead classes, %s" % (nx, variant), worst)
        assert worst <= 1.0
        want, last = averaged_curve(per, DEAD_COUNTS, DEAD_MIN_COUNT)
        assert last == 2
        assert np.array_equal(bits(curve[1]), bits(want)), variant
        assert np.array_equal(bits(curve[0]), bits(freq_axis(nx)))
        np.testing.assert_array_equal(curve[2], shell_points(nx))
        if variant == "mixed":        # a dead class in the average would move it by more than 0.05 (test_dead_class_cases)
            assert np.abs(curve[1] - np.mean([p["val"] for p in (ref[0], ref[2])], axis=0)).max() < 1e-6
        elif variant == "odd_zero":
            assert np.all(curve[1] == 0)
        else:
            assert np.all(per[0] == 1) and np.all(curve[1] == -1)
        # the device entry: the same curve as fit_tanh leaves it, the same axis and points
        f, c = device_fit(eng, ds, counts, DEAD_MIN_COUNT)
        frsc = [list(map(float, curve[0])), list(map(float, curve[1])), list(map(float, curve[2]))]
        fl, aa = api.fit_tanh(frsc)
        assert f[4] == 0.0
        assert np.array_equal(bits(c[0]), bits(curve[0])) and np.array_equal(bits(c[2]), bits(curve[2]))
        assert np.array_equal(bits(c[1]), bits(np.asarray(frsc[1], np.float32))), variant
        assert abs(f[2] - fl) < 2e-5 and abs(f[3] - aa) < 2e-5, (variant, f[:4], fl, aa)
    # every class dead: the host entry reports its state error, the device entry status 1 and the upper clamps
    dead = on(eng, (3, 3, 0, 1), np.int32)
    with pytest.raises(api.EngineError):
        eng.class_fsc(ds, dead, DEAD_MIN_COUNT, masked=False)
    f, c = device_fit(eng, ds, dead, DEAD_MIN_COUNT, fl_hi=0.37, aa_hi=0.11)
    assert f[4] == 1.0 and f[0] == np.float32(0.37) and f[1] == np.float32(0.11)


# ---- 4. the fit at the lane edges

@pytest.mark.parametrize("kind", FIT_KINDS)
@pytest.mark.parametrize("nx", FIT_NX)
def test_fit_at_the_lane_edges(engines, nx, kind):
    """fsc_fit_kernel at len = 17 (32, most lanes idle), 17 (33, odd), 64, 65, 128, 129 in each branch of the fit against the host
    pair class_fsc + api.fit_tanh: the curve as fit_tanh leaves it and the points row identical, (fl, aa) within the project's
    2e-5; the clamped pair exactly max(min(fl_hi, fl), fl_lo), min(aa, aa_hi) of the device's own fitted pair, with clamps that
    bite from below and from above; and the fitted pair against refine_oracle.fit_tanh within the host routine's tolerance
    (test_refine_cpu.test_host_fit_against_the_oracle) plus 2e-5"""
    eng = engines(nx, FIT_NREF)
    s, counts = fit_case(nx, kind)
    ds, dc = on(eng, s), on(eng, counts, np.int32)
    frsc = eng.class_fsc(ds, dc, 4, masked=False)
    if kind == "signal_negdc":
        assert frsc[1][0] == -1.0
    orc = [list(frsc[0]), list(frsc[1]), list(frsc[2])]
    fl, aa = api.fit_tanh(frsc)
    ofl, oaa = ro.fit_tanh(orc)
    fitted = None
    for clamps in (dict(fl_lo=0.3, fl_hi=0.45, aa_hi=0.05), dict(fl_lo=0.001, fl_hi=0.05, aa_hi=0.15)):
        f, c = device_fit(eng, ds, dc, 4, **clamps)
        assert f[4] == 0.0
        assert np.array_equal(bits(c[0]), bits(np.asarray(frsc[0], np.float32)))
        assert np.array_equal(bits(c[1]), bits(np.asarray(frsc[1], np.float32))), (nx, kind)
        assert np.array_equal(bits(c[2]), bits(np.asarray(frsc[2], np.float32)))
        print("fit nx=%d %-13s device (%.7f, %.7f) host (%.7f, %.7f) oracle (%.7f, %.7f)" % (nx, kind, f[2], f[3], fl, aa, ofl, oaa))
        assert abs(f[2] - fl) < 2e-5 and abs(f[3] - aa) < 2e-5, (f[:4], fl, aa)
        assert abs(f[2] - ofl) < HOST_FIT_TOL + 2e-5 and abs(f[3] - oaa) < HOST_FIT_TOL + 2e-5, (f[:4], ofl, oaa)
        lo, hi, ah = (np.float32(clamps[k]) for k in ("fl_lo", "fl_hi", "aa_hi"))
        assert f[0] == max(min(hi, f[2]), lo) and f[1] == min(f[3], ah)
        assert fitted is None or np.array_equal(bits(fitted), bits(f[2:4]))
        fitted = f[2:4].copy()
    if kind == "same":
        assert f[2] == np.float32(0.49) and f[3] == np.float32(0.1) and f[0] == np.float32(0.05) and f[1] == np.float32(0.1)
    if kind == "signal":          # both clamp sets bite: the first from below and on aa, the second from above
        assert 0.05 < f[2] < 0.3 and f[3] > 0.05


# ---- 5. filter, centre, shift

def filter_calls(eng, imgs):
    """every case of test_filter_centre_shift on the stack imgs [k][nx][nx] through filter_references and filter_references_dev
    (bitwise equal, centres included); returns {case: (images, centres)}"""
    k = imgs.shape[0]
    fl, aa = (float(np.float32(v)) for v in FILTER_FLAA)
    flaa = on(eng, FILTER_FLAA)
    shifts = filter_shifts(k)
    out = {}
    for name, hfl, dfl, center, cs in (("filter", fl, flaa, 0, None), ("round trip", 0.0, None, 0, None),
                                       ("shift", fl, flaa, -1, shifts), ("plain shift", 0.0, None, -1, shifts),
                                       ("centre", fl, flaa, 1, None)):
        x = on(eng, imgs)
        hcs = eng.filter_references(x, hfl, aa if hfl else 0.0, center=center, cs_in=cs, normalize=False)
        y = on(eng, imgs)
        dcs = torch.full((k, 2), SENTINEL, device=eng.dev)
        eng.filter_references_dev(y, dfl, center=center, cs_in=on(eng, cs) if cs is not None else None, normalize=False, cs_out=dcs)
        x, y, dcs = host(eng, x), host(eng, y), host(eng, dcs)
        assert np.array_equal(bits(x), bits(y)), name
        assert np.array_equal(bits(hcs), bits(dcs)), name
        out[name] = (x, hcs)
    return out


@pytest.mark.parametrize("nx", FILTER_NX)
def test_filter_centre_shift(nx):
    """filt_tanl, phase_cog, fshift and the inverse transform element by element, normalize = False, through filter_references and
    filter_references_dev, on a FRESH engine with 1, then 2 nref, then 2 nref + 3 images: the first call sizes the workspace for
    2 nref images, the third regrows it; the earlier images' results must not change when they are recomputed after the growth.

    Bound per pixel: |got - want| <= 2^-24 |want| + 16 nx 2^-53 sum |img|.  want is the float64 reference, rounded once to float32
    by the device (2^-24 |want|).  Each of the four passes is an nx-term double sum whose terms' abs-sum is at most sum |img| / nx^2
    per unit of output after the 1/nx^2 scale (|H| <= 1, the phase ramp has modulus 1, the half-spectrum weights 2 restore the
    full sum): 4 passes x (nx + 3) 2^-53, the two components of a complex coefficient combined, stay below 16 nx 2^-53 sum |img|.
    "round trip" (no filter, no centring) returns the input to the same bound: an even box has weight 1 on its Nyquist column,
    an odd box has no such column.  "plain shift" (center = -1, no filter) keeps the rows next to ky = nx / 2 at full weight: the
    filter of the other cases takes them to nothing, and with them the sign convention of ky at the even Nyquist row and the
    odd box's last positive row.
    Centres (center = 1): |c - ref| <= 2^-23 max(1, |c|) + nx / (2 pi) eps_F / |F|, eps_F = 4 nx 2^-53 sum |img| the error of the
    coefficient F = F[0][1] (x) or F[1][0] (y) as filtered, whose phase is read (an error eps in F turns the phase by at most
    eps / |F|), and 2^-23 for the rounding of the centre to float32 and the double arithmetic behind it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    eng = make_engine(nx, 2)
    try:
        imgs = filter_images(nx)
        assert FILTER_NIMG == 2 * eng.nref + 3
        runs = [filter_calls(eng, imgs[:k]) for k in (1, 2 * eng.nref, FILTER_NIMG)]
        for small in runs[:2]:
            for name, (x, cs) in small.items():
                k = x.shape[0]
                assert np.array_equal(bits(x), bits(runs[2][name][0][:k])), (name, k)
                assert np.array_equal(bits(cs), bits(runs[2][name][1][:k])), (name, k)
        got = runs[2]
        fl, aa = FILTER_FLAA
        shifts = filter_shifts(FILTER_NIMG)
        worst = dict.fromkeys(got, 0.0)
        worst_c = 0.0
        for i, img in enumerate(imgs):
            for name, rfl, center, cs in (("filter", fl, 0, None), ("round trip", 0.0, 0, None), ("shift", fl, -1, shifts[i]),
                                          ("plain shift", 0.0, -1, shifts[i]), ("centre", fl, 1, None)):
                want, c, a01, a10 = refine_ref(img, rfl, aa, center, cs)
                x, gcs = got[name]
                worst[name] = max(worst[name], float((np.abs(x[i] - want) / filter_bound(want, img)).max()))
                if center == 1:
                    for d, a in ((0, a01), (1, a10)):
                        worst_c = max(worst_c, abs(float(gcs[i, d]) - c[d]) / centre_bound(c[d], nx, img, a))
                elif center == -1:
                    assert np.array_equal(bits(gcs[i]), bits(shifts[i]))
                else:
                    assert np.all(gcs[i] == 0)
            # the pure round trip is the input
            assert np.all(np.abs(got["round trip"][0][i] - img) <= filter_bound(img.astype(np.float64), img))
        for name, w in worst.items():
            report("filter nx=%d %s" % (nx, name), w)
        report("filter nx=%d centres" % nx, worst_c)
        assert max(worst.values()) <= 1.0 and worst_c <= 1.0
    finally:
        eng.close()


def test_class_curves_survive_workspace_growth():
    """the per-class curves behind last_class_fsc are kept when a later filter call with more than 2 nref images regrows the
    workspace (they used to be reallocated with it and read back as zeros), and the FSC of the regrown workspace is the same bits"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nx = 33
    eng = make_engine(nx, FIT_NREF)
    try:
        s, counts = fit_case(nx, "signal")
        ds, dc = on(eng, s), on(eng, counts, np.int32)
        eng.class_fsc(ds, dc, 4, masked=True)
        per, pts = (a.copy() for a in eng.last_class_fsc())
        assert np.all(pts > 0) and np.all(per[:, :3] > 0.9)
        x = on(eng, filter_images(nx))
        eng.filter_references_dev(x, None, center=0, normalize=False)
        again = eng.last_class_fsc()
        assert np.array_equal(bits(again[0]), bits(per)) and np.array_equal(bits(again[1]), bits(pts))
        eng.class_fsc(ds, dc, 4, masked=True)
        again = eng.last_class_fsc()
        assert np.array_equal(bits(again[0]), bits(per)) and np.array_equal(bits(again[1]), bits(pts))
    finally:
        eng.close()


# ---- 6. normalize.mask

@pytest.mark.parametrize("nx", (32, 33, 131))
def test_normalize_mask(engines, nx):
    """normalize_mask_kernel on a known input: the centred, filtered call of test_filter_centre_shift with normalize = True against
    the float64 normalize.mask of the SAME call's normalize = False output, |got - want| <= 4 2^-24 (|v| + |mean|) / sigma per
    pixel (mean and v - mean rounded to float32, sigma rounded twice, one division), and against the kernel's arithmetic
    restated operation by operation in its summation order (normalize_kernel_steps), bit for bit.  update_refs_kernel is the same
    arithmetic on (even + odd) / count: update_references equals class_averages followed by that normalisation, bit for bit."""
    eng = engines(nx, FIT_NREF)
    imgs = filter_images(nx)[:2 * FIT_NREF]
    mask = circle_mask(nx)
    fl, aa = (float(np.float32(v)) for v in FILTER_FLAA)
    flaa = on(eng, FILTER_FLAA)
    plain, normed, normed_dev = on(eng, imgs), on(eng, imgs), on(eng, imgs)
    c0 = eng.filter_references(plain, fl, aa, center=1, normalize=False)
    c1 = eng.filter_references(normed, fl, aa, center=1, normalize=True)
    eng.filter_references_dev(normed_dev, flaa, center=1, normalize=True)
    plain, normed, normed_dev = host(eng, plain), host(eng, normed), host(eng, normed_dev)
    assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(normed), bits(normed_dev))
    worst = 0.0
    for v, got in zip(plain, normed):
        want, mean, sigma = normalize_mask_ref(v, mask)
        worst = max(worst, float((np.abs(got - want) / normalize_bound(v, mean, sigma)).max()))
        assert np.array_equal(bits(got), bits(normalize_kernel_steps(v, mask)))
    report("normalize.mask nx=%d" % nx, worst)
    assert worst <= 1.0
    s = halves(nx, FIT_NREF, "signal")
    counts = on(eng, (5, 1234), np.int32)
    avg = torch.full((FIT_NREF, nx, nx), SENTINEL, device=eng.dev)
    upd = torch.full((FIT_NREF, nx, nx), SENTINEL, device=eng.dev)
    eng.class_averages(on(eng, s), counts, avg, 4)
    eng.update_references(on(eng, s), counts, upd, 4)
    avg, upd = host(eng, avg), host(eng, upd)
    for j in range(FIT_NREF):
        assert np.array_equal(bits(upd[j]), bits(normalize_kernel_steps(avg[j], mask))), j


# ---- 7. state_from_params_dev

@pytest.mark.parametrize("mode", (api.RA_MODE_MREF, api.RA_MODE_REFFREE), ids=("mref", "reffree"))
def test_state_from_params_dev(engines, mode):
    """ra_state_from_params_dev gives the bits of ra_state_from_params with the same cs, in both engine modes, for n = 1, 255, 256,
    257 (blocks of 256), both mirror values, angles on and off the quadrant axes, cs zero and non-zero; and both equal
    geometry.inverse_transform2 / combine_params2 in float64 after rounding to float32 -- or lie one float32 ulp off where the
    float64 value is within 2^-45 (relative) of a rounding boundary, for at most 1 % of the entries (the CPU file shows that the
    parameters keep the reference inside that share)."""
    reffree = mode == api.RA_MODE_REFFREE
    eng = engines(32, 1 if reffree else 2, mode)
    off = total = 0
    for n in STATE_N:
        alpha, sx, sy, mirror = state_params(n)
        rec = np.zeros(n, api.RESULT_DTYPE)
        rec["alpha"], rec["sx"], rec["sy"], rec["mirror"] = alpha, sx, sy, mirror
        res = torch.from_numpy(rec.view(np.int32).reshape(n, 8).copy()).to(eng.dev)
        for cs in STATE_CS:
            a = torch.full((n + 2, 2), SENTINEL, device=eng.dev)
            b = torch.full((n + 2, 2), SENTINEL, device=eng.dev)
            eng.state_from_params(res, a[1:n + 1], cs)
            eng.state_from_params_dev(res, b[1:n + 1], on(eng, cs))
            a, b = host(eng, a), host(eng, b)
            assert np.array_equal(bits(a), bits(b)), (n, cs)
            assert np.all(a[0] == np.float32(SENTINEL)) and np.all(a[-1] == np.float32(SENTINEL))        # nothing outside [n][2]
            want = state_ref(alpha, sx, sy, mirror, cs, reffree)
            off += state_check(b[1:n + 1], want)
            total += want.size
    print("state_from_params_dev %s: %d of %d entries one ulp off at a rounding boundary" % ("reffree" if reffree else "mref", off, total))
    assert off <= 0.01 * total


# ---- 8. repeatability

@pytest.mark.parametrize("nx", (33, 130))
def test_repeatability(engines, nx):
    """the per-class table of class_fsc, the fit and curve of class_fsc_fit and the images and centres of filter_references_dev are
    the same bytes twice on one engine"""
    eng = engines(nx, FIT_NREF)
    s, counts = fit_case(nx, "signal")
    ds, dc = on(eng, s), on(eng, counts, np.int32)
    imgs = filter_images(nx)[:3]
    flaa = on(eng, FILTER_FLAA)
    outs = []
    for rep in range(2):
        eng.class_fsc(ds, dc, 4, masked=True)
        per, pts = eng.last_class_fsc()
        f, c = device_fit(eng, ds, dc, 4, masked=False)
        x = on(eng, imgs)
        cs = torch.full((3, 2), SENTINEL, device=eng.dev)
        eng.filter_references_dev(x, flaa, center=1, normalize=True, cs_out=cs)
        outs.append([per.copy(), pts.copy(), f[:5].copy(), c.copy(), host(eng, x), host(eng, cs)])
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b))
