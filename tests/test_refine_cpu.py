"""Float64 references and case builders for the reference-update kernels (csrc/ralign_refine.h), and the checks of both that
need no GPU.  tests/test_gpu_refine.py imports everything it compares the device with from here.

References.  Each one is written from the definition in the header comments of ralign_refine.h in float64 numpy (np.fft for the
transforms; test_inverse_transform_is_the_definition holds np.fft.irfft2 against the separable definition with its Nyquist
weight) and is held against oracle/refine_oracle.py at every box size used:
    fsc_parts             even/odd FSC per shell with the integer-exact shell table (shell_index)
    masked_input          (img - mean under the mask) * mask in float32, mean = float32 of the float64 mean
    tanl_values           tangent low-pass H on the half spectrum
    phase_cog_coeff       centre of gravity read off F[0][1], F[1][0]
    refine_ref            filter, centre (center = 1 | -1 | 0), phase ramp (fshift by -cs), inverse transform
    normalize_mask_ref    zero mean, unit sample sigma under the mask
    class_average_ref     (even + odd) * float32(1 / float32(count)), classes below min_count untouched
    state_ref             inverse_transform2 (after combine_params2 with -cs in the reference-free mode) of float32 parameters

Conditions the device tests rely on, asserted here:
    shells                (2r - 1)^2 <= 4 (kx^2 + ky^2) < (2r + 1)^2 in integers equals the float32 formulas of the oracle and of
                          fsc_shell_table coefficient for coefficient at all eight box sizes: points per shell are exact integers
    masked means          no float64 masked mean lies within 2^-40 (relative) of a float32 rounding boundary: the order of the
                          device's double sum cannot change the float32 mean, so the transformed image is known exactly
    fit branches          "signal" crosses 0.5 strictly inside the curve (ordinary simplex), "same" has FSC exactly 1 (never below
                          0.5: 0.49, 0.1), "uncorrelated" is below 0.5 at i = 1 (f0 = 0: the simplex starts at a[0] == 0),
                          "signal_negdc" has fsc[0] = -1 (flipped)
    host fit              ra_fit_tanh against refine_oracle.fit_tanh on the averaged curve of every fit case (test_host.py's 2e-5)
    state parameters      the share of entries whose float64 value lies within 2^-45 of a float32 rounding boundary is <= 1 %
"""
import functools
import itertools
import math
import os

import numpy as np
import pytest

from cryo_ralib_amd import geometry
from oracle import refine_oracle as ro

U24 = 2.0 ** -24
U53 = 2.0 ** -53

SMALL_NX = (32, 33)              # even / odd, most lanes of the fit idle
STRIDE_NX = (130, 131)           # nxh = 66 > 64 and nx > 128: the second trip of every thread-stride loop
FIT_EDGE_NX = (126, 128, 254, 256)   # len = 64, 65, 128, 129: one / two points per lane, the n > 128 branch
FSC_NX = SMALL_NX + FIT_EDGE_NX[:2] + STRIDE_NX + FIT_EDGE_NX[2:]
FILTER_NX = SMALL_NX + STRIDE_NX
FIT_NX = SMALL_NX + FIT_EDGE_NX
FIT_KINDS = ("signal", "same", "uncorrelated", "signal_negdc")
HOST_FIT_TOL = 2e-5              # test_host.test_fit_tanh_matches_the_python_restatement


def engine_geometry(nx):
    """(last ring, shift range) of the engines of the device tests: the largest ring ra_create accepts with a one-pixel search"""
    return (nx - 1) // 2 - 2, 1


def circle_mask(nx):
    """the engine's mask: geometry.model_circle(last ring) -- 1 inside the radius about (nx // 2, nx // 2), float32"""
    ou = engine_geometry(nx)[0]
    y, x = np.mgrid[0:nx, 0:nx]
    d2 = (x - nx // 2) ** 2 + (y - nx // 2) ** 2
    return (d2 <= ou * ou).astype(np.float32)


# ---- shells

def half_plane(nx):
    """signed ky [nx][1] and kx [1][nx/2+1] of the half spectrum (ky > nx/2 wraps to ky - nx: the even Nyquist row is +nx/2)"""
    ky = np.arange(nx, dtype=np.int64)
    return np.where(ky > nx // 2, ky - nx, ky)[:, None], np.arange(nx // 2 + 1, dtype=np.int64)[None, :]


@functools.lru_cache(maxsize=None)
def shell_index(nx):
    """shell of every half-spectrum coefficient in exact integer arithmetic, -1 where it is not counted (beyond nx/2; the
    kx = 0 column counts ky >= 0 only): the r with (2r - 1)^2 <= 4 (kx^2 + ky^2) < (2r + 1)^2, i.e. sqrt(kx^2 + ky^2) rounded to the
    nearest integer (4 k^2 is never an odd square, so there is no tie)"""
    kys, kx = half_plane(nx)
    s = 4 * (kx * kx + kys * kys)
    t = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    t -= (t * t > s)
    t += ((t + 1) * (t + 1) <= s)
    assert np.all(t * t <= s) and np.all((t + 1) * (t + 1) > s)
    r = (t + 1) // 2
    use = (r <= nx // 2) & ~((kx == 0) & (kys < 0))
    out = np.where(use, r, -1)
    out.setflags(write=False)
    return out


def shell_index_table_f32(nx):
    """the float32 arithmetic of fsc_shell_table, operation by operation"""
    f = np.float32
    inc = nx // 2
    kys, kx = half_plane(nx)
    d2 = f(1.0) / f(inc) / f(inc)
    argx = f(0.5) * np.sqrt((kys * kys).astype(f) * d2 + (kx * kx).astype(f) * d2)
    assert argx.dtype == np.float32
    rr = np.floor(f(inc) * f(2.0) * argx + f(0.5)).astype(np.int64)
    use = (rr <= inc) & ~((kx == 0) & (kys < 0))
    return np.where(use, rr, -1)


def shell_index_oracle_f32(nx):
    """the formula of refine_oracle.fsc (the argument rounded to float32 once, the rest in float64)"""
    inc = nx // 2
    kys, kx = half_plane(nx)
    ky = kys.astype(np.float64); kxf = kx.astype(np.float64)
    argx = 0.5 * np.sqrt(np.float32(ky * ky / (inc * inc) + kxf * kxf / (inc * inc)).astype(np.float64))
    r = np.floor(inc * 2 * argx + 0.5).astype(np.int64)
    use = (r <= inc) & ~((kx == 0) & (kys < 0))
    return np.where(use, r, -1)


def shell_points(nx):
    """points per shell as the kernels report them: 2 per counted coefficient"""
    sh = shell_index(nx)
    return 2.0 * np.bincount(sh[sh >= 0], minlength=nx // 2 + 1)


# ---- FSC

def masked_input(img, mask):
    """the image fsc_mask transforms: (img - mean) * mask in float32, mean = the float64 mean under the mask rounded to float32.
    Returns (v, float64 mean)."""
    m = mask > 0.5
    mean = float(img[m].astype(np.float64).sum() / int(m.sum()))
    return ((img - np.float32(mean)) * mask).astype(np.float32), mean


def f32_boundary_distance(x):
    """distance of the float64 x from the nearest float32 rounding boundary (the midpoints between neighbouring float32),
    relative to |x|"""
    r = np.float32(x)
    mids = [(float(r) + float(np.nextafter(r, np.float32(s)))) / 2.0 for s in (-np.inf, np.inf)]
    return min(abs(x - m) for m in mids) / abs(x)


def fsc_parts(a, b):
    """FSC of the images a, b as transformed (float32 or float64 [nx][nx]), float64 throughout.  Returns a dict: val [len] (0 where
    a shell has no points or n1 n2 == 0), cnt (coefficients per shell), ret, n1, n2 and the abs-sums the error bound needs"""
    nx = a.shape[0]
    n = nx // 2 + 1
    sh = shell_index(nx)
    use = sh >= 0
    idx = sh[use]
    F = np.fft.rfft2(a.astype(np.float64))[use]
    G = np.fft.rfft2(b.astype(np.float64))[use]
    aF, aG = np.abs(F), np.abs(G)
    p = {"cnt": np.bincount(idx, minlength=n).astype(np.float64),
         "ret": np.bincount(idx, F.real * G.real + F.imag * G.imag, n),
         "n1": np.bincount(idx, F.real ** 2 + F.imag ** 2, n), "n2": np.bincount(idx, G.real ** 2 + G.imag ** 2, n),
         "absF": np.bincount(idx, aF, n), "absG": np.bincount(idx, aG, n), "absFG": np.bincount(idx, aF * aG, n),
         "sum_a": float(np.abs(a.astype(np.float64)).sum()), "sum_b": float(np.abs(b.astype(np.float64)).sum()), "nx": nx}
    ok = (p["cnt"] > 0) & (p["n1"] > 0) & (p["n2"] > 0)
    den = np.sqrt(np.where(ok, p["n1"] * p["n2"], 1.0))
    p["ok"] = ok
    p["val"] = np.where(ok, p["ret"] / den, 0.0)
    return p


def fsc_bound(p):
    """entry-wise bound on |device fsc - val| (derivation: test_gpu_refine.test_per_class_fsc)"""
    nx = p["nx"]
    ea, eb = 4.0 * nx * U53 * p["sum_a"], 4.0 * nx * U53 * p["sum_b"]
    cu = (p["cnt"] + 4.0) * U53
    ok = p["ok"]
    n1, n2 = np.where(ok, p["n1"], 1.0), np.where(ok, p["n2"], 1.0)
    d_ret = ea * p["absG"] + eb * p["absF"] + cu * p["absFG"]
    d_n1 = 2.0 * ea * p["absF"] + cu * n1
    d_n2 = 2.0 * eb * p["absG"] + cu * n2
    b = d_ret / np.sqrt(n1 * n2) + 0.5 * np.abs(p["val"]) * (d_n1 / n1 + d_n2 / n2) + 4.0 * U53 * np.abs(p["val"]) + U24
    return np.where(ok, b, 0.0)


def class_fsc_ref(sums, mask=None):
    """fsc_parts of every class of sums [nref][2][nx][nx]; mask: fsc_mask"""
    out = []
    for ev, od in sums:
        if mask is not None:
            ev, od = masked_input(ev, mask)[0], masked_input(od, mask)[0]
        out.append(fsc_parts(ev, od))
    return out


def averaged_curve(per_class_f32, counts, min_count):
    """what ra_class_fsc / fsc_fit_kernel make of the per-class float32 curves [nref][len]: the mean over the live classes, summed
    in double in class order and rounded to float32 once -- or the last live class's curve if the grand total is 0.
    Returns (curve float32 [len], index of the last live class), or (None, -1) if no class is live"""
    live = [j for j in range(len(counts)) if counts[j] >= min_count]
    if not live:
        return None, -1
    a = np.zeros(per_class_f32.shape[1], np.float64)
    for j in live:
        a = a + per_class_f32[j].astype(np.float64)
    tot = 0.0
    for v in a:
        tot += v
    if tot != 0.0:
        return (a / len(live)).astype(np.float32), live[-1]
    return per_class_f32[live[-1]].astype(np.float32), live[-1]


def freq_axis(nx):
    return (np.arange(nx // 2 + 1, dtype=np.float64) / (2.0 * (nx // 2))).astype(np.float32)


def fit_branch(curve):
    """which way fit_tanh goes on a float32 curve: "ordinary" (f0 > 0), "f0=0", "never" (0.49, 0.1) or "tail" (0.5, 0.2)"""
    c = [float(v) for v in curve]
    n = len(c)
    for i in range(1, n):
        if 2 * c[i] / (1.0 + c[i]) < 0.1:
            c[i:] = [0.0] * (n - i)
            break
    for i in range(1, n - 1):
        if 2 * c[i] / (1.0 + c[i]) < 0.5:
            return "ordinary" if i > 1 else "f0=0"
    return "tail" if c[-1] < 0.5 else "never"


# ---- filter, centre, shift

def tanl_values(nx, fl, aa):
    """H = (tanh(c (d + fl)) - tanh(c (d - fl))) / 2 on the half spectrum, c = pi / (2 aa fl), d = |(kx, ky)| / nx; fl, aa are
    the float32 values the kernel is handed"""
    fl, aa = float(np.float32(fl)), float(np.float32(aa))
    kys, kx = half_plane(nx)
    d = np.sqrt((kx / float(nx)) ** 2 + (kys / float(nx)) ** 2)
    c = math.pi / (2.0 * aa * fl)
    return 0.5 * (np.tanh(c * (d + fl)) - np.tanh(c * (d - fl)))


def phase_cog_coeff(F, nx):
    """EMData::phase_cog from the half spectrum: the phase of conj(F[0][1]) (x) and conj(F[1][0]) (y) in [0, 2 pi) as a
    position, relative to the integer centre nx / 2"""
    P = 2.0 * math.pi / nx
    out = []
    for c in (F[0, 1], F[1, 0]):
        a = math.atan2(-c.imag, c.real)
        if a < 0.0:
            a += 2.0 * math.pi
        out.append(a / P - nx // 2)
    return out[0], out[1]


def phase_ramp(nx, cs):
    """fshift(img, -cs): F'(k) = F(k) e^{+2 pi i (kx csx + ky csy) / nx}"""
    kys, kx = half_plane(nx)
    return np.exp(2j * math.pi * (kx * float(cs[0]) + kys * float(cs[1])) / nx)


def idft_direct(F, nx):
    """the separable inverse of the header comments: U[y][kx] = sum_ky F[ky][kx] e^{+2 pi i ky y / nx}, then
    out[y][x] = 1/nx^2 sum_kx c_kx Re(U[y][kx] e^{+2 pi i kx x / nx}), c = 1 for kx = 0 and the even Nyquist, else 2"""
    y = np.arange(nx)
    U = np.exp(2j * math.pi * np.outer(y, y) / nx) @ F
    kx = np.arange(nx // 2 + 1)
    c = np.where((kx == 0) | (2 * kx == nx), 1.0, 2.0)
    E = np.exp(2j * math.pi * np.outer(kx, y) / nx)
    return ((U * c[None, :]) @ E).real / (nx * nx)


def refine_ref(img, fl, aa, center, cs_in=None):
    """filter_center_kernel between the forward and the inverse transform, float64.  fl = 0: no filter.  Returns (image float64,
    applied centre (x, y), |F[0][1]|, |F[1][0]| of the filtered spectrum)"""
    nx = img.shape[0]
    F = np.fft.rfft2(img.astype(np.float64))
    if fl > 0:
        F = F * tanl_values(nx, fl, aa)
    cs = (0.0, 0.0)
    if center == 1:
        cs = phase_cog_coeff(F, nx)
    elif center == -1:
        cs = (float(np.float32(cs_in[0])), float(np.float32(cs_in[1])))
    a01, a10 = abs(F[0, 1]), abs(F[1, 0])
    if center != 0 and (cs[0] != 0.0 or cs[1] != 0.0):
        F = F * phase_ramp(nx, cs)
    return np.fft.irfft2(F, s=(nx, nx)), cs, a01, a10


def filter_bound(want, img):
    """|got - want| <= 2^-24 |want| + 16 nx 2^-53 sum |img| (derivation: test_gpu_refine.test_filter_centre_shift)"""
    return U24 * np.abs(want) + 16.0 * img.shape[0] * U53 * float(np.abs(img.astype(np.float64)).sum())


def centre_bound(c, nx, img, a):
    """2^-23 max(1, |c|) + nx / (2 pi) eps_F / |F|, eps_F = 4 nx 2^-53 sum |img|, a = |F[0][1]| or |F[1][0]| as filtered"""
    return 2.0 ** -23 * max(1.0, abs(c)) + nx / (2.0 * math.pi) * 4.0 * nx * U53 * float(np.abs(img.astype(np.float64)).sum()) / a


def normalize_mask_ref(img, mask):
    """normalize.mask(no_sigma = 1) in float64.  Returns (image, mean, sigma)"""
    m = mask > 0.5
    v = img[m].astype(np.float64)
    n = v.size
    mean = v.sum() / n
    sigma = math.sqrt((np.sum(v * v) - v.sum() ** 2 / n) / (n - 1))
    return (img.astype(np.float64) - mean) / sigma, mean, sigma


def normalize_bound(img, mean, sigma):
    return 4.0 * U24 * (np.abs(img.astype(np.float64)) + abs(mean)) / sigma


def normalize_kernel_steps(img, mask):
    """normalize_mask_kernel / update_refs_kernel operation by operation: 256 threads stride over the pixels and sum v and v * v
    (exact in double for float32 v) under the mask in double, a 64-lane butterfly and the four waves in order; mean and sigma are
    rounded to float32 as the kernels do, the image is (v - mean) / sigma in float32 with IEEE division and square root"""
    f = np.float32
    v = img.astype(np.float32).ravel()
    m = mask.ravel() > 0.5
    npix = v.size
    rows = -(-npix // 256)
    vp = np.zeros(rows * 256, np.float64); vp[:npix] = np.where(m, v.astype(np.float64), 0.0)
    s = np.zeros(256); q = np.zeros(256)
    for row in vp.reshape(rows, 256):
        s = s + row
        q = q + row * row
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lane ^ o]
        q = q + q[lane ^ o]
    S = ((s[0] + s[64]) + s[128]) + s[192]
    Q = ((q[0] + q[64]) + q[128]) + q[192]
    nm = int(m.sum())
    mean = f(f(S) / f(nm))
    sigma = np.sqrt(f((Q - S * S / nm) / (nm - 1)))
    assert mean.dtype == np.float32 and sigma.dtype == np.float32
    return ((v - mean) / sigma).reshape(img.shape)


def class_average_ref(sums, counts, min_count, before):
    """class_average_kernel: (even + odd) * float32(1 / float32(count)) in float32, one add and one multiply (nothing to fuse);
    classes below min_count keep what `before` holds"""
    out = before.copy()
    for j, c in enumerate(counts):
        if c >= min_count:
            out[j] = (sums[j, 0] + sums[j, 1]) * np.float32(1.0 / float(np.float32(c)))
    return out


# ---- case builders

def blob(nx, cx, cy, sigma, amp=1.0):
    """periodic Gaussian of width sigma pixels centred at (cx, cy) (x = column, y = row), float64"""
    y, x = np.mgrid[0:nx, 0:nx].astype(np.float64)
    dx = (x - cx + nx / 2.0) % nx - nx / 2.0
    dy = (y - cy + nx / 2.0) % nx - nx / 2.0
    return amp * np.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma))


SIGNAL_SIGMA = 2.5           # pixels; with SNR 1e4 at DC the spectral SNR passes 1/2 (FSC 1/3, 2f/(1+f) = 1/2) near 0.2 / pixel
SIGNAL_SNR0 = 1.0e4


def signal_offset(j):
    """known off-centre placement (dx, dy) of class j's blob"""
    return 2.25 + j, -1.5 - 0.5 * j


def _signal(nx, nref, rng):
    out = np.zeros((nref, 2, nx, nx), np.float32)
    amp = math.sqrt(SIGNAL_SNR0) * nx / (2.0 * math.pi * SIGNAL_SIGMA ** 2)
    for j in range(nref):
        dx, dy = signal_offset(j)
        b = blob(nx, nx // 2 + dx, nx // 2 + dy, SIGNAL_SIGMA, amp)
        for h in range(2):
            out[j, h] = (b + rng.standard_normal((nx, nx))).astype(np.float32)
    return out


def _uncorrelated_ok(s):
    """builder condition of "uncorrelated": the averaged curve has fsc[0] > 0 and 2 f / (1 + f) < 0.5 at i = 1"""
    per = np.array([p["val"] for p in class_fsc_ref(s)]).astype(np.float32)
    c, _ = averaged_curve(per, [1] * len(s), 1)
    return c[0] > 0 and 2.0 * float(c[1]) / (1.0 + float(c[1])) < 0.5


@functools.lru_cache(maxsize=None)
def halves(nx, nref, kind, seed=0):
    """even / odd class sums [nref][2][nx][nx], float32 (read-only, cached)
    "signal"         a common Gaussian blob off-centre by signal_offset(class) plus independent unit white noise per half: the FSC
                     falls from 1 through 0.5 to 0 inside the curve, every shell keeps energy
    "same"           even == odd (the even half of "signal")
    "uncorrelated"   independent unit white noise only; shell 1 holds four coefficients, so the first seed from `seed` upwards
                     whose averaged curve is positive at 0 and below 2 f / (1 + f) = 0.5 at 1 is taken
    "signal_negdc"   "signal" with the mean term of every odd half negated: fsc[0] = -1"""
    if kind == "signal":
        s = _signal(nx, nref, np.random.default_rng([seed, nx, nref, 1]))
    elif kind == "same":
        s = _signal(nx, nref, np.random.default_rng([seed, nx, nref, 1]))
        s[:, 1] = s[:, 0]
    elif kind == "signal_negdc":
        s = _signal(nx, nref, np.random.default_rng([seed, nx, nref, 1]))
        for j in range(nref):
            s[j, 1] = (s[j, 1].astype(np.float64) - 2.0 * s[j, 1].astype(np.float64).mean()).astype(np.float32)
    elif kind == "uncorrelated":
        for t in itertools.count(seed):
            s = np.random.default_rng([t, nx, nref, 2]).standard_normal((nref, 2, nx, nx)).astype(np.float32)
            if _uncorrelated_ok(s):
                break
    else:
        raise ValueError(kind)
    s.setflags(write=False)
    return s


FIT_NREF = 2


def fit_case(nx, kind):
    """(sums, counts) of a fit case: FIT_NREF live classes"""
    return halves(nx, FIT_NREF, kind), np.full(FIT_NREF, 9, np.int32)


@functools.lru_cache(maxsize=None)
def fit_case_curve(nx, kind):
    """the averaged float32 curve of a fit case from the float64 reference"""
    s, counts = fit_case(nx, kind)
    per = np.array([p["val"] for p in class_fsc_ref(s)]).astype(np.float32)
    return averaged_curve(per, counts, 4)[0]


FIT_BRANCH = {"signal": "ordinary", "same": "never", "uncorrelated": "f0=0", "signal_negdc": "ordinary"}

# the live-class average (device test 3): classes 0 and 2 live, 1 (count below min_count) and 3 (empty) dead
DEAD_COUNTS = (10, 3, 4, 0)
DEAD_MIN_COUNT = 4


@functools.lru_cache(maxsize=None)
def dead_class_sums(nx, variant):
    """[4][2][nx][nx] for DEAD_COUNTS.  The dead classes hold curves unlike the live ones (1: even == odd, FSC 1; 3: noise).
    "mixed"      live classes are "signal" with different noise
    "odd_zero"   live classes have an all-zero odd half: n2 = 0 in every shell, every curve 0, the total 0
    "cancel"     class 0 has even == odd (FSC +1), class 2 has odd == -even (FSC -1): the total is exactly 0 and the curve falls
                 back to the LAST live class's, all -1 -- unlike class 0's and unlike the dead classes'"""
    s = np.array(halves(nx, 4, "signal", 5))
    s[1, 1] = s[1, 0]
    s[3] = np.random.default_rng([nx, 77]).standard_normal((2, nx, nx)).astype(np.float32)
    if variant == "odd_zero":
        s[0, 1] = 0.0; s[2, 1] = 0.0
    elif variant == "cancel":
        s[0, 1] = s[0, 0]; s[2, 1] = -s[2, 0]
    elif variant != "mixed":
        raise ValueError(variant)
    s.setflags(write=False)
    return s


FILTER_FLAA = (0.17, 0.15)
FILTER_NIMG = 2 * 2 + 3          # nref = 2: 1, then 2 nref, then 2 nref + 3 images on one engine


def cog_offsets(nx):
    """known centres of gravity (x, y) relative to nx // 2 of filter_images' first three images: up-left, down-right, and within
    a pixel of the wrap at -nx/2 in x"""
    return (-3.25, -2.5), (4.5, 1.75), (0.5 - nx // 2, 1.25)


@functools.lru_cache(maxsize=None)
def filter_images(nx):
    """[FILTER_NIMG][nx][nx] float32: three noise-free positive blobs at cog_offsets (a symmetric periodic blob's phase centre is
    its centre), then blobs with noise"""
    rng = np.random.default_rng([nx, 31])
    out = np.zeros((FILTER_NIMG, nx, nx), np.float32)
    for i, (dx, dy) in enumerate(cog_offsets(nx)):
        out[i] = blob(nx, nx // 2 + dx, nx // 2 + dy, 2.0 + 0.5 * i, 3.0 + i).astype(np.float32)
    for i in range(3, FILTER_NIMG):
        out[i] = (blob(nx, nx // 2 + 1.5 * (i - 4), nx // 2 - 0.75 * i, 3.0, 5.0) + rng.standard_normal((nx, nx))).astype(np.float32)
    out.setflags(write=False)
    return out


def filter_shifts(n):
    """per-image fractional shifts of both signs for center = -1"""
    base = np.array([[1.25, -0.5], [-2.75, 3.125], [0.3, 0.7], [-0.1, -4.6], [5.5, 0.0], [0.0, -1.5], [-7.2, 6.9]], np.float32)
    return np.ascontiguousarray(base[:n])


STATE_N = (1, 255, 256, 257)
STATE_CS = ((0.0, 0.0), (0.375, -1.625))


def state_params(n):
    """(alpha, sx, sy, mirror) float32 / int for n particles: both mirror values, angles on the quadrant axes (0, 90, 180, 270) and
    off them, integer, fractional and zero shifts"""
    rng = np.random.default_rng([n, 41])
    alpha = rng.uniform(0.0, 360.0, n).astype(np.float32)
    alpha[::5] = np.float32(90.0) * (np.arange(len(alpha[::5])) % 4)
    sx = (rng.integers(-12, 13, n) / 4.0).astype(np.float32)
    sy = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    sy[::7] = 0.0
    mirror = (np.arange(n) % 2).astype(np.int32) if n > 1 else np.ones(1, np.int32)
    return alpha, sx, sy, mirror


def state_ref(alpha, sx, sy, mirror, cs, reffree):
    """float64 [n][2]: inverse_transform2 of (alpha, sx, sy) -- in the reference-free mode of combine_params2(alpha, sx, sy, mirror,
    0, -cs) first (ali2d_single_iter); the multi-reference mode ignores mirror and cs"""
    out = np.zeros((len(alpha), 2))
    for i in range(len(alpha)):
        a, x, y = float(alpha[i]), float(sx[i]), float(sy[i])
        if reffree:
            a, x, y, _ = geometry.combine_params2(a, x, y, int(mirror[i]), 0.0, -float(np.float32(cs[0])), -float(np.float32(cs[1])), 0)
        _, ix, iy, _ = geometry.inverse_transform2(a, x, y, 0)
        out[i] = ix, iy
    return out


def near_f32_boundary(x, rel=2.0 ** -45):
    """mask of the float64 entries within rel (relative) of a float32 rounding boundary"""
    x = np.asarray(x, np.float64)
    r = x.astype(np.float32)
    out = np.zeros(x.shape, bool)
    for s in (-np.inf, np.inf):
        mid = (r.astype(np.float64) + np.nextafter(r, np.float32(s)).astype(np.float64)) / 2.0
        out |= np.abs(x - mid) <= rel * np.abs(x)
    return out & (x != 0)


def state_check(got, want64):
    """got float32 against the float64 reference: equal after rounding, or one float32 ulp off where the reference lies within
    2^-45 of a rounding boundary.  Returns the count of such entries; anything else fails"""
    w = want64.astype(np.float32)
    bad = got != w
    near = near_f32_boundary(want64)
    one_ulp = (got == np.nextafter(w, np.float32(np.inf))) | (got == np.nextafter(w, np.float32(-np.inf)))
    assert not np.any(bad & ~(near & one_ulp)), (got[bad & ~(near & one_ulp)][:5], w[bad & ~(near & one_ulp)][:5])
    return int(bad.sum())


# ---- the checks that need no GPU

@pytest.mark.parametrize("nx", FSC_NX)
def test_shells_are_unambiguous(nx):
    """the integer definition holds, and both float32 formulas give the same shell for every coefficient"""
    assert len(FSC_NX) == 8
    sh = shell_index(nx)
    kys, kx = half_plane(nx)
    s = 4 * (kx * kx + kys * kys) + 0 * sh
    r = np.where(sh >= 0, sh, 0)
    ok = ((r == 0) | ((2 * r - 1) ** 2 <= s)) & (s < (2 * r + 1) ** 2)        # r = 0: 2r - 1 < 0, no lower bound
    assert np.all(ok[sh >= 0])
    assert not np.any((sh[:, 0] >= 0) & (kys[:, 0] < 0)) and np.all(sh[kys[:, 0] >= 0, 0] >= 0)
    np.testing.assert_array_equal(shell_index_table_f32(nx), sh)
    np.testing.assert_array_equal(shell_index_oracle_f32(nx), sh)
    pts = shell_points(nx)
    assert pts[0] == 2 and np.all(pts > 0) and len(pts) == nx // 2 + 1


@pytest.mark.parametrize("nx", FSC_NX)
def test_fsc_reference_agrees_with_the_oracle(nx):
    s = halves(nx, 2, "signal")
    mask = circle_mask(nx)
    np.testing.assert_array_equal(mask, geometry.model_circle(engine_geometry(nx)[0], nx, nx))
    for j in range(2):
        for m in (None, mask):
            p = class_fsc_ref(s[j:j + 1], m)[0]
            o = ro.fsc(s[j, 0], s[j, 1]) if m is None else ro.fsc_mask(s[j, 0], s[j, 1], m)
            np.testing.assert_allclose(p["val"], o[1], rtol=0, atol=1e-12)
            np.testing.assert_array_equal(2 * p["cnt"], o[2])
            np.testing.assert_array_equal(2 * p["cnt"], shell_points(nx))
            np.testing.assert_allclose(freq_axis(nx), o[0], rtol=0, atol=2.0 ** -25)
            # (the masked shell 0 is the rounding residue of the mean: its bound is the widest)
            assert np.all(fsc_bound(p)[1:] < 1e-6) and fsc_bound(p)[0] < 1e-3 and np.all(fsc_bound(p) >= U24)


@pytest.mark.parametrize("nx", FSC_NX)
def test_masked_means_are_away_from_float32_boundaries(nx):
    mask = circle_mask(nx)
    for nref, kind, seed in ((FIT_NREF, "signal", 0), (4, "signal", 5)):
        if nref == 4 and nx not in SMALL_NX:
            continue
        for img in halves(nx, nref, kind, seed).reshape(-1, nx, nx):
            mean = masked_input(img, mask)[1]
            assert f32_boundary_distance(mean) > 2.0 ** -40, (nx, mean)


@pytest.mark.parametrize("nx", FILTER_NX)
def test_inverse_transform_is_the_definition(nx):
    """np.fft.irfft2 of a half spectrum that is not Hermitian in its kx = 0 and Nyquist columns (a fractional shift) equals the
    separable definition: the real part of those columns' row transform with weight 1 (even Nyquist) or no Nyquist at all (odd)"""
    img = filter_images(nx)[4]
    F = np.fft.rfft2(img.astype(np.float64)) * phase_ramp(nx, (1.3, -2.6))
    a, b = np.fft.irfft2(F, s=(nx, nx)), idft_direct(F, nx)
    assert np.abs(a - b).max() < 1e-12 * np.abs(a).max()
    if nx % 2 == 0:        # the weight matters: 2 on the Nyquist column is another image
        Fw = F.copy(); Fw[:, -1] *= 2.0
        assert np.abs(idft_direct(Fw, nx) - b).max() > 1e-6 * np.abs(b).max()


@pytest.mark.parametrize("nx", FILTER_NX)
def test_filter_centre_shift_references_agree_with_the_oracle(nx):
    fl, aa = FILTER_FLAA
    np.testing.assert_allclose(tanl_values(nx, fl, aa), ro.tanl_filter_values(nx, float(np.float32(fl)), float(np.float32(aa))),
                               rtol=0, atol=1e-15)
    imgs = filter_images(nx)
    for i in (0, 2, 5):
        img = imgs[i]
        scale = np.abs(img).max()
        t, _, _, _ = refine_ref(img, fl, aa, 0)
        o = ro.filt_tanl(img, float(np.float32(fl)), float(np.float32(aa)))
        assert np.abs(t - o).max() <= U24 * scale * 1.01
        c = phase_cog_coeff(np.fft.rfft2(img.astype(np.float64)), nx)
        oc = ro.phase_cog(img)
        assert abs(c[0] - oc[0]) < 1e-9 and abs(c[1] - oc[1]) < 1e-9
        sh = filter_shifts(FILTER_NIMG)[i]
        t, cs, _, _ = refine_ref(img, 0.0, 0.0, -1, sh)
        o = ro.fshift(img, -float(sh[0]), -float(sh[1]))
        assert cs == (float(sh[0]), float(sh[1])) and np.abs(t - o).max() <= U24 * scale * 1.01
    # the blobs' centres of gravity are the known ones, the third within a pixel of the wrap at -nx/2
    for i, (dx, dy) in enumerate(cog_offsets(nx)):
        _, cs, a01, a10 = refine_ref(imgs[i], fl, aa, 1)
        assert abs(cs[0] - dx) < 1e-5 and abs(cs[1] - dy) < 1e-5, (cs, dx, dy)
        assert centre_bound(cs[0], nx, imgs[i], a01) < 1e-5 and centre_bound(cs[1], nx, imgs[i], a10) < 1e-5
    assert -nx // 2 <= cog_offsets(nx)[2][0] < 1 - nx // 2 + 0.0 and cog_offsets(nx)[0][0] < 0 < cog_offsets(nx)[1][0]


@pytest.mark.parametrize("nx", (32, 33, 131))
def test_normalize_reference_agrees_with_the_oracle(nx):
    mask = circle_mask(nx)
    for img in filter_images(nx)[[0, 4]]:
        want, mean, sigma = normalize_mask_ref(img, mask)
        b = normalize_bound(img, mean, sigma)
        assert np.all(np.abs(ro.normalize_mask(img, mask) - want) <= b)
        assert np.all(np.abs(geometry.normalize_mask(img, mask, 1) - want) <= b)
        assert np.all(np.abs(normalize_kernel_steps(img, mask) - want) <= b)
        m = mask > 0.5
        assert abs(want[m].mean()) < 1e-12 and abs(want[m].std(ddof=1) - 1.0) < 1e-12


def test_class_average_reference():
    s = halves(32, 4, "signal", 5)
    before = np.full((4, 32, 32), -7.5, np.float32)
    out = class_average_ref(s, DEAD_COUNTS, DEAD_MIN_COUNT, before)
    assert np.all(out[1] == -7.5) and np.all(out[3] == -7.5)
    np.testing.assert_allclose(out[0], (s[0, 0].astype(np.float64) + s[0, 1]) / 10.0, rtol=3 * U24)
    np.testing.assert_array_equal(out[2], (s[2, 0] + s[2, 1]) * np.float32(0.25))


@pytest.mark.parametrize("nx", FIT_NX)
def test_fit_cases_reach_their_branches(nx):
    n = nx // 2 + 1
    for kind in FIT_KINDS:
        c = fit_case_curve(nx, kind)
        assert fit_branch(c) == FIT_BRANCH[kind], (nx, kind, fit_branch(c))
    c = fit_case_curve(nx, "signal").astype(np.float64)
    conv = 2 * c / (1 + c)
    below = np.nonzero(conv[1:] < 0.5)[0] + 1
    assert 1 < below[0] < n - 1, below[0]            # crosses 0.5 strictly inside the curve
    assert conv[1] > 0.9 and np.any(conv < 0.1)      # from near 1 to near 0
    np.testing.assert_array_equal(fit_case_curve(nx, "same"), np.ones(n, np.float32))     # exactly 1
    u = fit_case_curve(nx, "uncorrelated").astype(np.float64)
    assert u[0] > 0 and 2 * u[1] / (1 + u[1]) < 0.5
    assert fit_case_curve(nx, "signal_negdc")[0] == -1.0
    # the rest of the curve is "signal"'s (the odd halves are rounded to float32 again, nothing more)
    np.testing.assert_allclose(fit_case_curve(nx, "signal_negdc")[1:], fit_case_curve(nx, "signal")[1:], rtol=0, atol=1e-5)


@pytest.mark.parametrize("nx", SMALL_NX)
def test_dead_class_cases(nx):
    for variant, first in (("mixed", None), ("odd_zero", 0.0), ("cancel", -1.0)):
        s = dead_class_sums(nx, variant)
        per = np.array([p["val"] for p in class_fsc_ref(s)]).astype(np.float32)
        c, last = averaged_curve(per, DEAD_COUNTS, DEAD_MIN_COUNT)
        assert last == 2
        np.testing.assert_array_equal(per[1], np.ones_like(per[1]))          # the dead classes would show in the average
        assert np.abs(per[3][1:]).max() < 1.0 and np.abs(per[3] - per[2]).max() > 0.1
        if first is None:
            np.testing.assert_array_equal(c, ((per[0].astype(np.float64) + per[2]) / 2.0).astype(np.float32))
            assert np.abs(c - per.mean(0)).max() > 0.05 and np.abs(c - per[2]).max() > 1e-3
        else:
            np.testing.assert_array_equal(c, np.full_like(c, first))
            np.testing.assert_array_equal(c, per[2])
            if variant == "cancel":
                np.testing.assert_array_equal(per[0], -per[2])
    assert averaged_curve(per, (3, 3, 0, 0), DEAD_MIN_COUNT) == (None, -1)


def test_host_fit_against_the_oracle():
    """ra_fit_tanh against refine_oracle.fit_tanh on the averaged curve of every fit case, all branches; records nothing"""
    from cryo_ralib_amd import api
    if not os.path.exists(api.LIB_PATH):
        pytest.skip("the library is not built")
    for nx in FIT_NX:
        for kind in FIT_KINDS:
            c = fit_case_curve(nx, kind)
            a = [[float(v) for v in freq_axis(nx)], [float(v) for v in c], [float(v) for v in shell_points(nx)]]
            b = [list(a[0]), list(a[1]), list(a[2])]
            want = ro.fit_tanh(a)
            got = api.fit_tanh(b)
            assert abs(got[0] - want[0]) < HOST_FIT_TOL and abs(got[1] - want[1]) < HOST_FIT_TOL, (nx, kind, got, want)
            assert max(abs(x - y) for x, y in zip(a[1], b[1])) < 1e-7
            if kind == "same":
                assert got == (np.float32(0.49), np.float32(0.1))


def test_state_parameters_keep_the_reference_inside_the_ulp_allowance():
    total = near = 0
    for n in STATE_N:
        alpha, sx, sy, mirror = state_params(n)
        if n > 1:
            assert set(mirror) == {0, 1} and np.any(alpha % 90 == 0) and np.any(alpha % 90 != 0)
        for reffree in (False, True):
            for cs in STATE_CS:
                w = state_ref(alpha, sx, sy, mirror, cs, reffree)
                total += w.size
                near += int(near_f32_boundary(w).sum())
                assert state_check(w.astype(np.float32), w) == 0
    assert near <= 0.01 * total, (near, total)
    # the closed form behind inverse_transform2: t' = -R(alpha)^T t
    alpha, sx, sy, mirror = state_params(257)
    w = state_ref(alpha, sx, sy, mirror, (0.0, 0.0), False)
    a = np.radians(alpha.astype(np.float64))
    np.testing.assert_allclose(w[:, 0], -(np.cos(a) * sx - np.sin(a) * sy), atol=1e-13)
    np.testing.assert_allclose(w[:, 1], -(np.sin(a) * sx + np.cos(a) * sy), atol=1e-13)
