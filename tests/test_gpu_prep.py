"""Particle preprocessing on the device (ra_prep_normalize / ra_prep_filter, cryo_ralib_amd/prep.py): entry by entry against the
float64 checker at the edges of the LDS plan, reproducibility and isolation, the C entries' refusals, the filter against the
engine's own tangent filter, the aligners' setup step, the tool, and the recovery of class assignments from a stack with
per-particle gain, plane and inverted contrast."""
import ctypes

import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, prep, stackio, synth
from cryo_ralib_amd.mref import MrefAligner, RefFreeAligner

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LDS_MAX = 201                      # the largest box whose image sits in LDS (csrc/ralign_prep.h pp_image_in_lds); 202 re-reads global


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def particles(nx, n, seed):
    """100 + 7 noise + a plane: the mean and the plane are large against the noise, so cancellation is real"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:nx, 0:nx] - nx // 2
    x = 100.0 + 7.0 * rng.standard_normal((n, nx, nx))
    x += rng.uniform(-0.5, 0.5, (n, 1, 1)) * u + rng.uniform(-0.5, 0.5, (n, 1, 1)) * v
    return x.astype(np.float32)


def normalize_dev(x, R, **kw):
    t, st = prep.normalize(dev(x), R, stats=True, **kw)
    return host(t), host(st)


# ---- N against the checker

WORST = {"stat": 0.0, "pixel": 0.0}


def check_normalize(x, R, ramp, invert):
    """statistics within max(1000 delta, 1e-12 scale), delta the checker's own discrepancy under the reversed summation order;
    pixels within 2^-23 |ref| + 1e-10 max|x| / sigma of float32(ref)"""
    n, nx = x.shape[0], x.shape[-1]
    got, st = normalize_dev(x, R, ramp=ramp, invert=invert)
    x64 = x.astype(np.float64)
    ref, rst = prep._normalize_numpy(x64, float(R), ramp, invert)
    _, rev = prep._normalize_numpy(x64, float(R), ramp, invert, order=-1)
    scale = float(np.abs(x).max())
    scales = np.array([scale, scale / (nx / 2.0), scale / (nx / 2.0), scale, scale])
    bar = np.maximum(1000.0 * np.abs(rst - rev).max(axis=0), 1e-12 * scales)
    err = np.abs(st - rst).max(axis=0)
    pix = np.abs(got.astype(np.float64) - ref.astype(np.float32)) - 2.0 ** -23 * np.abs(ref)
    pbar = 1e-10 * scale / rst[:, 4]
    WORST["stat"] = max(WORST["stat"], float((err / scales).max()))
    WORST["pixel"] = max(WORST["pixel"], float((pix.max(axis=(1, 2)) / pbar).max()))
    print("normalize nx=%d n=%d R=%g ramp=%d invert=%d: max stat err / scale %.3e (bar / scale %.3e), pixel excess over one ulp / "
          "absolute term %.3e; worst so far %.3e, %.3e" % (nx, n, R, ramp, invert, (err / scales).max(), (bar / scales).min(),
                                                           (pix.max(axis=(1, 2)) / pbar).max(), WORST["stat"], WORST["pixel"]))
    assert np.all(err <= bar), (err, bar)
    assert np.all(pix.max(axis=(1, 2)) <= pbar)


@pytest.mark.parametrize("nx", [4, 5, 63, 64, 65, 90, 129, LDS_MAX, LDS_MAX + 1, 256])
def test_normalize_matches_the_checker_entry_by_entry(nx):
    x = particles(nx, 3, nx)
    for R in (1.0, nx / 2.0, 0.5 + nx / 3.0 if nx > 5 else 1.75):
        for ramp, invert in ((False, False), (True, False), (False, True), (True, True)):
            check_normalize(x, R, ramp, invert)


@pytest.mark.parametrize("nx,n", [(5, 2100), (LDS_MAX, 300)])
def test_normalize_workgroups_that_loop_over_particles(nx, n):
    """more particles than the grid holds (2048 workgroups of a small box, 256 of the largest LDS-resident one)"""
    check_normalize(particles(nx, n, nx + 1), 0.4 * nx, True, False)


# ---- N properties

@pytest.mark.parametrize("nx", [90, LDS_MAX + 1])
def test_normalize_is_bitwise_reproducible(nx):
    x = particles(nx, 6, 3)
    kw = dict(ramp=True, invert=True)
    a, sa = normalize_dev(x, 30.0, **kw)
    b, sb = normalize_dev(x, 30.0, **kw)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(sa), bits(sb))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        c, sc = normalize_dev(x, 30.0, **kw)
    assert np.array_equal(bits(a), bits(c)) and np.array_equal(bits(sa), bits(sc))
    # the same particle at another place of a larger batch
    big = np.concatenate([particles(nx, 300, 4), x[::-1]])
    d, sd = normalize_dev(big, 30.0, **kw)
    assert np.array_equal(bits(d[300:][::-1]), bits(a)) and np.array_equal(bits(sd[300:][::-1]), bits(sa))


@pytest.mark.parametrize("nx", [64, LDS_MAX + 1])
def test_normalize_bad_and_constant_particles_stay_alone(nx):
    x = particles(nx, 7, 9)
    bad = x.copy()
    bad[1, nx // 2, nx // 2] = np.nan          # inside the disc: no sum over the background sees it
    bad[3] = 3.0                               # sigma == 0
    bad[5, 0, 0] = np.inf
    b, sb = normalize_dev(bad, 20.0)
    c, sc = normalize_dev(x, 20.0)
    keep = [0, 2, 4, 6]
    assert np.array_equal(bits(b[keep]), bits(c[keep])) and np.array_equal(bits(sb[keep]), bits(sc[keep]))
    for i in (1, 5):
        assert np.all(np.isnan(b[i])) and np.all(np.isnan(sb[i]))
    assert np.all(b[3] == 0.0) and sb[3, 4] == 0.0 and sb[3, 3] == 3.0


# ---- F

FILTERS = [(("tanl", 0.2, 0.1), None), (("gauss", 0.15), None), (("tanl", 0.3, 0.2), ("gauss", 0.03)), (None, ("tanl", 0.05, 0.5))]
# the boxes with kernels specialised for them (PF_FIXED_BOXES; 128, 130 and 256 at 2x keep their block in global scratch), two
# general boxes in LDS and one general box on the global-scratch route
BOXES = [(90, True), (90, False), (100, True), (128, True), (130, True), (256, True), (45, True), (64, False), (150, True)]


def filter_dev(x, lowpass, highpass, pad):
    return host(prep.fourier_filter(dev(x), lowpass, highpass, pad=pad))


@pytest.mark.parametrize("nx,pad", BOXES + [(45, False), (64, True)])
def test_filter_matches_the_checker(nx, pad):
    x = np.random.default_rng(nx).standard_normal((3, nx, nx)).astype(np.float32)
    for lowpass, highpass in FILTERS:
        got = filter_dev(x, lowpass, highpass, pad)
        ref = prep.fourier_filter(x, lowpass, highpass, pad=pad, backend="numpy")
        rel = max(np.abs(got[i] - ref[i]).max() / np.abs(ref[i]).max() for i in range(3))
        print("filter nx=%d pad=%d %r %r: max |gpu - checker| / max |checker| = %.3e" % (nx, pad, lowpass, highpass, rel))
        assert rel <= 1e-5


@pytest.mark.parametrize("nx", [64, 90])
def test_filter_matches_the_engines_tangent_filter(nx):
    """Engine.filter_references transforms in double: an independent implementation of the same profile, periodic as pad=False"""
    fl, aa = 0.25, 0.125
    x = np.random.default_rng(nx + 1).standard_normal((3, nx, nx)).astype(np.float32)
    eng = api.Engine(nx, nx // 2 - 8, 2, 2, 1.0, 3, api.RA_MODE_MREF)
    eng.use_current_stream()
    want = dev(x)
    eng.filter_references(want, fl, aa, center=0, normalize=False)
    eng.sync()
    want = host(want)
    eng.close()
    got = filter_dev(x, ("tanl", fl, aa), None, False)
    for i in range(3):
        assert np.abs(got[i] - want[i]).max() <= 1e-5 * np.abs(want[i]).max()


@pytest.mark.parametrize("nx,pad", [(90, True), (45, False), (150, True)])
def test_an_all_pass_filter_returns_the_input(nx, pad):
    x = np.random.default_rng(5).standard_normal((2, nx, nx)).astype(np.float32)
    assert np.all(prep.filter_multiplier(nx, 2 * nx if pad else nx, ("tanl", 0.999, 0.01)).astype(np.float32) == 1.0)
    got = filter_dev(x, ("tanl", 0.999, 0.01), None, pad)
    for i in range(2):
        assert np.abs(got[i] - x[i]).max() <= 1e-5 * np.abs(x[i]).max()


@pytest.mark.parametrize("nx,pad", [(90, True), (64, False), (150, True)])
def test_filter_is_bitwise_reproducible(nx, pad):
    x = np.random.default_rng(8).standard_normal((5, nx, nx)).astype(np.float32)
    lp, hp = FILTERS[2]
    a, b = filter_dev(x, lp, hp, pad), filter_dev(x, lp, hp, pad)
    assert np.array_equal(bits(a), bits(b))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        c = filter_dev(x, lp, hp, pad)
    assert np.array_equal(bits(a), bits(c))
    big = np.concatenate([np.random.default_rng(9).standard_normal((300, nx, nx)).astype(np.float32), x[::-1]])
    d = filter_dev(big, lp, hp, pad)
    assert np.array_equal(bits(d[300:][::-1]), bits(a))


# ---- the C entries

def test_c_entries_refuse_without_touching_the_images():
    L = api.load_library()
    x = torch.full((2, 32, 32), 7.0, device=DEV)
    st = torch.full((2, 5), 7.0, device=DEV, dtype=torch.float64)
    p, ps = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(st.data_ptr())
    nan, inf = float("nan"), float("inf")
    for n, nx, R, ramp, invert, ptr in [(-1, 32, 8.0, 0, 0, p), (2, 3, 1.0, 0, 0, p), (2, 1025, 8.0, 0, 0, p), (2, 32, 0.999, 0, 0, p),
                                        (2, 32, 16.001, 0, 0, p), (2, 32, nan, 0, 0, p), (2, 32, inf, 0, 0, p), (2, 32, 8.0, 2, 0, p),
                                        (2, 32, 8.0, 0, -1, p), (2, 32, 8.0, 1, 1, None)]:
        assert L.ra_prep_normalize(ptr, n, nx, R, ramp, invert, ps, None) == -1, (n, nx, R, ramp, invert)
        assert L.ra_last_error()
    good = (1, 0.2, 0.1, 2, 0.03, 0.0)
    for n, nx, pad, f, ptr in [(-1, 32, 0, good, p), (2, 1, 0, good, p), (2, 1025, 0, good, p), (2, 32, 2, good, p), (2, 32, 0, good, None),
                               (2, 32, 0, (0, 0.0, 0.0, 0, 0.0, 0.0), p), (2, 32, 0, (3, 0.2, 0.1, 0, 0.0, 0.0), p),
                               (2, 32, 0, (1, 0.0, 0.1, 0, 0.0, 0.0), p), (2, 32, 0, (1, 1.0, 0.1, 0, 0.0, 0.0), p),
                               (2, 32, 0, (1, 0.2, 0.0, 0, 0.0, 0.0), p), (2, 32, 0, (1, 0.2, nan, 0, 0.0, 0.0), p),
                               (2, 32, 0, (2, 0.0, 0.0, 0, 0.0, 0.0), p), (2, 32, 0, (2, inf, 0.0, 0, 0.0, 0.0), p),
                               (2, 32, 0, (0, 0.0, 0.0, 2, -1.0, 0.0), p), (2, 32, 0, (0, 0.0, 0.0, 1, 0.2, -0.1), p),
                               (2, 32, 0, (0, 0.0, 0.0, -1, 0.2, 0.1), p)]:
        assert L.ra_prep_filter(ptr, n, nx, pad, *f, None) == -1, (n, nx, pad, f)
    assert L.ra_prep_normalize(None, 0, 32, 8.0, 1, 0, None, None) == 0
    assert L.ra_prep_filter(None, 0, 32, 1, *good, None) == 0
    torch.cuda.synchronize()
    assert bool((x == 7).all()) and bool((st == 7).all())
    with pytest.raises(prep.PrepError):
        prep.normalize(x, 17.0)
    with pytest.raises(prep.PrepError):
        prep.fourier_filter(x)
    with pytest.raises(prep.PrepError):
        prep.normalize(x.double(), 8.0)
    assert bool((x == 7).all())


# ---- the aligners and the tool

def align_data(nx=64, ou=24, n=40, nref=3):
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, 2, 2, 0.5, ou=ou)
    return refs, (30.0 + 4.0 * parts).astype(np.float32), truth


def test_mref_aligner_normalises_at_setup_and_is_otherwise_unchanged():
    refs, parts, _ = align_data()
    R = 26.0
    a = MrefAligner(parts, refs, 24, 2, 2, 1.0, normalize_bg=R, normalize_ramp=True, invert=True)
    pre = host(prep.normalize(dev(parts), R, ramp=True, invert=True))
    b = MrefAligner(pre, refs, 24, 2, 2, 1.0)
    assert torch.equal(a.particles, b.particles)
    for _ in range(2):
        assert np.array_equal(a.iterate(), b.iterate())
        assert torch.equal(a.buf.sums, b.buf.sums) and torch.equal(a.refs, b.refs)
    a.engine.sync(); b.engine.sync()
    assert np.array_equal(a.params(), b.params())
    # invert alone multiplies by -1
    c = MrefAligner(parts, refs, 24, 2, 2, 1.0, invert=True)
    d = MrefAligner(-parts, refs, 24, 2, 2, 1.0)
    assert torch.equal(c.particles, d.particles)
    with pytest.raises(ValueError):
        MrefAligner(parts, refs, 24, 2, 2, 1.0, normalize_ramp=True)
    for al in (a, b, c, d):
        al.close()


def test_reffree_aligner_normalises_at_setup_and_is_otherwise_unchanged():
    _, parts, _ = align_data()
    R = 26.0
    a = RefFreeAligner(parts, 24, 2, 2, 1.0, normalize_bg=R, normalize_ramp=True, invert=True)
    pre = host(prep.normalize(dev(parts), R, ramp=True, invert=True))
    b = RefFreeAligner(pre, 24, 2, 2, 1.0)
    assert torch.equal(a.particles, b.particles)
    for _ in range(2):
        assert a.iterate() == b.iterate()
        assert torch.equal(a.buf.sums, b.buf.sums) and torch.equal(a.buf.counts_i, b.buf.counts_i)
    a.engine.sync(); b.engine.sync()
    assert np.array_equal(a.params(), b.params()) and torch.equal(a.tavg, b.tavg)
    a.close(); b.close()


def ctf_table(n, nx, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 9), np.float32)
    t[:] = [nx, 1.2, 0, 0, 0, 300.0, 2.7, 0.1, 0.0]
    t[:, 2] = rng.uniform(8000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(0, 3000, n)
    t[:, 4] = rng.uniform(-180, 180, n)
    return t


def test_tool_writes_what_the_api_computes(tmp_path):
    x = particles(90, 7, 5)
    tab = ctf_table(7, 90, 6)
    src, dst, sts, ctf = (str(tmp_path / f) for f in ("in.npy", "out.mrcs", "st.npy", "ctf.npy"))
    np.save(src, x)
    np.save(ctf, tab)
    # one step
    assert prep.main([src, dst, "--norm_bg", "40", "--ramp", "--stats", sts, "--batch", "3"]) == 0
    want, st = normalize_dev(x, 40.0, ramp=True)
    assert np.array_equal(stackio.read_stack(dst), want) and np.array_equal(np.load(sts), st)
    assert prep.main([src, dst, "--highpass_gauss", "100", "--res", "--apix", "1.5", "--filter_pad"]) == 0
    assert np.array_equal(stackio.read_stack(dst), filter_dev(x, None, ("gauss", 0.015), True))
    # the chain: normalise, phase flip, filter, resize
    assert prep.main([src, dst, "--norm_bg", "40", "--ctf", ctf, "--lowpass_tanl", "0.25", "0.1", "--box", "64", "--batch", "4"]) == 0
    t = prep.normalize(dev(x), 40.0)
    api.phase_flip(t, tab, pad=True)
    prep.fourier_filter(t, ("tanl", 0.25, 0.1))
    assert np.array_equal(stackio.read_stack(dst), host(api.fourier_resize(t, 64)))


# ---- use

def test_normalisation_recovers_the_assignments_of_the_clean_stack():
    """two classes; every particle with its own gain in [0.2, 5] and its own plane, and -- as a second case -- the whole stack
    inverted as well.  With normalize_bg + normalize_ramp (and invert for the inverted stack) the multi-reference assignments
    equal those of the clean stack on at least the share of particles that the clean stack assigns to its planted class"""
    nx, ou, n, nref = 64, 24, 80, 2
    refs = synth.make_references(nref, nx, ou, seed=77)
    clean, truth = synth.make_particles(refs, n, 1, 1, 0.3, ou=ou)
    rng = np.random.default_rng(2025)
    v, u = np.mgrid[0:nx, 0:nx] - nx // 2
    gain = rng.uniform(0.2, 5.0, (n, 1, 1))
    plane = rng.uniform(-0.2, 0.2, (n, 1, 1)) * u + rng.uniform(-0.2, 0.2, (n, 1, 1)) * v + rng.uniform(-20, 20, (n, 1, 1))
    bad = (gain * clean + plane).astype(np.float32)

    def assign(x, **kw):
        al = MrefAligner(x, refs, ou, 1, 1, 1.0, **kw)
        al.search()
        al.engine.sync()
        ids = al.params()["ref_id"].copy()
        al.close()
        return ids

    base = assign(clean)
    clean_share = float((base == truth["cls"]).mean())
    kw = dict(normalize_bg=ou + 2.0, normalize_ramp=True)
    shares = {"raw": float((assign(bad) == base).mean()),
              "normalised": float((assign(bad, **kw) == base).mean()),
              "inverted, normalised": float((assign(-bad, invert=True, **kw) == base).mean()),
              "inverted, raw": float((assign(-bad) == base).mean())}
    print("clean stack on its planted classes: %.3f; agreement with the clean assignments: %r" % (clean_share, shares))
    assert clean_share == 1.0
    assert shares["normalised"] >= clean_share and shares["inverted, normalised"] >= clean_share
