"""The CTF phase flip on the device (ra_phase_flip / api.phase_flip): the multiplier against the reference tree's CTF values,
the flip against the float64 statement of the contract (ctf.flip_reference), reproducibility, isolation of bad particles,
the aligners' setup flip, the effect on a multi-reference alignment, and the stand-alone tool."""
import os

import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, ctf, synth
from cryo_ralib_amd.mref import MrefAligner, RefFreeAligner

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctf_ref.npz")
DEV = torch.device("cuda", 0)


def table(n, nx, seed, binned=False):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 9), np.float32)
    t[:, 0] = nx * (2 if binned else 1)
    t[:, 1] = rng.uniform(0.9, 3.5, n) / (2 if binned else 1)
    t[:, 2] = rng.uniform(8000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(0, 3000, n)
    t[:, 4] = rng.uniform(-180, 180, n)
    t[:, 5] = rng.choice([200.0, 300.0], n)
    t[:, 6] = rng.uniform(0.01, 2.7, n)
    t[:, 7] = rng.uniform(0.0, 0.2, n)
    t[:, 8] = rng.choice([0.0, 25.0], n)
    return t


def flip(x, tab, pad=True):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    api.phase_flip(t, tab, pad)
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("k", range(8))
def test_multiplier_matches_the_reference_ctf_sign(k):
    z = np.load(GOLD)
    row, nx, gold = z["params_%d" % k].astype(np.float32), int(z["nx_%d" % k]), z["ctf_%d" % k]
    img = np.zeros((1, nx, nx), np.float32)
    img[0, 0, 0] = 1.0
    m = np.fft.rfft2(flip(img, row[None], pad=False)[0].astype(np.float64))
    g = gold[:, :nx // 2 + 1]
    sel = np.abs(g) > 1e-6
    if nx % 2 == 0:
        sel[:, nx // 2] = False          # Nyquist column of an even box: the real output keeps the Hermitian part of m only
    assert (np.sign(m.real[sel]) == -np.sign(g[sel])).all()
    assert np.abs(np.abs(m[sel]) - 1).max() < 1e-5


WORST = {}


# boxes next to a switch of the transform plan (pf_make_plan), with the padding for which the box is the edge.  2x: 90 | 91 two
# workgroups per CU -> one; 113 | 114 block in LDS (P = 226: a radix-113 stage) -> block in global scratch; 97: P = 2 x 97;
# 598 | 599 the global-scratch batch drops below its usual size; 1024 the largest box.  1x: 127 one radix-127 stage; 131 | 132 two
# workgroups per CU -> one; 171 | 172 block in LDS -> global scratch
PLAN_EDGES = [(n, True, nx) for n in (1, 5) for nx in (91, 113, 114, 97)] + \
             [(n, False, nx) for n in (1, 5) for nx in (127, 131, 132, 171, 172)] + [(2, True, 599), (2, True, 1024)]


@pytest.mark.parametrize("n,pad,nx", [(n, pad, nx) for n in (1, 5) for pad in (True, False) for nx in (32, 64, 90, 100, 128, 130, 256, 45)] +
                         PLAN_EDGES)
def test_flip_matches_the_float64_statement(nx, pad, n):
    rng = np.random.default_rng(nx * 10 + n)
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    tab = table(n, nx, nx + n, binned=(n == 5))
    got = flip(x, tab, pad)
    ref = ctf.flip_reference(x, tab, pad)
    rel = max(np.abs(got[i] - ref[i]).max() / np.abs(ref[i]).max() for i in range(n))
    WORST[(nx, pad, n)] = rel
    print("phase flip nx=%d pad=%d n=%d: max |gpu - oracle| / max |oracle| = %.3e (worst so far %.3e)"
          % (nx, pad, n, rel, max(WORST.values())))
    assert rel <= 1e-5


@pytest.mark.parametrize("nx", [130, 150])
def test_workgroups_that_loop_over_particles(nx):
    """the global-block route (130 x 130: the kernel specialised for the box; 150 x 150: the one taking the plan as an argument)
    runs fewer workgroups than particles, each reusing its scratch slice for particle p, p + grid, ...: n = 300 against the
    statement, and a NaN particle whose workgroup goes on to a good one leaves that one bitwise as without it"""
    n = 300
    rng = np.random.default_rng(nx)
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    tab = table(n, nx, nx + 1)
    got = flip(x, tab)
    ref = ctf.flip_reference(x, tab)
    rel = max(np.abs(got[i] - ref[i]).max() / np.abs(ref[i]).max() for i in range(n))
    print("phase flip nx=%d n=%d (looping workgroups): max rel err %.3e" % (nx, n, rel))
    assert rel <= 1e-5
    bad = x.copy()
    bad[3, 10, 10] = np.nan
    bad[4] = np.inf
    c = flip(bad, tab)
    keep = [i for i in range(n) if i not in (3, 4)]
    assert np.array_equal(c[keep].view(np.uint32), got[keep].view(np.uint32))


def test_unpadded_flip_twice_is_the_identity():
    """m^2 = 1 on an odd box (on an even one the Nyquist row / column keep only the Hermitian part of m, which may be 0)"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((6, 91, 91)).astype(np.float32)
    tab = table(6, 91, 8)
    y = flip(flip(x, tab, False), tab, False)
    assert np.abs(y - x).max() <= 1e-5 * np.abs(x).max()


def test_bitwise_reproducible_and_bad_particles_stay_alone():
    rng = np.random.default_rng(11)
    for nx in (90, 256):
        x = rng.standard_normal((9, nx, nx)).astype(np.float32)
        tab = table(9, nx, 12)
        a, b = flip(x, tab), flip(x, tab)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        bad = x.copy()
        bad[2, 5, 7] = np.nan
        bad[6] = np.inf
        c = flip(bad, tab)
        keep = [i for i in range(9) if i not in (2, 6)]
        assert np.array_equal(c[keep].view(np.uint32), a[keep].view(np.uint32))


def test_bad_parameters_are_refused_before_any_launch():
    x = torch.ones((3, 32, 32), device=DEV)
    good = table(3, 32, 1)
    for col, val in [(0, 0.0), (1, -1.0), (5, 0.0), (7, 1.0), (7, -0.5), (2, np.nan), (8, np.inf)]:
        t = good.copy()
        t[1, col] = val
        with pytest.raises(api.EngineError, match="row 1"):
            api.phase_flip(x, t)
    with pytest.raises(api.EngineError):
        api.phase_flip(x, good[:2])
    torch.cuda.synchronize()
    assert bool((x == 1).all())
    L = api.load_library()
    for nx, pad in ((1, 1), (2048, 0), (32, 2)):
        assert L.ra_phase_flip(api.ctypes.c_void_p(x.data_ptr()), 1, nx, good.ctypes.data_as(api.float_ptr), pad, None) == -1


def _align_data(nx=64, ou=24, n=40, nref=3):
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, 2, 2, 0.5, ou=ou)
    return refs, parts, truth, table(n, nx, 5)


def test_mref_aligner_flips_at_setup_and_is_otherwise_unchanged():
    refs, parts, _, tab = _align_data()
    a = MrefAligner(parts, refs, 24, 2, 2, 1.0, ctf=tab)
    # normalize_particles then the flip, bitwise
    b = MrefAligner(parts, refs, 24, 2, 2, 1.0)
    flipped = b.particles.clone()
    api.phase_flip(flipped, tab)
    torch.cuda.synchronize()
    assert torch.equal(a.particles, flipped)
    b.particles.copy_(flipped)
    for _ in range(2):
        ca, cb = a.iterate(), b.iterate()
        assert np.array_equal(ca, cb)
        assert torch.equal(a.buf.sums, b.buf.sums) and torch.equal(a.refs, b.refs)
    a.engine.sync(); b.engine.sync()
    assert np.array_equal(a.params(), b.params())
    # the CPU oracle on the same flipped images: one iteration agrees as in smoke()
    from oracle import oracle as orc
    ou, nx = 24, parts.shape[-1]
    rg = orc.rings(1, ou, 1)
    refs_n, cref = orc.prepare_refs(refs, orc.model_circle(ou, nx, nx), rg)
    c = MrefAligner(parts, refs, ou, 2, 2, 1.0, ctf=tab)
    fp = c.particles.cpu().numpy()
    params, _, _, counts = orc.mref_iteration(fp, cref, rg, 2, 2, 1.0, np.zeros((len(fp), 2), np.float32), nthreads=4)
    c.search()
    c.engine.sync()
    r = c.params()
    assert (r["ref_id"] == params[:, 4].astype(int)).all() and (r["mirror"] == params[:, 3].astype(int)).all()
    assert np.abs(r["peak"] - params[:, 5]).max() <= 1e-4 * np.abs(params[:, 5]).max()
    for al in (a, b, c):
        al.close()


def test_reffree_aligner_subtracts_the_mean_then_flips():
    _, parts, _, tab = _align_data()
    a = RefFreeAligner(parts, 24, 2, 2, 1.0, ctf=tab)                 # preprocess=False: the mean still goes first
    ref = torch.from_numpy(parts).to(DEV)
    b = RefFreeAligner(ref, 24, 2, 2, 1.0, preprocess=True)
    flipped = b.particles.clone()
    api.phase_flip(flipped, tab)
    torch.cuda.synchronize()
    assert torch.equal(a.particles, flipped)
    b.particles.copy_(flipped)
    for _ in range(2):
        assert a.iterate() == b.iterate()
        assert torch.equal(a.buf.sums, b.buf.sums) and torch.equal(a.buf.counts_i, b.buf.counts_i)
    a.engine.sync(); b.engine.sync()
    assert np.array_equal(a.params(), b.params()) and torch.equal(a.tavg, b.tavg)
    a.close(); b.close()


def _apply_ctf(parts, tab):
    """each particle convolved with its own CTF in a 2x padded image, in EMAN2's orientation (-ctf_np: positive before the first
    zero, so the first band keeps the references' contrast)"""
    n, nx = parts.shape[0], parts.shape[-1]
    out = np.empty_like(parts)
    P, o = 2 * nx, nx // 2
    for i in range(n):
        big = np.zeros((P, P))
        big[o:o + nx, o:o + nx] = parts[i]
        out[i] = np.fft.irfft2(np.fft.rfft2(big) * -ctf.ctf_grid(tab[i], nx, P), s=(P, P))[o:o + nx, o:o + nx]
    return out


def test_flip_recovers_class_assignments_of_ctf_modulated_particles():
    """4 classes, each particle convolved with its own CTF (defocus 1-3 um), noise; alignment against the CTF-free references
    assigns more particles to their true class with the flip than without it.  The CPU oracle on the same particles (flipped
    with the float64 statement) gives the bar the device must reach; with this seed it assigned 119 of 120 with the flip and
    76 without."""
    nx, ou, n, nref = 64, 26, 120, 4
    refs = synth.make_references(nref, nx, ou, seed=77)
    clean, truth = synth.make_particles(refs, n, 1, 1, 0.0, ou=ou)
    rng = np.random.default_rng(2024)
    tab = np.zeros((n, 9), np.float32)
    tab[:] = [nx, 1.0, 0, 0, 0, 300.0, 2.7, 0.1, 0.0]
    tab[:, 2] = rng.uniform(10000, 30000, n)
    tab[:, 3] = tab[:, 2] - rng.uniform(0, 1500, n)
    tab[:, 4] = rng.uniform(0, 180, n)
    noisy = (_apply_ctf(clean, tab) + rng.normal(0, 0.7 * clean.std(), clean.shape)).astype(np.float32)
    hits = {}
    for name, c in (("flip", tab), ("none", None)):
        al = MrefAligner(noisy, refs, ou, 1, 1, 1.0, ctf=c)
        al.search()
        al.engine.sync()
        hits[name] = int((al.params()["ref_id"] == truth["cls"]).sum())
        al.close()
    from oracle import oracle as orc
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    _, cref = orc.prepare_refs(refs, mask, rg)
    pre = noisy - np.array([p[mask > 0.5].mean() for p in noisy], np.float32)[:, None, None]
    fl = ctf.flip_reference(pre, tab).astype(np.float32)
    params, _, _, _ = orc.mref_iteration(fl, cref, rg, 1, 1, 1.0, np.zeros((n, 2), np.float32), nthreads=4)
    oracle_hits = int((params[:, 4].astype(int) == truth["cls"]).sum())
    print("true class: flip %d, no flip %d, CPU oracle with flip %d of %d" % (hits["flip"], hits["none"], oracle_hits, n))
    assert oracle_hits >= 115
    assert hits["flip"] >= oracle_hits - 2
    assert hits["flip"] >= hits["none"] + 30


def test_phaseflip_tool_writes_what_the_api_computes(tmp_path):
    from cryo_ralib_amd import phaseflip
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 90, 90)).astype(np.float32)
    tab = table(7, 90, 6)
    np.save(str(tmp_path / "in.npy"), x)
    np.save(str(tmp_path / "ctf.npy"), tab)
    for ext, extra, pad in (("npy", [], True), ("mrcs", ["--nopad"], False)):
        out = str(tmp_path / ("out." + ext))
        assert phaseflip.main([str(tmp_path / "in.npy"), out, "--ctf", str(tmp_path / "ctf.npy")] + extra) == 0
        from cryo_ralib_amd import stackio
        assert np.array_equal(stackio.read_stack(out), flip(x, tab, pad))
