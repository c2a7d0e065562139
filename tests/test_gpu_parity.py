"""GPU parity tests: the HIP engine (through the C ABI) against the CPU oracle on the same
seeded inputs, against the committed golden fixtures, and -- at BASELINE.json's full size --
through size-independent properties.

Bars (BASELINE.json north_star): CCF peaks within 1e-4 relative; identical integer
(ref, mirror, angle-bin, shift) assignments -- literally: every oracle comparison asserts zero
disagreements (float near-ties, |dpeak|/peak < 3e-6, are decided by the engine in the CPU path's
arithmetic; the count of every comparison is logged in gpurun_out/parity_audit.json).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, geometry, synth
from cryo_ralib_amd.mref import MrefAligner, RefFreeAligner
from oracle import oracle as orc
from xsum_cases import xs_runs

pytestmark = pytest.mark.gpu

PEAK_RTOL = 1e-4        # north_star tolerance on CCF peaks
TIE_RTOL = 3e-6         # below this two candidates are indistinguishable in f32


def default_path_only(*switches):
    """tests that assert WHICH kernel path runs (or restate the default path's association of the class sums) are statements
    about the default selection: under a path switch of the whole-suite runs (RALIGN_FUSED=0, RALIGN_XSUM=0, RALIGN_TILED=0 ..)
    they are skipped, not failed, so that the remaining tests of that run are reached"""
    on = [sw for sw in (switches or ("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC")) if os.environ.get(sw) is not None]
    if on:
        pytest.skip("asserts the default kernel path; %s is set" % ", ".join(on))


def oracle_setup(refs, ou, nx):
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    refs_n, cref = orc.prepare_refs(refs, mask, rg)
    return rg, mask, refs_n, cref


def run_engine(parts, refs_n, ou, xr, yr, step, mode=api.RA_MODE_MREF, state=None, chunk=0, cs=None, prev=None):
    n, nx = parts.shape[0], parts.shape[-1]
    eng = api.Engine(nx, ou, xr, yr, step, refs_n.shape[0], mode, chunk=chunk)
    dev = eng.dev
    eng.set_references(torch.from_numpy(np.ascontiguousarray(refs_n)).to(dev))
    tp = torch.from_numpy(parts).to(dev)
    st = eng.new_state(n) if state is None else torch.from_numpy(state.copy()).to(dev)
    res = eng.new_result(n) if prev is None else prev
    eng.align(tp, st, res, cs)
    eng.sync()
    return eng, tp, st, res


def assert_images_close(got, want, mask, atol):
    """class sums / averages against the oracle's.  rot_shift2D's quadratic interpolant (quadri)
    is not continuous across pixel-cell borders and switches to the "background" copy where the
    source leaves the image, so a 1e-5 degree difference in the interpolated angle (prb1d on an
    f32 instead of an f64 peak neighbourhood) moves single pixels by O(noise sigma).  The bar is
    therefore: 99.9 % of the pixels under the mask within `atol`, and a relative L2 error
    below 2e-4 overall."""
    diff = np.abs(got - want)
    sel = np.broadcast_to(mask > 0.5, diff.shape)
    assert np.quantile(diff[sel], 0.999) < atol, np.quantile(diff[sel], 0.999)
    assert np.linalg.norm(diff[sel]) < 2e-4 * np.linalg.norm(want[sel]) + 1e-6


LAST_COMPARE = {}       # figures of the last compare_search call, copied into the audit log by _log_flips


def assert_alpha_equal_to_the_ulp(got, want):
    """every particle refined: the sub-bin angle is the oracle's float32, bit for bit -- up to two ulp (6e-5 degrees near 360) for
    the few particles where the last digits of the engine's own normalisation of particles and of its updated references
    (torch / device double arithmetic against the oracle's: images equal to 3e-6) reach the rounding of the result"""
    da = np.abs(((got.astype(np.float64) - want.astype(np.float64)) + 180.0) % 360.0 - 180.0)
    bad = np.where(got != want)[0]
    assert da.max() <= 6.2e-5, (da.max(), bad, got[bad], want[bad])
    assert (got == want).mean() >= 0.97, (got == want).mean()


def compare_search(r, st, params, infos, d, max_tie_frac=0.0, alpha_outlier_frac=0.0):
    """the bar of BASELINE.json's north_star, literally: identical integer (ref, mirror, angle bin, shift) assignments -- no
    allowance for float ties since round 5: the engine decides them in the CPU path's arithmetic (refine_winner_kernel), so a
    disagreement is a finding to fix there, not to admit here -- and CCF peaks within 1e-4"""
    n = len(r)
    jt = np.array([infos[i].jtot for i in range(n)])
    same = (r["ref_id"] == params[:, 4].astype(int)) & (r["mirror"] == params[:, 3].astype(int)) & \
           (r["angle_bin"] == jt) & (np.abs(st - d).max(1) < 1e-6)
    rel = np.abs(r["peak"] - params[:, 5]) / np.abs(params[:, 5])
    assert rel.max() < PEAK_RTOL, "CCF peak differs: %g" % rel.max()
    bad = np.where(~same)[0]
    # audit: a disagreement is admissible only when the two winners are a float tie
    for i in bad:
        assert rel[i] < TIE_RTOL, "particle %d: assignment differs and peaks are not tied (%g)" % (i, rel[i])
    assert len(bad) <= max(0, int(max_tie_frac * n)), "too many tie flips: %d of %d" % (len(bad), n)
    ok = same
    # Util::prb1d divides by c3 = 5 b1 - 3 b3 - 4 b4 - 3 b5 + 5 b7, which cancels to almost nothing on a flat peak (a blurred
    # reference): there the sub-bin position amplifies the f32-vs-f64 difference of the neighbourhood.  Such particles keep
    # the same integer bin; callers that expect flat peaks state how many of them may move by more than 2e-3 degrees.
    da = np.abs(((r["alpha"][ok] - params[ok, 0]) + 180.0) % 360.0 - 180.0)
    nout = int((da > 2e-3).sum())
    LAST_COMPARE.update(flips=len(bad), alpha_outliers=nout, max_alpha_diff_deg=float(da.max()) if da.size else 0.0,
                        max_rel_peak=float(rel.max()), n=n)
    assert nout <= int(alpha_outlier_frac * n), "sub-bin angle differs for %d of %d particles (max %g deg)" % (nout, n, da.max())
    if nout:
        print("sub-bin angle outliers (ill-conditioned prb1d): %d of %d, max %.3f deg" % (nout, n, da.max()))
    ok = ok.copy(); ok[np.where(ok)[0][da > 2e-3]] = False
    np.testing.assert_allclose(r["sx"][ok], params[ok, 1], atol=3e-4)     # |shift| * 2e-3 deg
    np.testing.assert_allclose(r["sy"][ok], params[ok, 2], atol=3e-4)
    return len(bad)


def test_prepared_references_match_applyws():
    nx, ou = 90, 36
    refs = synth.make_references(10, nx, ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    eng = api.Engine(nx, ou, 3, 3, 1.0, 10)
    eng.set_references(torch.from_numpy(refs_n).to(eng.dev))
    got = eng.prepared_references()
    assert got.shape == cref.shape == (10, 5816)
    assert np.abs(got - cref).max() < 1e-6 * np.abs(cref).max()
    eng.close()


@pytest.mark.parametrize("nx,ou,xr,mode", [(90, 36, 3, api.RA_MODE_MREF), (90, 36, 3, api.RA_MODE_REFFREE),
                                           (32, 12, 2, api.RA_MODE_MREF), (64, 25, 4, api.RA_MODE_MREF)])
def test_polar_ring_fft_stage_bin_for_bin(nx, ou, xr, mode):
    """first kernel alone: Polar2Dm -> (Normalize_ring) -> Frngs of every search offset, compared
    element by element with the oracle in EMAN2's packed ring layout."""
    polar_stage_check(nx, ou, xr, mode)


def polar_stage_check(nx, ou, xr, mode, n=3, rtol=1e-5):
    refs = synth.make_references(2, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg = orc.rings(1, ou, 1)
    eng = api.Engine(nx, ou, xr, xr, 1.0, 2 if mode == api.RA_MODE_MREF else 1, mode)
    st = np.zeros((n, 2), np.float32)
    st[1] = (1, -1)
    got = eng.debug_spectra(torch.from_numpy(parts).to(eng.dev), torch.from_numpy(st).to(eng.dev))
    sh = geometry.shift_list(xr, xr, 1.0)
    assert got.shape == (n, len(sh), rg.lcirc)
    cnx = nx // 2 + 1
    mashi = cnx - ou - 2
    for p in range(n):
        for s in range(len(sh)):
            # offsets outside the particle's window are masked later and may differ (zero border vs clamped taps)
            lo = geometry.search_range(nx, ou, st[p, 0], xr), geometry.search_range(nx, ou, st[p, 1], xr)
            if not (-lo[0][0] <= sh[s, 0] <= lo[0][1] and -lo[1][0] <= sh[s, 1] <= lo[1][1]):
                continue
            c = orc.polar2dm(parts[p], cnx + st[p, 0] + sh[s, 0], cnx + st[p, 1] + sh[s, 1], rg)
            if mode == api.RA_MODE_MREF:
                c = orc.normalize_ring(c, rg)
            want = orc.frngs(c, rg)
            assert np.abs(got[p, s] - want).max() < rtol * np.abs(want).max(), (p, s)
    assert mashi > 0
    eng.close()


@pytest.mark.parametrize("sigma,n", [(0.25, 256), (1.0, 256)])
def test_mref_search_headline_config(sigma, n):
    nx, ou, nref, xr = 90, 36, 10, 3
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, sigma, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=8)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    r = eng.result_to_numpy(res)
    flips = compare_search(r, st.cpu().numpy(), params, infos, d)
    if sigma == 0.25:
        assert flips == 0
        assert (r["ref_id"] == truth["cls"]).all() and (r["mirror"] == truth["mir"]).all()
    # transform + class sums
    gs = torch.zeros((nref, 2, nx, nx), device=eng.dev)
    gc = torch.zeros(nref, dtype=torch.int32, device=eng.dev)
    al = torch.zeros((n, nx, nx), device=eng.dev)
    eng.transform_accumulate(tp, res, 0, al, gs, gc)
    eng.sync()
    if flips == 0:
        np.testing.assert_array_equal(gc.cpu().numpy(), counts)
        assert_images_close(gs.cpu().numpy(), sums, mask, 2e-5 * np.abs(sums).max() + 1e-4)
    a = al.cpu().numpy()
    for i in range(0, n, 37):
        want = orc.rot_shift2d(parts[i], float(r["alpha"][i]), float(r["sx"][i]), float(r["sy"][i]), int(r["mirror"][i]))
        np.testing.assert_allclose(a[i], want, atol=1e-4)   # cosf vs (float)cos: 1 ulp in the rotation
    eng.close()


@pytest.mark.parametrize("name", ["mref_32.npz", "mref_90.npz"])
def test_golden_mref_two_iterations(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    ou, xr = int(g["ou"]), float(g["xr"])
    parts = g["particles"]
    n, nx = parts.shape[0], parts.shape[-1]
    nref = g["refs"].shape[0]
    eng = api.Engine(nx, ou, xr, xr, 1.0, nref)
    dev = eng.dev
    refs = torch.from_numpy(g["refs"]).to(dev)
    tp = torch.from_numpy(parts).to(dev)
    st, res = eng.new_state(n), eng.new_result(n)
    for it in range(2):
        eng.set_references(refs)
        eng.align(tp, st, res)
        gs = torch.zeros((nref, 2, nx, nx), device=dev)
        gc = torch.zeros(nref, dtype=torch.int32, device=dev)
        eng.transform_accumulate(tp, res, 0, None, gs, gc)
        eng.sync()
        r = eng.result_to_numpy(res)
        p = g["params%d" % it]
        np.testing.assert_array_equal(r["ref_id"], p[:, 4].astype(int))
        np.testing.assert_array_equal(r["mirror"], p[:, 3].astype(int))
        np.testing.assert_array_equal(r["angle_bin"], g["jtot%d" % it])
        np.testing.assert_allclose(st.cpu().numpy(), g["state%d" % it], atol=1e-6)
        assert (np.abs(r["peak"] - p[:, 5]) / np.abs(p[:, 5])).max() < PEAK_RTOL
        np.testing.assert_array_equal(gc.cpu().numpy(), g["counts%d" % it])
        assert np.abs(gs.cpu().numpy() - g["sums%d" % it]).max() < 1e-4
        if "newrefs%d" % it in g:
            eng.update_references(gs, gc, refs, 1)
            eng.sync()
            np.testing.assert_allclose(refs.cpu().numpy(), g["newrefs%d" % it], atol=2e-5)
    eng.close()


def test_golden_reffree_with_centre_correction(golden_dir):
    g = np.load(os.path.join(golden_dir, "reffree_32.npz"))
    ou, xr = int(g["ou"]), float(g["xr"])
    parts = g["particles"]
    n, nx = parts.shape[0], parts.shape[-1]
    eng = api.Engine(nx, ou, xr, xr, 1.0, 1, api.RA_MODE_REFFREE)
    dev = eng.dev
    eng.set_references(torch.from_numpy(g["tavg"]).to(dev))
    tp = torch.from_numpy(parts).to(dev)
    st, res = eng.new_state(n), eng.new_result(n)
    for it in range(2):
        cs = g["cs%d" % it]
        eng.align(tp, st, res, cs if cs.any() else None)
        eng.sync()
        r = eng.result_to_numpy(res)
        p = g["params%d" % it]
        np.testing.assert_array_equal(r["mirror"], p[:, 3].astype(int))
        np.testing.assert_array_equal(r["angle_bin"], g["jtot%d" % it])
        np.testing.assert_allclose(st.cpu().numpy(), g["state%d" % it], atol=2e-5)
        np.testing.assert_allclose(r["sx"], p[:, 1], atol=1e-4)
        np.testing.assert_allclose(r["sy"], p[:, 2], atol=1e-4)
        assert (np.abs(r["peak"] - p[:, 5]) / np.abs(p[:, 5])).max() < PEAK_RTOL
    eng.close()


@pytest.mark.parametrize("n,nref", [(1, 1), (7, 1), (5, 9), (33, 17), (64, 8)])
def test_ragged_sizes_and_reference_tiles(n, nref):
    nx, ou, xr = 32, 12, 2
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    eng.close()


def test_empty_batch_is_a_no_op():
    eng = api.Engine(32, 12, 2, 2, 1.0, 3)
    eng.set_references(torch.zeros((3, 32, 32), device=eng.dev))
    tp = torch.zeros((0, 32, 32), device=eng.dev)
    eng.align(tp, eng.new_state(0), eng.new_result(0))
    eng.transform_accumulate(tp, eng.new_result(0), 0, None, None, None)
    eng.sync()
    eng.close()


def test_edge_limited_windows_and_reset_rule():
    """accumulated offsets near mashi = cnx-ou-2 shrink the window asymmetrically (search_range);
    beyond mashi they are reset to zero (test_mref_gpu_align.py:1030-1038)."""
    nx, ou, nref, xr, n = 90, 36, 3, 3, 24
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    rng = np.random.default_rng(7)
    d0 = rng.integers(-10, 11, (n, 2)).astype(np.float32)
    d0[0] = (8, -8); d0[1] = (9, 0); d0[2] = (7, 7); d0[3] = (-6, 5)
    d = d0.copy()
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0, state=d0)
    compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    assert np.abs(d).max() <= 8 + 3
    eng.close()


@pytest.mark.parametrize("xr,yr,step", [(2, 1, 1.0), (1, 1, 0.5), (0, 0, 1.0), (3, 0, 1.0)])
def test_anisotropic_and_fractional_windows(xr, yr, step):
    nx, ou, nref, n = 32, 10, 3, 12
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, 1, 1, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, yr, step, d)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, yr, step)
    assert eng.num_shifts == (2 * int(xr / step) + 1) * (2 * int(yr / step) + 1)
    compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    eng.close()


# One geometry per launch path of the resident batch loop (ra_align, ra_align_classes) and of the chunked path.  Geometries by name are
# those of tests/test_gpu_dispatch.py::CASES and tests/test_gpu_plan_table.py::EXTRA; n and chunk give at least three launches and a
# ragged last one (the size-generic cases: n > chunk, one refine launch behind the last chunk).  family = (search_path, search_tiled,
# search_offsets_per_pass); ledger = a row only that path's engine has in its LDS ledger.
#   id,                   geometry,           environment,           n,  chunk, family,    maxrin, ledger
CHUNK_CASES = [
    # the case this test began with: prepared references, noise of sigma 1, and no family asserted (it runs under every path switch)
    ("box32-R4", ("box32", 32, 12, 1, 1, 2, 2, 1.0, 4, 0, api.RA_MODE_MREF, None), {}, 150, 32, None, None, None),
    ("fused-pack",         "R14",              {},                    16, 6, (1, 0, 0), 256,  "search_fused_kernel"),
    ("fused-pack-box93",   "box93-ou36",       {},                    16, 6, (1, 0, 0), 256,  "search_fused_kernel<pack>"),       # (R14 plans no pack kernel)
    ("fused-no-pack",      "R14",              {"RALIGN_PACK": "0"},  16, 6, (1, 0, 0), 256,  "search_fused_kernel"),
    ("fused-crop",         "box94-ou36",       {},                    16, 6, (1, 0, 0), 256,  "search_fused_kernel<pack> (crop)"),
    ("tiled",              "R15",              {},                    16, 6, (1, 1, 0), 256,  "search_tiled_kernel"),
    ("tiled-crop",         "R16-crop",         {},                    16, 6, (1, 1, 0), 256,  "search_tiled_kernel (crop)"),
    ("pair",               "box128-ou40-R8",   {},                    16, 6, (3, 0, 2), 256,  "search_pair_kernel"),
    ("duo",                "box100-ou41",      {},                    16, 6, (3, 0, 2), 512,  "search_duo_kernel"),
    ("solo",               "box100-ou41",      {"RALIGN_DUO": "0"},   16, 6, (3, 0, 1), 512,  "search_solo_kernel"),
    ("kernel-pair",        "R17-maxrin128",    {},                    16, 6, (0, 0, 0), 128,  "ccf_kernel"),
    ("generic",            "box140-ou61",      {},                    7,  2, (2, 0, 0), 512,  "ccf_generic_kernel<2, 2>"),
    ("generic-split",      "box200-ou88-R50",  {},                    7,  2, (2, 0, 0), 1024, "gccf_ifft_kernel<4, 7>"),
    ("class-resident",     ("classes", 64, 25, 1, 1, 2, 2, 1.0, 1, 0, api.RA_MODE_REFFREE, None), {}, 16, 6, (1, 0, 0), 256, "search_fused_kernel"),
]


@pytest.mark.parametrize("refine", [None, -1.0], ids=["refine-default", "refine-all"])
@pytest.mark.parametrize("case", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_chunking_is_invisible(case, refine, monkeypatch):
    """every kernel family: results and states of an engine that takes the call in one launch
    (chunk = 0) and of one that cuts it into batches are equal bit for bit, with the default refine threshold and with every
    particle on the refine list (which then grows past its create-time size)"""
    from test_gpu_plan_table import BY_NAME, SWITCHES
    cid, geom, env, n, chunk, family, maxrin, ledger = case
    if family:
        default_path_only(*SWITCHES)
    _, nx, ou, ir, rs, xr, yr, ts, nref, _, mode, _ = BY_NAME[geom] if isinstance(geom, str) else geom
    ncls = 3 if cid == "class-resident" else 0
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda:0")
    refs = synth.make_references(ncls or nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, yr, 0.5 if family else 1.0, ou=ou)
    if not family:
        refs = np.ascontiguousarray(oracle_setup(refs, ou, nx)[2])
    tp, tr = torch.from_numpy(parts).to(dev), torch.from_numpy(refs).to(dev)
    tc = (torch.arange(n, device=dev) % 3).to(torch.int32)
    out = []
    for ch in (0, chunk):
        eng = api.Engine(nx, ou, xr, yr, ts, nref, mode, first_ring=ir, ring_skip=rs, chunk=ch)
        if family:
            assert (eng.search_path, int(eng.search_tiled), eng.search_offsets_per_pass) == family and eng.maxrin == maxrin
            assert ledger in [r["kernel"] for r in eng.lds_report()]
        if refine is not None:
            eng.set_refine(refine)
        st, res = eng.new_state(n), eng.new_result(n)
        if ncls:
            eng.set_class_references(tr)
            eng.align_classes(tp, st, res, tc)
        else:
            eng.set_references(tr)
            eng.align(tp, st, res)
        eng.sync()
        if refine is not None:
            # (a resident launch starts the list anew; the chunked path collects the whole call in one list)
            assert eng.last_refine_count() == (n if ch == 0 or eng.search_path in (0, 2) else n - (n - 1) // ch * ch)
        out.append((res, st))
        eng.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_reset_shifts_shrinks_window():
    nx, ou, nref, n = 32, 12, 3, 10
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, 1, 1, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    eng = api.Engine(nx, ou, 2, 2, 1.0, nref)
    eng.set_references(torch.from_numpy(refs_n).to(eng.dev))
    eng.reset_shifts(1, 1, 1.0)
    assert eng.num_shifts == 9
    tp = torch.from_numpy(parts).to(eng.dev)
    st, res = eng.new_state(n), eng.new_result(n)
    eng.align(tp, st, res); eng.sync()
    d = np.zeros((n, 2), np.float32)
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, 1, 1, 1.0, d)
    compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    with pytest.raises(api.EngineError):
        eng.reset_shifts(3, 3, 1.0)      # more offsets than the engine was sized for
    eng.close()


def test_normalize_particles_and_update_references():
    nx, ou, nref = 90, 36, 5
    rng = np.random.default_rng(11)
    eng = api.Engine(nx, ou, 3, 3, 1.0, nref)
    mask = orc.model_circle(ou, nx, nx)
    imgs = rng.normal(3, 2, (6, nx, nx)).astype(np.float32)
    t = torch.from_numpy(imgs).to(eng.dev)
    eng.normalize_particles(t); eng.sync()
    for i in range(6):
        np.testing.assert_allclose(t[i].cpu().numpy(), orc.normalize_mask(imgs[i], mask, 0), atol=2e-6)
    sums = rng.normal(0, 5, (nref, 2, nx, nx)).astype(np.float32)
    counts = np.array([10, 3, 4, 100, 0], np.int32)
    refs0 = rng.normal(size=(nref, nx, nx)).astype(np.float32)
    refs = torch.from_numpy(refs0).to(eng.dev)
    eng.update_references(torch.from_numpy(sums).to(eng.dev), torch.from_numpy(counts).to(eng.dev), refs, 4)
    eng.sync()
    out = refs.cpu().numpy()
    for j in range(nref):
        if counts[j] < 4:          # vanished classes are left for the caller to re-seed
            np.testing.assert_array_equal(out[j], refs0[j])
        else:
            avg = (sums[j, 0] + sums[j, 1]) * np.float32(1.0 / float(counts[j]))
            np.testing.assert_allclose(out[j], orc.normalize_mask(avg, mask, 1), atol=2e-5)
    eng.close()


def test_reference_ctypes_surface_mref_align_run_m():
    """the reference's own call protocol (test_mref_gpu_align.py:373-449,
    test_mref_cheng_yu_bdb_cuda.py:546-556) through the drop-in symbols."""
    nx, ou, nref, xr, n = 90, 36, 4, 3, 40
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    lib = api.load_library()
    cfg = api.AlignConfig(n, nref, nx, ou, 256, 1.0, float(xr), float(xr))
    assert lib.pre_align_size_check(n, ctypes.byref(cfg), 0, 0.9, False) is True
    ptr = lib.pre_align_init(n, ctypes.byref(cfg), 0)
    prm = ctypes.cast(ptr, api.aln_param_ptr)
    lib.pre_align_fetch(api.get_c_ptr_array(list(parts)), n, b"sbj_batch")
    lib.reset_shifts(float(xr), 1.0)
    d = np.zeros((n, 2), np.float32)
    for it in range(2):
        lib.pre_align_fetch(api.get_c_ptr_array(list(refs_n)), nref, b"ref_batch")
        hs = lib.mref_align_run_m(0, n)
        params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d)
        got = np.ctypeslib.as_array(hs, shape=(2, nref, nx, nx))
        cnt = np.ctypeslib.as_array(lib.get_num_ref(), shape=(nref,))
        np.testing.assert_array_equal(cnt, counts)
        assert_images_close(got[0], sums[:, 0], mask, 2e-4)
        assert_images_close(got[1], sums[:, 1], mask, 2e-4)
        for k in range(n):
            assert prm[k].ref_id == int(params[k, 4]) and prm[k].mirror == bool(params[k, 3])
            assert prm[k].shift_x == d[k, 0] and prm[k].shift_y == d[k, 1]
        # the caller-side conversion of test_mref_gpu_align.py:578-588
        ang, sx, sy, m = geometry.alignparam_to_eman2([prm[k].angle for k in range(n)], [prm[k].shift_x for k in range(n)],
                                                      [prm[k].shift_y for k in range(n)], [prm[k].mirror for k in range(n)])
        np.testing.assert_allclose(sx, params[:, 1], atol=1e-4)
        np.testing.assert_allclose(sy, params[:, 2], atol=1e-4)
    # device-pointer returning variant: aligned images stay on the GPU
    dptr = lib.mref_align_run(0, n)
    assert dptr != 0
    lib.pre_align_fetch(api.get_c_ptr_array(list(refs_n)), nref, b"bogus")   # prints, returns (gpu_aln_noref.cu:373-376)
    lib.gpu_clear()


def test_reference_ctypes_surface_pre_align_run_m():
    nx, ou, xr, n = 32, 12, 2, 16
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg = orc.rings(1, ou, 1)
    tavg = parts.mean(0)[None].astype(np.float32)
    _, cref = orc.prepare_refs(tavg, None, rg)
    lib = api.load_library()
    cfg = api.AlignConfig(n, 1, nx, ou, 256, 1.0, float(xr), float(xr))
    prm = ctypes.cast(lib.pre_align_init(n, ctypes.byref(cfg), 0), api.aln_param_ptr)
    lib.pre_align_fetch(api.get_c_ptr_array(list(parts)), n, b"sbj_batch")
    lib.pre_align_fetch(api.get_c_ptr_array(list(tavg)), 1, b"ref_batch")
    assert lib.pre_align_run_m(0, n) != 0
    d = np.zeros((n, 2), np.float32); params = np.zeros((n, 6), np.float32)
    params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, xr, xr, 1.0, (0, 0), d, params)
    for k in range(n):
        assert prm[k].mirror == bool(params[k, 3]) and prm[k].shift_x == d[k, 0] and prm[k].shift_y == d[k, 1]
        assert prm[k].angle == pytest.approx(params[k, 0], abs=2e-3)
    lib.pre_align_run(0, n)
    lib.gpu_clear()


def _oracle_mref_loop_step(op, cur, rg, mask, xr, prev_params, d_exact, roundtrip):
    """one iteration of mref_ali2d from oracle calls: Polar2Dm/Frngs/Applyws of the current references, the state
    (round trip through the float32 header values, test_mref_gpu_align.py:1024-1026, or the exact carry), the search"""
    _, cref = orc.prepare_refs(cur, None, rg)
    d = orc.state_from_params(prev_params, 0) if (roundtrip and prev_params is not None) else d_exact.copy()
    params, infos, sums, counts = orc.mref_iteration(op, cref, rg, xr, xr, 1.0, d, nthreads=8)
    return params, infos, sums, counts, d


@pytest.mark.parametrize("roundtrip", [True, False], ids=["header-round-trip", "exact-carry"])
def test_iteration_loop_matches_oracle_loop(roundtrip):
    """four full iterations of the host driver (search, class sums, reference update) against the same loop built from
    oracle calls -- with the reference's state round trip (default) and with the exact carry.  A float tie in one
    iteration changes the class sums; the oracle is then re-seeded with the device's parameters and references and the
    comparison goes on (every iteration is checked, none is skipped)."""
    nx, ou, nref, xr, n = 90, 36, 4, 3, 96
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5)
    # refine = -1: the sub-bin angle of every particle is re-evaluated with the CPU path's arithmetic, so alpha / sx / sy equal
    # the oracle's to the last bit and the class sums differ only by the association of their additions
    al = MrefAligner(parts, refs, ou, xr, xr, 1.0, preprocess=True, state_roundtrip=roundtrip, refine=-1)
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    cur = np.stack([orc.normalize_mask(r, mask, 1) for r in refs])
    op = np.stack([orc.normalize_mask(p, mask, 0) for p in parts])
    np.testing.assert_allclose(al.particles.cpu().numpy(), op, atol=2e-6)
    d = np.zeros((n, 2), np.float32)
    prev = None
    reseeds = 0
    for it in range(4):
        params, infos, sums, counts, d = _oracle_mref_loop_step(op, cur, rg, mask, xr, prev, d, roundtrip)
        got_counts = al.iterate()
        r = al.params()
        flips = compare_search(r, al.state.cpu().numpy(), params, infos, d)
        _log_flips("mref loop %s it=%d" % ("round trip" if roundtrip else "exact carry", it), n, flips)
        if flips:
            # re-seed: continue from the device's parameters, state and references
            reseeds += 1
            prev = np.zeros((n, 6), np.float32)
            prev[:, 0] = r["alpha"]; prev[:, 1] = r["sx"]; prev[:, 2] = r["sy"]; prev[:, 3] = r["mirror"]
            d = al.state.cpu().numpy().copy()
            cur = al.refs.cpu().numpy().copy()
            continue
        prev = params
        np.testing.assert_array_equal(got_counts, counts)
        assert_alpha_equal_to_the_ulp(r["alpha"], params[:, 0])
        np.testing.assert_allclose(r["sx"], params[:, 1], rtol=0, atol=5e-7)       # one float32 ulp: the device's double sin / cos
        np.testing.assert_allclose(r["sy"], params[:, 2], rtol=0, atol=5e-7)       # against libm's in combine_params2
        cur = np.stack([orc.normalize_mask((sums[j, 0] + sums[j, 1]) * np.float32(1.0 / float(counts[j])), mask, 1)
                        for j in range(nref)])
        np.testing.assert_allclose(al.refs.cpu().numpy(), cur, rtol=0, atol=2e-6 * np.abs(cur).max())
    assert reseeds <= 1
    al.close()


def test_state_round_trip_matches_oracle():
    """ra_state_from_params against the oracle's restatement of inverse_transform2 / combine_params2 on random float32
    parameters, both modes: identical float32 shifts"""
    rng = np.random.default_rng(5)
    n = 4096
    prm = np.zeros((n, 6), np.float32)
    prm[:, 0] = rng.uniform(0, 360, n); prm[:, 1:3] = rng.normal(0, 4, (n, 2)); prm[:, 3] = rng.integers(0, 2, n)
    for mode, cs in ((api.RA_MODE_MREF, None), (api.RA_MODE_REFFREE, (0.37, -1.21)), (api.RA_MODE_REFFREE, None)):
        eng = api.Engine(32, 12, 2, 2, 1.0, 1 if mode == api.RA_MODE_REFFREE else 3, mode)
        res = eng.new_result(n)
        rec = np.zeros(n, api.RESULT_DTYPE)
        rec["alpha"] = prm[:, 0]; rec["sx"] = prm[:, 1]; rec["sy"] = prm[:, 2]; rec["mirror"] = prm[:, 3].astype(np.int32)
        res.copy_(torch.from_numpy(rec.view(np.int32).reshape(n, 8)))
        st = eng.new_state(n)
        eng.state_from_params(res, st, cs)
        eng.sync()
        want = orc.state_from_params(prm, 0 if mode == api.RA_MODE_MREF else 1, cs if cs else (0.0, 0.0))
        got = st.cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)          # device double sin / cos vs libm: last-bit noise only
        assert (got == want).mean() > 0.999
        eng.close()


def test_round_trip_decides_edge_limited_windows_like_the_oracle():
    """particles parked at |sxi| = mashi - k (k = 0, 1, 2): after one search the shift comes back through
    inverse_transform2 of float32 (alpha, sx, sy) as e.g. -6.9999995, and search_range -> int(range / step) or the
    |sxi| > mashi reset then differ from the exact carry.  Engine and oracle must take the same decisions, iteration
    after iteration (reference loop: test_mref_gpu_align.py:1024-1038)."""
    nx, ou, nref, xr, n = 90, 36, 3, 3, 192
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    mashi = nx // 2 + 1 - ou - 2
    d0 = np.zeros((n, 2), np.float32)
    rng = np.random.default_rng(11)
    d0[:, 0] = rng.choice([-1, 1], n) * (mashi - rng.integers(0, 3, n))
    d0[:, 1] = rng.choice([-1, 1], n) * (mashi - rng.integers(0, 3, n))
    eng = api.Engine(nx, ou, xr, xr, 1.0, nref, api.RA_MODE_MREF)
    eng.set_references(torch.from_numpy(refs_n).to(eng.dev))
    tp = torch.from_numpy(parts).to(eng.dev)
    st = torch.from_numpy(d0.copy()).to(eng.dev)
    res = eng.new_result(n)
    d = d0.copy()
    differs_from_exact = 0
    for it in range(4):
        if it > 0:
            eng.state_from_params(res, st)
            d_exact = d.copy()
            d = orc.state_from_params(params, 0)
            differs_from_exact += int((d != d_exact).any(1).sum())
            eng.sync()
            # identical up to the last bit of the DOUBLE sin / cos (device library vs libm): visible only where the shift
            # comes back as ~1e-8 instead of 0
            np.testing.assert_allclose(st.cpu().numpy(), d, rtol=0, atol=1e-12)
            d = st.cpu().numpy().copy()
        params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=8)
        eng.align(tp, st, res)
        eng.sync()
        r = eng.result_to_numpy(res)
        flips = compare_search(r, st.cpu().numpy(), params, infos, d)
        _log_flips("edge-parked round trip it=%d" % it, n, flips)
        assert flips == 0
        # keep the two loops on the same float32 parameters (a sub-bin angle may differ in the last digits)
        params[:, 0] = r["alpha"]; params[:, 1] = r["sx"]; params[:, 2] = r["sy"]
    assert differs_from_exact > 0          # the round trip really is not the exact carry on these particles
    eng.close()


def test_reffree_driver_runs_and_improves_criterion():
    nx, ou, xr, n = 32, 12, 2, 200
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    al = RefFreeAligner(parts, ou, xr, xr, 1.0)
    crit = [al.iterate() for _ in range(5)]
    assert crit[-1] > crit[0]       # sum_mask tavg^2 grows as the stack comes into register
    al.close()


def test_full_size_properties():
    """BASELINE configs[1] size (50 000 x 90x90, nref=10): linearity / conservation checks that
    do not need the oracle."""
    import bench
    nx, ou, nref, xr, n = 90, 36, 10, 3, 50000
    dev = torch.device("cuda", 0)
    refs = synth.make_references(nref, nx, ou)
    parts, truth = bench.generate_shard(dev, refs, n, xr, xr, 0.25, 0, nx, ou)
    al = MrefAligner(parts, refs, ou, xr, xr, 1.0, preprocess=True)
    al.search()
    al.engine.sync()
    r = al.params()
    assert int(al.buf.counts_i.sum().item()) == n
    np.testing.assert_array_equal(np.bincount(r["ref_id"], minlength=nref), al.buf.counts_i.cpu().numpy())
    # planted classes and mirrors are recovered at SNR ~ 16
    assert (r["ref_id"] == truth["cls"]).mean() > 0.999
    assert (r["mirror"] == truth["mir"]).mean() > 0.999
    # checksum of checksums: the class sums add up to the sum of all aligned images
    aligned = torch.zeros((8192, nx, nx), device=dev)
    total = torch.zeros((nx, nx), dtype=torch.float64, device=dev)
    for s in range(0, n, 8192):
        e = min(n, s + 8192)
        al.engine.transform_accumulate(al.particles[s:e], al.result[s:e].contiguous(), s, aligned[:e - s], None, None)
        total += aligned[:e - s].double().sum(0)
    got = al.buf.sums.double().sum((0, 1))
    assert (got - total).abs().max().item() < 1e-3 * total.abs().max().item()
    # even/odd split is by global index parity
    assert abs(float(al.buf.sums[:, 0].abs().sum() / al.buf.sums[:, 1].abs().sum()) - 1.0) < 0.2
    # idempotence: searching again from the converged offsets keeps every assignment
    ref_before = r["ref_id"].copy()
    al.engine.align(al.particles, al.state, al.result)
    al.engine.sync()
    r2 = al.params()
    assert (r2["ref_id"] == ref_before).mean() > 0.999
    assert np.abs(al.state.cpu().numpy()).max() <= 8 + xr
    al.close()


def test_command_line_entry_points(tmp_path):
    """the named entry points end to end (.mrcs inputs, EMAN2-MDF .hdf outputs like the reference): outputs exist,
    classes are recovered"""
    from cryo_ralib_amd import cli, stackio
    nx, ou, nref, xr, n = 32, 12, 3, 2, 120
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 0.25)
    stackio.write_stack(str(tmp_path / "stack.mrcs"), parts)
    stackio.write_stack(str(tmp_path / "refs.mrcs"), refs)
    out = tmp_path / "out"
    assert cli.main_mref([str(tmp_path / "stack.mrcs"), str(tmp_path / "refs.mrcs"), str(out), "--ou=12", "--xr=2",
                          "--yr=2", "--maxit=3", "--function=none"]) == 0
    rows = np.loadtxt(out / "params.txt")
    assert rows.shape == (n, 6) and (rows[:, 5].astype(int) == truth["cls"]).mean() > 0.98
    assert stackio.read_stack(str(out / "aqm002.hdf")).shape == (nref, nx, nx)
    # default --function=ref_ali2d --center=1: FSC-fitted tangent filter + centring of every average on the device
    out1 = tmp_path / "out1"
    assert cli.main_mref([str(tmp_path / "stack.mrcs"), str(tmp_path / "refs.mrcs"), str(out1), "--ou=12", "--xr=2",
                          "--yr=2", "--maxit=3"]) == 0
    rows1 = np.loadtxt(out1 / "params.txt")
    acc = (rows1[:, 5].astype(int) == truth["cls"]).mean()
    print("class recovery with ref_ali2d:", acc)
    assert rows1.shape == (n, 6) and acc > 0.8
    assert np.isfinite(stackio.read_stack(str(out1 / "aqm002.hdf"))).all()
    with pytest.raises(SystemExit):
        cli.main_mref([str(tmp_path / "stack.mrcs"), str(tmp_path / "refs.mrcs"), str(out1), "--function=my_func"])
    # the extension point: --function=file.py:callable gets the class averages, the reduced sums and the class sizes
    uf = tmp_path / "my_functions.py"
    uf.write_text("calls = []\ndef soften(refs, buf, counts):\n    calls.append((tuple(refs.shape), int(counts.sum())))\n"
                  "    return refs * 0.5\n")
    out4 = tmp_path / "out4"
    assert cli.main_mref([str(tmp_path / "stack.mrcs"), str(tmp_path / "refs.mrcs"), str(out4), "--ou=12", "--xr=2", "--yr=2",
                          "--maxit=2", "--function=%s:soften" % uf]) == 0
    import sys as _sys
    assert _sys.modules.get("ralign_user_function") is None or True
    rows4 = np.loadtxt(out4 / "params.txt")
    assert (rows4[:, 5].astype(int) == truth["cls"]).mean() > 0.98
    out2 = tmp_path / "out2"
    assert cli.main_reffree([str(tmp_path / "stack.mrcs"), str(out2), "--ou=12", "--xr=2", "--ts=1", "--maxit=3",
                             "--center=0"]) == 0
    assert np.loadtxt(out2 / "initial2Dparams.txt").shape == (n, 4)
    # per-iteration artefacts of the reference's drivers: aqc / aqf stacks (reference-free), FSC curves drm%03d%04d.txt and the
    # members of every class in the aqm headers (multi-reference with the default user function)
    assert stackio.read_stack(str(out2 / "aqf.hdf")).shape == (3, nx, nx) and stackio.read_stack(str(out2 / "aqc.hdf")).shape == (3, nx, nx)      # one image per iteration, the first included (:383)
    drm = np.loadtxt(out1 / "drm0020001.txt")
    assert drm.shape == (nx // 2 + 1, 3) and drm[0, 0] == 0.0 and abs(drm[-1, 0] - 0.5) < 1e-6 and np.abs(drm[:, 1]).max() <= 1.0 + 1e-5
    from cryo_ralib_amd import mdfio as _m
    _, hat = _m.read_mdf_stack(str(out1 / "aqm002.hdf"), with_attrs=True)
    mem = np.concatenate([np.atleast_1d(hat[j]["EMAN.members"]) for j in range(nref)])
    assert sorted(mem.tolist()) == list(range(n)) and sum(int(hat[j]["EMAN.n_objects"]) for j in range(nref)) == n
    assert all((rows1[np.atleast_1d(hat[j]["EMAN.members"]), 5] == j).all() for j in range(nref))
    # an .hdf input stack: the parameters go into the headers of a COPY under outdir by default, into the stack itself
    # only with --header_writeback
    from cryo_ralib_amd import mdfio
    hdf = str(tmp_path / "stack.hdf")
    mdfio.write_mdf_stack(hdf, parts, [{"source_n": np.int32(i)} for i in range(n)])
    before = open(hdf, "rb").read()
    out3 = tmp_path / "out3"
    assert cli.main_mref([hdf, str(tmp_path / "refs.mrcs"), str(out3), "--ou=12", "--xr=2", "--yr=2", "--maxit=2", "--function=none"]) == 0
    assert open(hdf, "rb").read() == before
    _, at = mdfio.read_mdf_stack(str(out3 / "stack.hdf"), with_attrs=True)
    rows3 = np.loadtxt(out3 / "params.txt")
    assert all(int(at[i]["EMAN.assign"]) == int(rows3[i, 5]) and int(at[i]["EMAN.source_n"]) == i for i in range(n))
    assert cli.main_mref([hdf, str(tmp_path / "refs.mrcs"), str(out3), "--ou=12", "--xr=2", "--yr=2", "--maxit=2", "--function=none",
                          "--header_writeback"]) == 0
    _, at = mdfio.read_mdf_stack(hdf, with_attrs=True)
    assert "EMAN.xform.align2d" in at[0] and int(at[5]["EMAN.source_n"]) == 5


@pytest.mark.parametrize("nx,ou,xr", [(90, 36, 3), (33, 12, 2), (64, 24, 3), (130, 52, 3),
                                      (200, 40, 3), (161, 45, 2), (256, 30, 4)])      # transform_sum_tile_kernel: even, odd, 16 full tiles
def test_class_sums_are_bitwise_reproducible(nx, ou, xr):
    """class sums are accumulated in a fixed order -- per batch and (class, parity) the member list is cut into `nrun`
    contiguous runs, each added in particle order (like Util.add_img on the CPU path) by one workgroup of
    transform_sum_kernel, the runs then added to the sums in run order -- so two runs agree bit for bit, and with a float32
    restatement of exactly that association on the aligned images of transform_kernel (the two kernels interpolate bit for
    bit alike: even and odd box sizes, mirrored and straight particles); the path that also returns the aligned images
    (class_sum_kernel, 16 runs per chunk) is pinned the same way"""
    default_path_only("RALIGN_XSUM", "RALIGN_XTILE")
    nref, n = 4, 300
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    outs = []
    for _ in range(2):
        eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0, chunk=128)
        gs = torch.zeros((nref, 2, nx, nx), device=eng.dev)
        gc = torch.zeros(nref, dtype=torch.int32, device=eng.dev)
        eng.transform_accumulate(tp, res, 3, None, gs, gc)
        eng.sync()
        outs.append((gs.cpu().numpy().copy(), gc.cpu().numpy().copy(), eng.result_to_numpy(res).copy()))
        eng.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    assert outs[0][1].sum() == n
    # and they equal that association applied to the engine's own aligned images in float32
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0, chunk=128)
    al = torch.zeros((n, nx, nx), device=eng.dev)
    gs2 = torch.zeros((nref, 2, nx, nx), device=eng.dev)
    gc2 = torch.zeros(nref, dtype=torch.int32, device=eng.dev)
    eng.transform_accumulate(tp, res, 3, al, gs2, gc2)          # aligned images AND sums: transform_kernel + class_sum_kernel
    eng.sync()
    a = al.cpu().numpy(); r = eng.result_to_numpy(res)
    np.testing.assert_array_equal(r["ref_id"], outs[0][2]["ref_id"])

    def restate(chunk, nrun_of):
        want = np.zeros((nref, 2, nx, nx), np.float32)
        for start in range(0, n, chunk):
            idx = np.arange(start, min(n, start + chunk))
            nrun = nrun_of(len(idx))
            for c in range(nref):
                for par in range(2):
                    mem = [i for i in idx if r["ref_id"][i] == c and (3 + i) % 2 == par]
                    if nrun > 1:
                        for run in range(nrun):
                            part = np.zeros((nx, nx), np.float32)
                            for i in mem[len(mem) * run // nrun:len(mem) * (run + 1) // nrun]:
                                part += a[i]
                            want[c, par] += part
                    else:
                        for i in mem:
                            want[c, par] += a[i]
        return want

    # transform_sum_kernel: one batch (n < 65536), runs from a zero partial sum even when there is one run only
    nrun = xs_runs(n, 2 * nref, nx)
    want = np.zeros((nref, 2, nx, nx), np.float32)
    for c in range(nref):
        for par in range(2):
            mem = [i for i in range(n) if r["ref_id"][i] == c and (3 + i) % 2 == par]
            for run in range(nrun):
                part = np.zeros((nx, nx), np.float32)
                for i in mem[len(mem) * run // nrun:len(mem) * (run + 1) // nrun]:
                    part += a[i]
                want[c, par] += part
    np.testing.assert_array_equal(outs[0][0], want)
    # class_sum_kernel: chunks of 128, 16 runs
    np.testing.assert_array_equal(gs2.cpu().numpy(), restate(128, lambda m: min(16, max(1, 4096 // (2 * nref * ((nx * nx + 255) // 256))))))
    np.testing.assert_array_equal(gc2.cpu().numpy(), outs[0][1])
    eng.close()


# ---------------------------------------------------------------------------------------------
# size-generic kernels (ralign_generic.h): large boxes, maxrin 512/1024, more than 48 rings

@pytest.mark.parametrize("mode", [api.RA_MODE_MREF, api.RA_MODE_REFFREE])
def test_generic_polar_stage_bin_for_bin_on_small_box(monkeypatch, mode):
    """the generic polar / ring-FFT kernel forced onto a geometry the specialised kernel also covers"""
    monkeypatch.setenv("RALIGN_GENERIC", "1")
    polar_stage_check(64, 25, 3, mode)


def test_generic_search_equals_specialised_search(monkeypatch):
    """same inputs through both kernel families: identical integer assignments, peaks within f32 noise"""
    nx, ou, nref, xr, n = 90, 36, 10, 3, 96
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    fast = api.Engine.result_to_numpy(res).copy()
    eng.close()
    monkeypatch.setenv("RALIGN_GENERIC", "1")
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    gen = api.Engine.result_to_numpy(res).copy()
    eng.close()
    for f in ("ref_id", "mirror", "angle_bin", "shift_idx"):
        assert (fast[f] == gen[f]).all(), f
    assert (np.abs(fast["peak"] - gen["peak"]) / np.abs(fast["peak"])).max() < 1e-5
    d = np.zeros((n, 2), np.float32)
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=8)
    compare_search(gen, st.cpu().numpy(), params, infos, d)


@pytest.mark.parametrize("nx,ou,xr,nref,n", [(256, 120, 5, 3, 6),      # BASELINE configs[4] geometry: maxrin 1024, 120 rings
                                              (160, 70, 3, 9, 5),       # maxrin 512, two reference tiles (5 + 4)
                                              (128, 50, 4, 2, 6)])      # maxrin 512, 50 rings
def test_large_box_search_transform_and_sums(nx, ou, xr, nref, n):
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.25, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    assert rg.maxrin >= 512
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=8)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    got = eng.prepared_references()
    assert np.abs(got - cref).max() < 1e-6 * np.abs(cref).max()
    r = api.Engine.result_to_numpy(res)
    compare_search(r, st.cpu().numpy(), params, infos, d)
    gs = torch.zeros((nref, 2, nx, nx), device=eng.dev)
    gc = torch.zeros(nref, dtype=torch.int32, device=eng.dev)
    eng.transform_accumulate(tp, res, 0, None, gs, gc)
    eng.sync()
    assert (gc.cpu().numpy() == counts).all()
    assert_images_close(gs.cpu().numpy(), sums, mask, 2e-5 * np.abs(sums).max() + 1e-4)
    eng.close()


def test_large_box_polar_stage_bin_for_bin():
    polar_stage_check(128, 50, 2, api.RA_MODE_MREF, n=2, rtol=2e-5)


# ---------------------------------------------------------------------------------------------
# reference update on the device against oracle/refine_oracle.py

def _searched_aligner(nx=90, ou=36, nref=5, xr=3, n=400, sigma=1.0):
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, sigma, ou=ou)
    al = MrefAligner(parts, refs, ou, xr, xr, 1.0, preprocess=True)
    al.search()
    al.buf.all_reduce()
    return al


def test_class_fsc_and_tangent_filter_against_oracle():
    from oracle import refine_oracle as ro
    al = _searched_aligner()
    sums = al.buf.sums.cpu().numpy()
    counts = al.buf.counts_i.cpu().numpy()
    mask = geometry.model_circle(al.ou, al.nx, al.nx)
    assert (counts >= 4).all()
    # fsc per class, averaged over the classes (test_mref_gpu_align.py:531-548)
    got = al.engine.class_fsc(al.buf.sums, al.buf.counts_i, 4, masked=False)
    per = [ro.fsc(sums[j, 0], sums[j, 1]) for j in range(al.nref)]
    want = np.mean([p[1] for p in per], axis=0)
    np.testing.assert_allclose(got[0], per[0][0], atol=1e-7)
    np.testing.assert_allclose(got[1], want, atol=2e-5)
    np.testing.assert_allclose(got[2], per[-1][2], atol=0)
    # fsc_mask (test_reffree_gpu_align.py:384)
    gotm = al.engine.class_fsc(al.buf.sums, al.buf.counts_i, 4, masked=True)
    wantm = np.mean([ro.fsc_mask(sums[j, 0], sums[j, 1], mask)[1] for j in range(al.nref)], axis=0)
    np.testing.assert_allclose(gotm[1], wantm, atol=2e-5)
    # class averages, tangent filter, phase_cog centring, normalize.mask
    avg = torch.zeros_like(al.refs)
    al.engine.class_averages(al.buf.sums, al.buf.counts_i, avg, 4)
    a = avg.cpu().numpy()
    for j in range(al.nref):
        np.testing.assert_allclose(a[j], (sums[j, 0] + sums[j, 1]) * np.float32(1.0 / counts[j]), rtol=0, atol=1e-6)
    for center in (0, 1):
        x = avg.clone()
        cs = al.engine.filter_references(x, 0.17, 0.15, center=center, normalize=True)
        x = x.cpu().numpy()
        for j in range(al.nref):
            t = ro.filt_tanl(a[j], 0.17, 0.15)
            c = (0.0, 0.0)
            if center:
                c = ro.phase_cog(t)
                t = ro.fshift(t, -c[0], -c[1])
            t = ro.normalize_mask(t, mask)
            assert abs(cs[j, 0] - c[0]) < 1e-3 and abs(cs[j, 1] - c[1]) < 1e-3
            assert np.abs(x[j] - t).max() < 2e-4 * np.abs(t).max()
    # fshift by a given centre (the reference-free average-centre rule), no filter, no normalisation
    x = avg[:1].clone()
    al.engine.filter_references(x, 0.0, 0.0, center=-1, cs_in=[[1.25, -0.5]], normalize=False)
    t = ro.fshift(a[0], -1.25, 0.5)
    assert np.abs(x[0].cpu().numpy() - t).max() < 2e-5 * np.abs(t).max()
    al.close()


def test_mref_iteration_with_default_user_function():
    """MrefAligner.iterate(user_func="ref_ali2d") = the reference's per-iteration update (:517-564)"""
    from oracle import refine_oracle as ro
    al = _searched_aligner(n=600)
    sums = al.buf.sums.cpu().numpy()
    counts = al.buf.counts_i.cpu().numpy()
    mask = geometry.model_circle(al.ou, al.nx, al.nx)
    want, curve, (fl, aa), css = ro.mref_reference_update(sums, counts, mask, center=1)
    al.reduce_and_update("ref_ali2d", center=1)
    got = al.refs.cpu().numpy()
    gfl, gaa = al.filter_params[-1]
    assert abs(gfl - fl) < 5e-5 and abs(gaa - aa) < 5e-5, (gfl, gaa, fl, aa)
    assert 0.12 <= gfl <= 0.4 and gaa <= 0.2
    np.testing.assert_allclose(al.centres[-1], css, atol=2e-3)
    for j in range(al.nref):
        assert np.abs(got[j] - want[j]).max() < 5e-4 * np.abs(want[j]).max(), j
    # the filtered, centred references are what the next search uses
    al.iterate("ref_ali2d", center=1)
    assert np.isfinite(al.refs.cpu().numpy()).all()
    al.close()


def test_reffree_driver_with_user_function_and_average_centring():
    nx, ou, xr, n = 64, 25, 2, 300
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    al = RefFreeAligner(parts, ou, xr, xr, 1.0)
    for it in range(4):
        al.iterate(center=-1, user_func="ref_ali2d")
    assert len(al.filter_params) == 4 and all(0.12 <= f <= 0.4 and a <= 0.2 for f, a in al.filter_params)
    assert np.isfinite(al.tavg.cpu().numpy()).all()
    assert al.criteria[-1] > al.criteria[0]
    al.close()


@pytest.mark.parametrize("cfg", [
    # nx, ou, ir, rs, xr, yr, ts, nref, n, mode
    dict(nx=91, ou=36, ir=1, rs=1, xr=3, yr=3, ts=1.0, nref=3, n=24, mode=api.RA_MODE_MREF),      # odd box
    dict(nx=90, ou=36, ir=3, rs=1, xr=2, yr=2, ts=1.0, nref=2, n=24, mode=api.RA_MODE_MREF),      # inner radius > 1
    dict(nx=90, ou=36, ir=1, rs=2, xr=2, yr=1, ts=1.0, nref=2, n=24, mode=api.RA_MODE_MREF),      # every second ring
    dict(nx=64, ou=28, ir=1, rs=1, xr=1, yr=1, ts=0.5, nref=17, n=20, mode=api.RA_MODE_MREF),     # 17 references: 3 tiles of 6, half-pixel steps
    dict(nx=48, ou=20, ir=1, rs=1, xr=0, yr=0, ts=1.0, nref=9, n=20, mode=api.RA_MODE_MREF),      # rotation-only search
    dict(nx=90, ou=40, ir=1, rs=1, xr=3, yr=3, ts=1.0, nref=1, n=24, mode=api.RA_MODE_REFFREE),   # single reference, ormq rules
    dict(nx=128, ou=60, ir=5, rs=1, xr=2, yr=2, ts=1.0, nref=2, n=6, mode=api.RA_MODE_MREF),      # generic kernels, ir > 1
], ids=lambda c: "nx%d_ou%d_ir%d_rs%d_R%d" % (c["nx"], c["ou"], c["ir"], c["rs"], c["nref"]))
def test_geometry_sweep_against_oracle(cfg):
    """ring ranges, odd boxes, ring skips, fractional steps, reference counts around the tile sizes"""
    nx, ou, nref, n = cfg["nx"], cfg["ou"], cfg["nref"], cfg["n"]
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, int(cfg["xr"]), int(cfg["yr"]), 0.25, ou=ou)
    rg = orc.rings(cfg["ir"], ou, cfg["rs"])
    mask = orc.model_circle(ou, nx, nx)
    refs_n, cref = orc.prepare_refs(refs, mask, rg)
    d = np.zeros((n, 2), np.float32)
    if cfg["mode"] == api.RA_MODE_MREF:
        params, infos, _, _ = orc.mref_iteration(parts, cref, rg, cfg["xr"], cfg["yr"], cfg["ts"], d, nthreads=8)
    else:
        params = np.zeros((n, 6), np.float32)
        params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, cfg["xr"], cfg["yr"], cfg["ts"], (0, 0), d, params, nthreads=8)
    eng = api.Engine(nx, ou, cfg["xr"], cfg["yr"], cfg["ts"], nref, cfg["mode"], first_ring=cfg["ir"], ring_skip=cfg["rs"])
    eng.set_references(torch.from_numpy(np.ascontiguousarray(refs_n)).to(eng.dev))
    got = eng.prepared_references()
    assert np.abs(got - cref).max() < 1e-6 * np.abs(cref).max()
    tp = torch.from_numpy(parts).to(eng.dev)
    st, res = eng.new_state(n), eng.new_result(n)
    eng.align(tp, st, res)
    eng.sync()
    compare_search(api.Engine.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    eng.close()


# ---------------------------------------------------------------------------------------------
# BASELINE.json configs beyond configs[1]: reference-free at 90 / 36 (configs[2]), nref = 50 (configs[3]),
# 256 x 256 with nref = 100 (configs[4]); flip counts are reported, not hidden

FLIP_LOG = []          # (test id, particles, flips) of every oracle comparison below; printed at the end of the session


def _log_flips(name, n, flips):
    """audit log of every oracle comparison: tie flips, sub-bin angle outliers, worst peak error.  Kept in a JSON file
    (gpurun_out/parity_audit.json, copied to profiles/ per round) because captured stdout does not survive a green run."""
    rec = {"test": name, "particles": n, "tie_flips": int(flips)}
    rec.update({k: v for k, v in LAST_COMPARE.items() if k != "n"})
    FLIP_LOG.append(rec)
    print("tie flips [%s]: %d of %d" % (name, flips, n))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        import json
        with open(os.path.join(out, "parity_audit.json"), "w") as f:
            json.dump({"_what": "oracle comparisons of tests/test_gpu_parity.py: float-tie flips of the integer assignment "
                                "(|dpeak|/peak < 3e-6), particles whose sub-bin angle differs by more than 2e-3 degrees, "
                                "largest relative CCF peak error", "comparisons": FLIP_LOG}, f, indent=1)
    except OSError:
        pass


@pytest.mark.parametrize("sigma", [0.25, 1.0])
def test_headline_sample_4096_particles(sigma):
    """BASELINE configs[1] geometry on a 4096-particle sample: identical integer assignments at sigma 0.25,
    audited float ties at sigma 1.0 (count recorded)"""
    nx, ou, nref, xr, n = 90, 36, 10, 3, 4096
    refs = synth.make_references(nref, nx, ou)
    dev = torch.device("cuda", 0)
    import bench
    tp, truth = bench.generate_shard(dev, refs, n, xr, xr, sigma, 0, nx, ou)
    al = MrefAligner(tp, refs, ou, xr, xr, 1.0, preprocess=True)
    parts = al.particles.cpu().numpy()
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    al.search()
    al.engine.sync()
    flips = compare_search(al.params(), al.state.cpu().numpy(), params, infos, d)
    _log_flips("headline sigma=%g" % sigma, n, flips)
    if sigma == 0.25:
        assert flips == 0
        np.testing.assert_array_equal(al.buf.counts_i.cpu().numpy(), counts)
    al.close()


def _oracle_reffree_average(sums, n, mask, ss, it, center, user_func):
    """what the main node does with the even/odd sums before the search of iteration `it`
    (test_reffree_gpu_align.py:374-429): tavg, criterion, user function, average-centre rule"""
    from oracle import refine_oracle as ro
    tavg = ((sums[0, 0] + sums[0, 1]) / np.float32(n)).astype(np.float32)
    a1 = float((tavg[mask > 0.5].astype(np.float64) ** 2).sum())
    cs, fl, aa = [0.0, 0.0], None, None
    if user_func == "ref_ali2d":
        frsc = ro.fsc_mask(sums[0, 0], sums[0, 1], mask)
        tavg, cs_u, fl, aa = ro.ref_ali2d(mask, 0 if center == -1 else center, tavg, frsc)
        if center != -1:
            cs = list(cs_u)
    if center == -1 and it > 0:
        cs = [float(ss[0]) / n, float(ss[1]) / n]
        tavg = ro.fshift(tavg, -cs[0], -cs[1])
    return tavg, a1, cs, fl, aa


@pytest.mark.parametrize("center,user_func", [(-1, "ref_ali2d"), (-1, None), (0, None), (1, "ref_ali2d")])
def test_reffree_loop_matches_oracle_loop_at_headline_geometry(center, user_func):
    """BASELINE configs[2] geometry (90 x 90, ou = 36, xr = yr = 3, ts = 1): three iterations of RefFreeAligner, every
    step of every iteration against the oracle's restatement of ali2d_base (test_reffree_gpu_align.py:361-540 /
    :579-901): the average and criterion from the even/odd sums, the user function, the average-centre rule
    (center = -1) with and without the default user function, and ali2d_single_iter.  The oracle is re-seeded with
    the device's state at every iteration, so that a float tie in one iteration cannot hide an error in the next."""
    nx, ou, xr, n = 90, 36, 3, 192
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    al = RefFreeAligner(parts, ou, xr, xr, 1.0, refine=-1)
    sums = np.zeros((1, 2, nx, nx), np.float32)
    for i in range(n):
        sums[0, i % 2] += parts[i]
    ss = np.zeros(2)
    for it in range(3):
        prev = al.params().copy()
        d = al.state.cpu().numpy().copy()
        want_tavg, want_a1, want_cs, fl, aa = _oracle_reffree_average(sums, n, mask, ss, it, center, user_func)
        a1 = al.iterate(center, user_func)
        al.engine.sync()
        assert a1 == pytest.approx(want_a1, rel=2e-5)
        np.testing.assert_allclose(al.cs, want_cs, atol=1e-3 if (user_func and center == 1) else 2e-4)
        t = al.tavg[0].cpu().numpy()
        if user_func:    # the cut-off comes out of a simplex fit with xtol 1e-4 on both sides: dH/dfl * 1e-4 ~ 1e-3
            assert al.filter_params[-1][0] == pytest.approx(fl, abs=1e-4) and al.filter_params[-1][1] == pytest.approx(aa, abs=1e-4)
            assert np.abs(t - want_tavg).max() < 1.5e-3 * np.abs(want_tavg).max() + 1e-6
        else:
            assert np.abs(t - want_tavg).max() < 2e-5 * np.abs(want_tavg).max() + 1e-6
        # ali2d_single_iter from the device's own average, centre and previous parameters
        _, cref = orc.prepare_refs(t[None], None, rg)
        params = np.zeros((n, 6), np.float32)
        params[:, 0] = prev["alpha"]; params[:, 1] = prev["sx"]; params[:, 2] = prev["sy"]; params[:, 3] = prev["mirror"]
        osums = np.zeros((1, 2, nx, nx), np.float32)
        params, infos, osums, oss = orc.reffree_iteration(parts, cref[0], rg, xr, xr, 1.0, al.cs, d, params, sums=osums, nthreads=16)
        r = al.params()
        flips = compare_search(r, al.state.cpu().numpy(), params, infos, d)
        _log_flips("reffree loop center=%d func=%s it=%d" % (center, user_func, it), n, flips)
        # the next iteration starts from the device's sums and parameter sums
        sums = al.buf.sums.cpu().numpy().copy()
        ss = np.array([float(al.buf.extra_f[0].item()), float(al.buf.extra_f[1].item())])
        # refine = -1: alpha equals the oracle's bit for bit, so rot_shift2D sees the same parameters and the sums differ by
        # the association of ~100 float additions only (no quadri cell-border jumps left to tolerate)
        same = (r["mirror"] == params[:, 3].astype(int))
        if flips == 0:
            assert same.all()
            assert_alpha_equal_to_the_ulp(r["alpha"], params[:, 0])
            np.testing.assert_allclose(sums, osums, rtol=0, atol=3e-6 * np.abs(osums).max())
            np.testing.assert_allclose(ss, oss, rtol=0, atol=2e-4)
    assert al.iteration == 3
    al.close()


def test_reffree_ten_iterations_without_reseeding_drift():
    """BASELINE configs[2]'s iteration count: 10 iterations of RefFreeAligner (center = -1, no user function) beside an
    INDEPENDENT oracle loop -- its own sums, average, centre rule and parameters, never re-seeded from the device.  A
    float tie in iteration k changes one particle's contribution to the average of iteration k + 1 (1 / n of it), so the
    two loops may drift; the drift is measured (agreement of the integer assignments, relative difference of the
    average and of the criterion per iteration) and written to the audit log."""
    nx, ou, xr, n = 90, 36, 3, 256
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    al = RefFreeAligner(parts, ou, xr, xr, 1.0)
    sums = np.zeros((1, 2, nx, nx), np.float32)
    for i in range(n):
        sums[0, i % 2] += parts[i]
    ss = np.zeros(2)
    params = np.zeros((n, 6), np.float32)
    d = np.zeros((n, 2), np.float32)
    drift = []
    for it in range(10):
        want_tavg, want_a1, want_cs, _, _ = _oracle_reffree_average(sums, n, mask, ss, it, -1, None)
        a1 = al.iterate(-1, None)
        al.engine.sync()
        _, cref = orc.prepare_refs(want_tavg[None], None, rg)
        osums = np.zeros((1, 2, nx, nx), np.float32)
        params, infos, osums, oss = orc.reffree_iteration(parts, cref[0], rg, xr, xr, 1.0, want_cs, d, params, sums=osums, nthreads=16)
        sums, ss = osums, np.array(oss)
        r = al.params()
        jt = np.array([infos[i].jtot for i in range(n)])
        # the shifts are no longer integers after the first centre correction, and both loops rebuild them from their own
        # sub-bin angles (prb1d on an f32 / f64 neighbourhood): equal to |t| x d(alpha), i.e. a few 1e-5 pixels
        dd = np.abs(al.state.cpu().numpy() - d).max(1)
        same = (r["mirror"] == params[:, 3].astype(int)) & (r["angle_bin"] == jt) & (dd < 2e-4)
        t = al.tavg[0].cpu().numpy()
        da = np.abs(((r["alpha"] - params[:, 0]) + 180.0) % 360.0 - 180.0)
        drift.append({"iteration": it, "assignments_equal": float(same.mean()), "max_shift_diff": float(dd.max()),
                      "max_alpha_diff_deg": float(da.max()),
                      "average_rel_l2": float(np.linalg.norm(t - want_tavg) / np.linalg.norm(want_tavg)),
                      "criterion_rel": float(abs(a1 - want_a1) / want_a1)})
    LAST_COMPARE.clear()
    LAST_COMPARE.update(drift=drift)
    _log_flips("reffree 10 iterations, no re-seeding", n, int(round((1.0 - drift[-1]["assignments_equal"]) * n)))
    LAST_COMPARE.clear()
    print(drift)
    # the two loops stay together: at most a few particles part ways, the averages agree to 1e-3
    assert drift[-1]["assignments_equal"] >= 0.97 and drift[-1]["average_rel_l2"] < 5e-3 and drift[-1]["criterion_rel"] < 1e-3
    al.close()


def test_reffree_search_full_config2_sample():
    """configs[2] search (single reference, ormq rules) on 2048 particles at the headline geometry"""
    nx, ou, xr, n = 90, 36, 3, 2048
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    rg = orc.rings(1, ou, 1)
    tavg = parts.mean(0)[None].astype(np.float32)
    _, cref = orc.prepare_refs(tavg, None, rg)
    d = np.zeros((n, 2), np.float32); params = np.zeros((n, 6), np.float32)
    params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, xr, xr, 1.0, (0, 0), d, params, nthreads=16)
    eng, tp, st, res = run_engine(parts, tavg, ou, xr, xr, 1.0, mode=api.RA_MODE_REFFREE)
    # the reference of iteration 0 is the mean of the unaligned stack: broad, flat peaks (see compare_search)
    flips = compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    _log_flips("reffree search 90/36", n, flips)
    eng.close()


def test_fifty_references_config3():
    """BASELINE configs[3] per-GPU shape: nref = 50 (7 reference tiles), 90 x 90, all-reduce buffer of 3.24 MB"""
    nx, ou, nref, xr, n = 90, 36, 50, 3, 400
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 0.25, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    al = MrefAligner(parts, refs, ou, xr, xr, 1.0, preprocess=True)
    assert al.buf.flat.numel() * 4 == (nref * 2 * nx * nx + nref) * 4
    al.search()
    al.engine.sync()
    flips = compare_search(al.params(), al.state.cpu().numpy(), params, infos, d)
    _log_flips("nref=50", n, flips)
    assert flips == 0
    assert (al.params()["ref_id"] == truth["cls"]).all()
    al.buf.all_reduce()
    np.testing.assert_array_equal(al.buf.counts_i.cpu().numpy(), counts)
    assert_images_close(al.buf.sums.cpu().numpy(), sums, mask, 2e-5 * np.abs(sums).max() + 1e-4)
    al.close()


@pytest.mark.timeout(900)
def test_large_box_hundred_references_config4():
    """BASELINE configs[4]: 256 x 256, ou = 120, xr = yr = 5 (121 offsets), nref = 100 (13 reference tiles,
    maxrin 1024) on 4 particles against the oracle"""
    nx, ou, nref, xr, n = 256, 120, 100, 5, 4
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 0.25, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    assert rg.maxrin == 1024
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    r = api.Engine.result_to_numpy(res)
    flips = compare_search(r, st.cpu().numpy(), params, infos, d)
    _log_flips("256^2 nref=100", n, flips)
    assert (r["ref_id"] == truth["cls"]).all()
    gs = torch.zeros((nref, 2, nx, nx), device=eng.dev)
    gc = torch.zeros(nref, dtype=torch.int32, device=eng.dev)
    eng.transform_accumulate(tp, res, 0, None, gs, gc)
    eng.sync()
    assert (gc.cpu().numpy() == counts).all()
    # class sums: (i) against the oracle's rot_shift2D of the engine's own parameters -- the transform and the
    # accumulation, free of the conditioning of the sub-bin angle; (ii) against the oracle's sums: with 4 images in
    # 100 classes a 6e-5 degree difference of one angle (2 ulp of its f32 value) moves a few pixels across quadri's
    # cell borders, so the bar is the quantile part of assert_images_close
    got = gs.cpu().numpy()
    want = np.zeros_like(sums)
    for i in range(n):
        want[int(r["ref_id"][i]), i & 1] += orc.rot_shift2d(parts[i], float(r["alpha"][i]), float(r["sx"][i]), float(r["sy"][i]),
                                                            int(r["mirror"][i]))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * np.abs(want).max())
    diff = np.abs(got - sums)
    sel = np.broadcast_to(mask > 0.5, diff.shape)
    assert np.quantile(diff[sel], 0.999) < 2e-5 * np.abs(sums).max() + 1e-4
    assert np.abs(((r["alpha"] - params[:, 0] + 180.0) % 360.0) - 180.0).max() < 2e-3
    eng.close()


@pytest.mark.timeout(900)
def test_large_box_hundred_references_config4_noisy_sample():
    """BASELINE configs[4] at the bench's noise level: 32 particles at sigma = 1.0 against the oracle's full search over 100
    references x 121 offsets x 2 x 1024 angles -- identical integer assignments, peaks within 1e-4"""
    nx, ou, nref, xr, n = 256, 120, 100, 5, 32
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    assert eng.search_path == 2
    flips = compare_search(api.Engine.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    _log_flips("256^2 nref=100 sigma=1", n, flips)
    eng.close()


def test_large_box_is_refined_to_the_ulp():
    """the sub-bin refinement on a geometry whose rings exceed the LDS (256 x 256, ou = 120: 271 KB per offset; the exact kernels
    then work on global scratch): with every particle refined alpha equals the oracle's float32 to the ulp, 32 particles at
    sigma = 1.0, 12 references"""
    nx, ou, nref, xr, n = 256, 120, 12, 5, 32
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, sums, counts = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    eng = api.Engine(nx, ou, xr, xr, 1.0, nref, api.RA_MODE_MREF)
    assert eng.search_path == 2
    eng.set_refine(-1.0)                       # RA_ERR_STATE before round 4
    dev = eng.dev
    eng.set_references(torch.from_numpy(refs_n).to(dev))
    tp = torch.from_numpy(parts).to(dev)
    st, res = eng.new_state(n), eng.new_result(n)
    eng.align(tp, st, res)
    eng.sync()
    r = api.Engine.result_to_numpy(res)
    flips = compare_search(r, st.cpu().numpy(), params, infos, d)
    _log_flips("256^2 refined nref=12 sigma=1", n, flips)
    assert_alpha_equal_to_the_ulp(r["alpha"], params[:, 0])
    np.testing.assert_allclose(r["sx"], params[:, 1], rtol=0, atol=5e-7)
    np.testing.assert_allclose(r["sy"], params[:, 2], rtol=0, atol=5e-7)
    eng.close()


def test_vanished_class_is_reseeded_from_the_main_node():
    """a class with fewer than 4 members gets a random particle of the main node as its next reference
    (test_mref_gpu_align.py:523-528): same draw as random.seed(rand_seed); randint(0, nima-1)"""
    import random
    nx, ou, nref, xr, n = 32, 12, 4, 2, 60
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs[:2], n, xr, xr, 0.25, ou=ou)       # classes 2 and 3 get no members
    refs2 = refs.copy()
    refs2[2] = -refs[0]; refs2[3] = -refs[1]                                # anti-correlated: never the best match
    for user_func in (None, "ref_ali2d"):
        al = MrefAligner(parts, refs2, ou, xr, xr, 1.0, preprocess=True, rand_seed=77)
        counts = al.iterate(user_func, 0)
        assert counts[2] < 4 and counts[3] < 4 and counts[0] >= 4
        rng = random.Random(77)
        picks = [rng.randint(0, n - 1) for _ in range(2)]
        pp = al.particles.cpu().numpy()
        got = al.refs.cpu().numpy()
        mask = orc.model_circle(ou, nx, nx)
        for j, k in zip((2, 3), picks):
            if user_func is None:
                want = orc.normalize_mask(pp[k], mask, 1)        # :563 re-normalisation of every reference
                np.testing.assert_allclose(got[j], want, atol=2e-5)
            else:
                assert np.isfinite(got[j]).all() and np.abs(got[j]).max() > 0
        assert np.isfinite(got).all()
        al.close()


def test_transform_kernel_matches_the_reference_tree_bit_for_bit(golden_dir):
    """rot_shift2D on the device against tests/golden/rot_shift2d_ref.npz (output of the reference tree's own
    rot_scale_trans2D_background / quadri_background text, notebook/02 cell 2)"""
    g = np.load(os.path.join(golden_dir, "rot_shift2d_ref.npz"))
    for k in range(int(g["ncase"])):
        img, ang, dx, dy, out = (g["%s%d" % (nm, k)] for nm in ("img", "ang", "dx", "dy", "out"))
        c, nx = img.shape[0], img.shape[-1]
        eng = api.Engine(nx, nx // 2 - 4, 1, 1, 1.0, 1)
        rec = np.zeros(c, api.RESULT_DTYPE)
        rec["alpha"] = ang; rec["sx"] = dx; rec["sy"] = dy
        for mirror in (0, 1):
            rec["mirror"] = mirror
            res = torch.from_numpy(rec.view(np.int32).reshape(c, 8).copy()).to(eng.dev)
            al = torch.zeros((c, nx, nx), device=eng.dev)
            eng.transform_accumulate(torch.from_numpy(img).to(eng.dev), res, 0, al, None, None)
            eng.sync()
            want = out.copy()
            if mirror:
                start = 1 - nx % 2
                want[:, :, start:] = want[:, :, start:][:, :, ::-1]
            np.testing.assert_array_equal(al.cpu().numpy(), want)
        eng.close()


@pytest.mark.parametrize("nx,ou", [(64, 25), (128, 30)], ids=["box64", "box128-crop"])
@pytest.mark.parametrize("fused", ["1", "0"], ids=["one-launch", "class-by-class"])
def test_class_resident_alignment_isac_surface(fused, nx, ou, monkeypatch):
    """ref_free_alignment_2D* (cuda/gpu_aln_noref.h:94-109): every particle against the average of its own class
    with ormq rules, rot_shift2D, class means rebuilt on the device, tangent filter of the averages; all classes in one
    launch of the fused search kernel (ra_set_class_references / ra_align_classes) and, with the fused kernel switched
    off, class by class through the kernel pair"""
    default_path_only()
    from oracle import refine_oracle as ro
    monkeypatch.setenv("RALIGN_FUSED", fused)
    # (box128-crop: an engine of the size-generic class -- the search runs the fused kernel over a crop of the image, or the pair
    # kernel with the fused kernel switched off; the class-resident launch is not available there and the library walks the classes)
    xr, ncls = 2, 5
    sizes = [17, 30, 1, 24, 40]
    refs = synth.make_references(ncls, nx, ou)
    parts, cids = [], []
    for c, m in enumerate(sizes):
        p, _ = synth.make_particles(refs[c:c + 1], m, xr, xr, 0.5, shard=c, ou=ou)
        parts.append(p); cids += [c] * m
    parts = np.concatenate(parts); n = len(cids)
    cid = (ctypes.c_int * n)(*cids)
    lib = api.load_library()
    cfg = api.AlignConfig(n, ncls, nx, ou, 256, 1.0, float(xr), float(xr))
    assert lib.ref_free_alignment_2D_size_check(ctypes.byref(cfg), 0, 0.9, False) is True
    assert lib.ref_free_alignment_2D_size_check(ctypes.byref(cfg), 0, 1e-9, False) is False
    prm = ctypes.cast(lib.ref_free_alignment_2D_init(ctypes.byref(cfg), api.get_c_ptr_array(list(parts)),
                                                     api.get_c_ptr_array(list(refs)), cid, 0), api.aln_param_ptr)
    rg = orc.rings(1, ou, 1)
    cur = refs.copy()
    d = np.zeros((n, 2), np.float32)
    params = np.zeros((n, 6), np.float32)
    got_refs = np.zeros_like(refs)
    for it in range(2):
        lib.ref_free_alignment_2D()
        start = 0
        new = np.zeros_like(cur)
        for c, m in enumerate(sizes):
            _, cref = orc.prepare_refs(cur[c:c + 1], None, rg)
            sl = slice(start, start + m)
            ps = params[sl].copy(); ds = d[sl].copy()
            ps, infos, _, _ = orc.reffree_iteration(parts[sl], cref[0], rg, xr, xr, 1.0, (0, 0), ds, ps)
            params[sl] = ps; d[sl] = ds
            acc = np.zeros((nx, nx), np.float32)
            for i in range(m):
                acc += orc.rot_shift2d(parts[start + i], float(ps[i, 0]), float(ps[i, 1]), float(ps[i, 2]), int(ps[i, 3]))
                k = start + i
                assert prm[k].ref_id == c and prm[k].mirror == bool(ps[i, 3])
                assert prm[k].shift_x == pytest.approx(ds[i, 0], abs=1e-5) and prm[k].shift_y == pytest.approx(ds[i, 1], abs=1e-5)
                assert prm[k].angle == pytest.approx(ps[i, 0], abs=3e-3)
            new[c] = acc / np.float32(m)
            start += m
        assert lib.ra_isac_get_references(got_refs.ctypes.data_as(api.float_ptr)) == 0
        assert_images_close(got_refs, new, np.ones((nx, nx), np.float32), 2e-5 * np.abs(new).max() + 1e-5)
        cur = got_refs.copy()       # continue from the device's averages: the loop is compared step by step
    lib.ref_free_alignment_2D_filter_references(0.25, 0.1)
    assert lib.ra_isac_get_references(got_refs.ctypes.data_as(api.float_ptr)) == 0
    for c in range(ncls):
        want = ro.filt_tanl(cur[c], 0.25, 0.1)
        assert np.abs(got_refs[c] - want).max() < 2e-4 * np.abs(want).max()
    lib.gpu_clear()


def test_align_classes_equals_the_class_loop():
    """ra_set_class_references + ra_align_classes (one launch, reference per particle) give the records of
    ra_set_references + ra_align run class by class, bit for bit"""
    default_path_only()
    nx, ou, xr, ncls = 64, 25, 2, 6
    sizes = [9, 33, 1, 20, 64, 5]
    refs = synth.make_references(ncls, nx, ou)
    parts, cls = [], []
    for c, m in enumerate(sizes):
        p, _ = synth.make_particles(refs[c:c + 1], m, xr, xr, 0.5, shard=c, ou=ou)
        parts.append(p); cls += [c] * m
    parts = np.concatenate(parts); n = len(cls)
    dev = torch.device("cuda:0")
    eng = api.Engine(nx, ou, xr, xr, 1.0, 1, api.RA_MODE_REFFREE)
    assert eng.search_path == 1
    tp = torch.from_numpy(parts).to(dev); tr = torch.from_numpy(refs).to(dev)
    tc = torch.tensor(cls, dtype=torch.int32, device=dev)
    st1, res1 = eng.new_state(n), eng.new_result(n)
    eng.set_class_references(tr)
    eng.align_classes(tp, st1, res1, tc)
    eng.sync()
    st2, res2 = eng.new_state(n), eng.new_result(n)
    start = 0
    for c, m in enumerate(sizes):
        eng.set_references(tr[c:c + 1])
        eng.align(tp[start:start + m], st2[start:start + m], res2[start:start + m])
        start += m
    eng.sync()
    assert torch.equal(res1, res2) and torch.equal(st1, st2)
    eng.close()
    # protocol: the class-resident launch needs one reference in ormq mode, and its references before the search
    eng = api.Engine(nx, ou, xr, xr, 1.0, 3, api.RA_MODE_MREF)
    with pytest.raises(api.EngineError):
        eng.set_class_references(tr)
    eng.close()
    eng = api.Engine(nx, ou, xr, xr, 1.0, 1, api.RA_MODE_REFFREE)
    with pytest.raises(api.EngineError):
        eng.align_classes(tp, st1, res1, tc)
    eng.close()


def test_size_check_says_no_when_it_does_not_fit_and_covers_what_init_allocates():
    lib = api.load_library()
    cfg = api.AlignConfig(2000, 10, 90, 36, 256, 1.0, 3.0, 3.0)
    assert lib.pre_align_size_check(2000, ctypes.byref(cfg), 0, 0.9, False) is True
    assert lib.pre_align_size_check(2000, ctypes.byref(cfg), 0, 1e-7, False) is False        # request of ~30 KB
    huge = api.AlignConfig(40_000_000, 10, 90, 36, 256, 1.0, 3.0, 3.0)                      # 1.3 TB of images
    assert lib.pre_align_size_check(40_000_000, ctypes.byref(huge), 0, 0.9, False) is False
    # the estimate is an upper bound of what pre_align_init really takes from the device
    free0 = torch.cuda.mem_get_info(0)[0]
    need = lib.ra_legacy_bytes(2000, ctypes.byref(cfg))
    lib.pre_align_init(2000, ctypes.byref(cfg), 0)
    used = free0 - torch.cuda.mem_get_info(0)[0]
    lib.gpu_clear()
    assert need >= used, (need, used)
    assert need < used + (4 << 30)          # the estimate also covers the two-kernel path's spectra panels (allocated on first use)


def test_reset_shifts_rejects_a_wider_window_at_constant_offset_count():
    """xr=1, ts=0.5 -> xr=4, ts=2 keeps 25 offsets but needs a wider image border than ra_create sized"""
    default_path_only("RALIGN_GENERIC")          # (the size-generic kernels have no LDS image border: they take the wider window)
    eng = api.Engine(64, 20, 1, 1, 0.5, 2)
    assert eng.num_shifts == 25
    with pytest.raises(api.EngineError):
        eng.reset_shifts(4, 4, 2.0)
    eng.reset_shifts(1, 1, 1.0)
    assert eng.num_shifts == 9
    eng.close()


def test_fused_kernel_is_the_default_path_and_agrees_with_the_kernel_pair(monkeypatch):
    """BASELINE configs[1] / [2] geometries run the particle-resident kernel (ralign_fused.h); the polar + contraction
    pair (RALIGN_FUSED=0, also the path for more than 16 references) gives the same assignments"""
    default_path_only()
    nx, ou, nref, xr, n = 90, 36, 10, 3, 300
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    assert eng.search_path == 1
    a = api.Engine.result_to_numpy(res).copy(); sa = st.cpu().numpy().copy()
    eng.reset_shifts(1, 1, 0.5)
    assert eng.search_path == 1          # any window of the geometry, fractional steps included
    eng.close()
    for mode, k in ((api.RA_MODE_REFFREE, 1),):
        e2 = api.Engine(nx, ou, xr, xr, 1.0, k, mode)
        assert e2.search_path == 1
        e2.close()
    monkeypatch.setenv("RALIGN_FUSED", "0")
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    assert eng.search_path == 0
    b = api.Engine.result_to_numpy(res).copy(); sb = st.cpu().numpy().copy()
    eng.close()
    rel = np.abs(a["peak"] - b["peak"]) / np.abs(a["peak"])
    assert rel.max() < 2e-5
    same = np.ones(n, bool)
    for fld in ("ref_id", "mirror", "angle_bin", "shift_idx"):
        same &= a[fld] == b[fld]
    assert (~same).sum() <= 2 and (rel[~same] < TIE_RTOL).all()
    np.testing.assert_array_equal(sa[same], sb[same])


# ---------------------------------------------------------------------------------------------
# search schedules and variants

def test_nomirror_search_matches_ormq_with_nomirror():
    """--nomirror (test_reffree_gpu_align.py:921 -> ali2d_single_iter -> ormq(nomirror) -> Util.Crosrng_ns): only the
    straight half of Crosrng_ms is searched, in both kernel families"""
    default_path_only()
    nx, ou, xr, n = 90, 36, 3, 256
    refs = synth.make_references(1, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)       # half of the particles are mirrored
    rg = orc.rings(1, ou, 1)
    _, cref = orc.prepare_refs(refs, None, rg)
    orc.set_nomirror(True)
    try:
        d = np.zeros((n, 2), np.float32)
        params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, xr, xr, 1.0, (0, 0), d, np.zeros((n, 6), np.float32), nthreads=16)
    finally:
        orc.set_nomirror(False)
    assert (params[:, 3] == 0).all() and truth["mir"].any()
    for fused in ("1", "0"):
        os.environ["RALIGN_FUSED"] = fused
        try:
            eng = api.Engine(nx, ou, xr, xr, 1.0, 1, api.RA_MODE_REFFREE)
        finally:
            del os.environ["RALIGN_FUSED"]
        assert eng.search_path == int(fused)
        eng.set_nomirror(True)
        eng.set_references(torch.from_numpy(refs).to(eng.dev))
        st, res = eng.new_state(n), eng.new_result(n)
        eng.align(torch.from_numpy(parts).to(eng.dev), st, res)
        eng.sync()
        r = eng.result_to_numpy(res)
        assert (r["mirror"] == 0).all()
        flips = compare_search(r, st.cpu().numpy(), params, infos, d)
        _log_flips("nomirror fused=%s" % fused, n, flips)
        # and with the mirror search back on, the mirrored particles are found mirrored
        eng.set_nomirror(False)
        st2, res2 = eng.new_state(n), eng.new_result(n)
        eng.align(torch.from_numpy(parts).to(eng.dev), st2, res2)
        eng.sync()
        assert (eng.result_to_numpy(res2)["mirror"] == truth["mir"]).mean() > 0.98
        eng.close()


def test_multi_stage_schedule_against_oracle():
    """--xr "2 1" --ts "1 0.5": one search window per stage, the engine re-shifted per stage
    (test_reffree_gpu_align.py:215-216, :355-357); every iteration against ali2d_single_iter with that stage's window"""
    from cryo_ralib_amd.mref import ali2d_base_gpu
    nx, ou, n = 64, 25, 160
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, 2, 2, 0.5, ou=ou)
    rg = orc.rings(1, ou, 1)
    al = RefFreeAligner(parts, ou, "2 1", "-1", "1 0.5")
    assert al.stages == [(2.0, 2.0, 1.0), (1.0, 1.0, 0.5)]
    assert al.engine.num_shifts == 25
    for stage in (0, 1):
        al.set_stage(stage)
        x, y, t = al.stages[stage]
        assert al.engine.num_shifts == (2 * int(x / t) + 1) ** 2
        for it in range(2):
            prev = al.params().copy()
            d = al.state.cpu().numpy().copy()
            al.iterate(0, None)
            al.engine.sync()
            _, cref = orc.prepare_refs(al.tavg.cpu().numpy(), None, rg)
            params = np.zeros((n, 6), np.float32)
            params[:, 0] = prev["alpha"]; params[:, 1] = prev["sx"]; params[:, 2] = prev["sy"]; params[:, 3] = prev["mirror"]
            params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, x, y, t, (0, 0), d, params, nthreads=16)
            flips = compare_search(al.params(), al.state.cpu().numpy(), params, infos, d)
            _log_flips("stage %d it %d" % (stage, it), n, flips)
    al.close()
    # the driver walks the stages itself when asked to (SPHIRE's schedule) ...
    seen = []
    ali2d_base_gpu(parts, ou, [2, 1], [2, 1], [1, 0.5], maxit=2, all_stages=True,
                   on_iteration=lambda i, a, c: seen.append((i, a.stage, a.engine.num_shifts)))
    assert seen == [(1, 0, 25), (2, 0, 25), (3, 1, 25), (4, 1, 25)]
    # ... and runs stage 0 only by default, like the reference's GPU driver (N_step = 0, test_reffree_gpu_align.py:355-357)
    seen = []
    ali2d_base_gpu(parts, ou, [2, 1], [2, 1], [1, 0.5], maxit=2, on_iteration=lambda i, a, c: seen.append((i, a.stage, a.engine.num_shifts)))
    assert seen == [(1, 0, 25), (2, 0, 25)]


def test_auto_stop_at_maxit_zero():
    """maxit = 0 with auto_stop: ten iterations at most, and a stage ends with the first iteration whose criterion falls
    below the best one so far (the rule of the comments at test_reffree_gpu_align.py:224-229, :392-396, :422-432)"""
    from cryo_ralib_amd.mref import ali2d_base_gpu
    nx, ou, xr, n = 32, 12, 2, 150
    refs = synth.make_references(1, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    crit = []
    _, _, criteria = ali2d_base_gpu(parts, ou, xr, xr, 1.0, maxit=0, auto_stop=True, on_iteration=lambda i, a, c: crit.append(c))
    assert crit == criteria and 1 <= len(crit) <= 10
    best = -1.0e22
    for i, c in enumerate(crit):
        if c < best:
            assert i == len(crit) - 1, "went on after the criterion decreased"
        else:
            best = c
    if len(crit) < 10:
        assert crit[-1] < max(crit[:-1])
    # a fixed count ignores the criterion
    _, _, c5 = ali2d_base_gpu(parts, ou, xr, xr, 1.0, maxit=5)
    assert len(c5) == 5
    # the default at maxit = 0 is the reference driver's: it computes the flag `again` and never tests it -> 10 iterations
    _, _, c10 = ali2d_base_gpu(parts, ou, xr, xr, 1.0, maxit=0)
    assert len(c10) == 10


@pytest.mark.parametrize("nref,nx,ou", [(13, 90, 36), (16, 90, 36), (12, 32, 12), (16, 48, 20)])
def test_fused_kernel_with_two_spectra_rounds(nref, nx, ou):
    """11 < nref <= 16: the accumulators of a pass feed two inverse-FFT rounds (the spectra of 4 offsets x nref references
    do not fit the ring-buffer space at once); also the widest unit count per wave"""
    default_path_only()
    xr, n = 2, 96
    refs = synth.make_references(nref, nx, ou)
    parts, truth = synth.make_particles(refs, n, xr, xr, 0.25, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    assert eng.search_path == 1
    r = api.Engine.result_to_numpy(res)
    flips = compare_search(r, st.cpu().numpy(), params, infos, d)
    _log_flips("nref=%d nx=%d" % (nref, nx), n, flips)
    assert flips == 0
    if nx >= 48:         # 12 references in a 32 x 32 box are too alike for the planted class to win every time (the oracle agrees)
        assert (r["ref_id"] == truth["cls"]).all()
    eng.close()


# ---------------------------------------------------------------------------------------------
# more than 16 references: search_tiled_kernel (ralign_tiled.h), BASELINE configs[3]

@pytest.mark.parametrize("nref,sigma", [(50, 0.25), (50, 1.0), (100, 1.0), (17, 1.0), (24, 1.0), (37, 0.5)])
def test_tiled_kernel_covers_more_than_sixteen_references(nref, sigma):
    """nref > 16 at the headline geometry stays particle-resident (search_path 1: reference tiles walked inside the
    workgroup, A operand in registers); assignments and peaks against the oracle, ragged last tiles included"""
    default_path_only()
    nx, ou, xr, n = 90, 36, 3, 300
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, sigma, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    d = np.zeros((n, 2), np.float32)
    d[::7] = (2, -1); d[3::11] = (-7, 6)             # edge-limited windows too
    d0 = d.copy()
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=16)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0, state=d0)
    assert eng.search_path == 1
    flips = compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d)
    _log_flips("tiled nref=%d sigma=%g" % (nref, sigma), n, flips)
    eng.close()


def test_tiled_kernel_equals_fused_kernel_at_ten_references(monkeypatch):
    """RALIGN_TILED=1 forces the tiled kernel at nref = 10 (one tile): same records as search_fused_kernel"""
    default_path_only()
    nx, ou, nref, xr, n = 90, 36, 10, 3, 300
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 1.0, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    a = api.Engine.result_to_numpy(res).copy(); sa = st.cpu().numpy().copy()
    eng.close()
    monkeypatch.setenv("RALIGN_TILED", "1")
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
    assert eng.search_path == 1
    b = api.Engine.result_to_numpy(res).copy(); sb = st.cpu().numpy().copy()
    eng.close()
    rel = np.abs(a["peak"] - b["peak"]) / np.abs(a["peak"])
    assert rel.max() < 2e-5
    same = np.ones(n, bool)
    for fld in ("ref_id", "mirror", "angle_bin", "shift_idx"):
        same &= a[fld] == b[fld]
    assert (~same).sum() <= 2 and (rel[~same] < TIE_RTOL).all()
    np.testing.assert_array_equal(sa[same], sb[same])


def test_tiled_kernel_in_the_iteration_loop():
    """three iterations of the host driver at nref = 24 (three reference tiles of 8 per pass, search_tiled_kernel) beside the
    oracle loop: state round trip, class sums, reference update; every particle refined, so alpha is the oracle's bit for bit"""
    default_path_only()
    nx, ou, nref, xr, n = 90, 36, 24, 3, 240
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5)
    al = MrefAligner(parts, refs, ou, xr, xr, 1.0, preprocess=True, refine=-1)
    assert al.engine.search_path == 1
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    cur = np.stack([orc.normalize_mask(r, mask, 1) for r in refs])
    op = np.stack([orc.normalize_mask(p, mask, 0) for p in parts])
    d = np.zeros((n, 2), np.float32)
    prev = None
    import random
    rng = random.Random(1000)                  # the driver's own draw for vanished classes (MrefAligner(rand_seed=1000))
    for it in range(3):
        params, infos, sums, counts, d = _oracle_mref_loop_step(op, cur, rg, mask, xr, prev, d, True)
        got_counts = al.iterate()
        r = al.params()
        flips = compare_search(r, al.state.cpu().numpy(), params, infos, d)
        _log_flips("tiled loop nref=24 it=%d" % it, n, flips)
        if flips:
            prev = np.zeros((n, 6), np.float32)
            prev[:, 0] = r["alpha"]; prev[:, 1] = r["sx"]; prev[:, 2] = r["sy"]; prev[:, 3] = r["mirror"]
            d = al.state.cpu().numpy().copy()
            cur = al.refs.cpu().numpy().copy()
            continue
        prev = params
        np.testing.assert_array_equal(got_counts, counts)
        assert_alpha_equal_to_the_ulp(r["alpha"], params[:, 0])
        live = counts >= 4
        # a vanished class (240 particles over 24 classes: likely) is re-seeded with a random particle of the main node, drawn
        # in class order from the driver's RNG, and normalised like every other reference (test_mref_gpu_align.py:523-528, 563)
        cur = np.stack([orc.normalize_mask((sums[j, 0] + sums[j, 1]) * np.float32(1.0 / float(max(counts[j], 1))), mask, 1)
                        if live[j] else orc.normalize_mask(op[rng.randint(0, n - 1)], mask, 1) for j in range(nref)])
        np.testing.assert_allclose(al.refs.cpu().numpy(), cur, rtol=0, atol=3e-6 * np.abs(cur).max())
    al.close()


@pytest.mark.parametrize("nx,ou,xr,yr,n,nref", [(90, 36, 3, 3, 23, 3), (90, 36, 3, 3, 1, 2), (32, 12, 2, 1, 37, 1), (32, 12, 1, 1, 5, 4),
                                               (32, 12, 1, 0, 9, 2), (32, 12, 0, 0, 7, 2),
                                               # search_tiled_kernel (a run-time flag of the same stream): 49, 15, 9 and 3 offsets
                                               (90, 36, 3, 3, 23, 18), (90, 36, 3, 3, 1, 16), (64, 28, 2, 1, 19, 20), (64, 28, 1, 1, 7, 24),
                                               (64, 28, 1, 0, 10, 15)])
def test_dense_offset_stream_is_bitwise_the_padded_one(nx, ou, xr, yr, n, nref):
    """search_fused_kernel's PACK: the offsets of a workgroup's consecutive particles fill the passes without padding (49
    offsets: 4 particles = 49 passes), a pass may hold offsets of two particles.  Everything behind the sampling is per offset
    slot, so the records -- peaks, neighbourhoods, assignments -- equal those of the padded stream (RALIGN_PACK=0) bit for bit;
    particle counts that leave partial last passes, one particle, and windows of 3 and 1 offsets (no packing: a pass would hold
    more than two particles) included"""
    default_path_only()
    refs = synth.make_references(max(nref, 1), nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, max(yr, 1), 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    mode = api.RA_MODE_MREF if nref > 1 else api.RA_MODE_REFFREE
    outs = []
    for pack in ("1", "0"):
        os.environ["RALIGN_PACK"] = pack
        try:
            # few workgroups, so that each walks over several particles
            os.environ["RALIGN_GRID"] = "3"
            eng, tp, st, res = run_engine(parts, refs_n[:nref] if nref > 1 else refs_n[:1], ou, xr, yr, 1.0, mode=mode)
        finally:
            os.environ.pop("RALIGN_PACK", None); os.environ.pop("RALIGN_GRID", None)
        assert eng.search_path == 1 and bool(eng.search_tiled) == (nref >= 15)
        outs.append((eng.result_to_numpy(res).copy(), st.cpu().numpy().copy()))
        eng.close()
    for f in api.RESULT_DTYPE.names:
        np.testing.assert_array_equal(outs[0][0][f], outs[1][0][f], err_msg=f)
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_device_fit_tanh_agrees_with_the_host_routine():
    """fsc_fit_kernel (FSC average over the live classes, fit_tanh with amoeba, ref_ali2d's clamps, all on the device) against the
    host restatement ra_class_fsc + ra_fit_tanh on the class sums of a searched stack: filter parameters within 2e-5, the curve
    fit_tanh leaves behind (zeroed behind its first drop below 0.1) and the points per shell identical"""
    al = _searched_aligner(n=600)
    eng = al.engine
    frsc = eng.class_fsc(al.buf.sums, al.buf.counts_i, 4, masked=False)
    fl, aa = api.fit_tanh(frsc)                                  # edits frsc[1] in place like the original
    fit = torch.zeros(8, device=eng.dev)
    curve = torch.zeros(3 * eng.fsc_len, device=eng.dev)
    eng.class_fsc_fit(al.buf.sums, al.buf.counts_i, fit, curve, 4, masked=False)
    eng.sync()
    f = fit.cpu().numpy(); c = curve.cpu().numpy().reshape(3, -1)
    assert f[4] == 0.0
    assert abs(f[2] - fl) < 2e-5 and abs(f[3] - aa) < 2e-5, (f[:4], fl, aa)
    assert f[0] == np.float32(max(min(0.4, f[2]), 0.12)) and f[1] == np.float32(min(f[3], 0.2))
    np.testing.assert_array_equal(c[0], np.asarray(frsc[0], np.float32))
    np.testing.assert_allclose(c[1], np.asarray(frsc[1], np.float32), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(c[2], np.asarray(frsc[2], np.float32))
    # every class below min_count: status 1, nothing fitted
    eng.class_fsc_fit(al.buf.sums, torch.zeros_like(al.buf.counts_i), fit, curve, 4, masked=False)
    eng.sync()
    assert fit.cpu().numpy()[4] == 1.0
    al.close()


@pytest.mark.timeout(900)
def test_large_box_block_shapes_are_bitwise_alike(monkeypatch):
    """the large-box contraction in every shape it has -- blocks of 1 x 7, 2 x 7 and 4 x 7 tiles with the transforms in a second
    kernel (half-spectrum scratch) -- is the same arithmetic per (particle-offset, reference) pair: peaks, neighbourhoods and
    assignments agree bit for bit; the one-kernel path of round 3 (another inverse FFT) agrees in every assignment and to
    1e-6 in the peaks; 3 particles x 124 offset slots = 47 tiles of 8, so every shape ends in a partial block"""
    nx, ou, nref, xr, n = 256, 120, 100, 5, 3
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    outs = {}
    for name, env in (("4x7", {"RALIGN_GCCF_TM": "4"}), ("2x7", {"RALIGN_GCCF_TM": "2"}), ("1x7", {"RALIGN_GCCF_TM": "1"}),
                      ("one kernel", {"RALIGN_GCCF_TM": "1", "RALIGN_GCCF_SPLIT": "0"})):
        for k in ("RALIGN_GCCF_TM", "RALIGN_GCCF_SPLIT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng, tp, st, res = run_engine(parts, refs_n, ou, xr, xr, 1.0)
        outs[name] = (api.Engine.result_to_numpy(res).copy(), st.cpu().numpy().copy())
        eng.close()
    r0, s0 = outs["4x7"]
    for name, (r, s) in outs.items():
        if name == "one kernel":        # another inverse FFT (five radix-4 stages through the LDS): peaks to the last bits only
            for f in ("ref_id", "mirror", "angle_bin", "shift_idx"):
                np.testing.assert_array_equal(r[f], r0[f], err_msg="%s: %s" % (name, f))
            np.testing.assert_allclose(r["peak"], r0["peak"], rtol=1e-6)
            continue
        for f in r0.dtype.names:
            np.testing.assert_array_equal(r[f], r0[f], err_msg="%s: %s" % (name, f))
        np.testing.assert_array_equal(s, s0, err_msg=name)
