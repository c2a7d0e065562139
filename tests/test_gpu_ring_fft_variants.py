"""The ring jobs' FFT half (transposes through LDS, split step) in every job variant and every partial job, at the smallest
geometries that reach each variant:

    nx 32, ou 12   128- and 64-sample jobs and the mixed job (8 - 32 samples); two 128-sample rings in a job of eight
    nx 64, ou 25   a 256-sample job with five of its eight rings
    nx 90, ou 36   full 256-sample jobs
    nx 94, ou 41   512-sample rings (ring_job512)

What each test reaches:

  * Element by element: Engine.debug_spectra against the oracle (Polar2Dm -> Normalize_ring -> Frngs), 1e-5 of the ring buffer's
    largest element (the bar of the polar-stage checks of test_gpu_parity.py).  For the 90 x 90 class of boxes debug_spectra
    launches polar_fft_kernel whichever family the engine's search uses, for nx 94 the polar stage of search_solo_kernel: these
    are ring_job<R1, LR> (codes 0 - 7), ring_job_mix and ring_job512 WITHOUT the early split-step reads (EARLY = false).  The
    engine is created under RALIGN_FUSED=0, the kernel pair's; a default engine would launch the same kernel, so it is not run.
  * The EARLY instantiations (ring_job<8, 8, true, true>, <16, 8, true, true>, <8, 4, true, true> of search_fused_kernel) have no
    spectra output.  They are compared through the full search: fused path against kernel pair on the same particles, identical
    integer assignments and peaks equal to 1e-6 relative, at every geometry above and in both modes.  At nx 94 RALIGN_FUSED=0
    does not change the path (search_solo_kernel both times); that case repeats one kernel.
"""
import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, geometry, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-5
GEOMETRIES = [(32, 12, 2), (64, 25, 3), (90, 36, 3), (94, 41, 2)]      # nx, ou, xr
N = 3

_inputs = {}


def inputs(nx, ou, xr):
    """particles, states and the oracle's spectra of one geometry, computed once: want[mode][p][s] (None outside the window)"""
    key = (nx, ou, xr)
    if key not in _inputs:
        refs = synth.make_references(2, nx, ou)
        parts, _ = synth.make_particles(refs, N, xr, xr, 0.5, ou=ou)
        rg = orc.rings(1, ou, 1)
        st = np.zeros((N, 2), np.float32)
        st[1] = (1, -1)
        sh = geometry.shift_list(xr, xr, 1.0)
        cnx = nx // 2 + 1
        want = {api.RA_MODE_MREF: [], api.RA_MODE_REFFREE: []}
        for p in range(N):
            # offsets outside the particle's window are masked later and may differ (zero border vs clamped taps)
            lo = geometry.search_range(nx, ou, st[p, 0], xr), geometry.search_range(nx, ou, st[p, 1], xr)
            rows = {m: [] for m in want}
            for s in range(len(sh)):
                if not (-lo[0][0] <= sh[s, 0] <= lo[0][1] and -lo[1][0] <= sh[s, 1] <= lo[1][1]):
                    for m in want:
                        rows[m].append(None)
                    continue
                c = orc.polar2dm(parts[p], cnx + st[p, 0] + sh[s, 0], cnx + st[p, 1] + sh[s, 1], rg)
                rows[api.RA_MODE_REFFREE].append(orc.frngs(c, rg))
                rows[api.RA_MODE_MREF].append(orc.frngs(orc.normalize_ring(c, rg), rg))
            for m in want:
                want[m].append(rows[m])
        for a in (parts, st):
            a.setflags(write=False)
        _inputs[key] = parts, st, sh, rg, want
    return _inputs[key]


def spectra(nx, ou, xr, mode, parts, st):
    eng = api.Engine(nx, ou, xr, xr, 1.0, 2 if mode == api.RA_MODE_MREF else 1, mode)
    try:
        return eng.debug_spectra(torch.from_numpy(parts.copy()).to(eng.dev), torch.from_numpy(st.copy()).to(eng.dev)), eng.search_path
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [api.RA_MODE_MREF, api.RA_MODE_REFFREE], ids=["mref", "reffree"])
@pytest.mark.parametrize("nx,ou,xr", GEOMETRIES)
def test_ring_spectra_element_by_element(monkeypatch, nx, ou, xr, mode):
    parts, st, sh, rg, want = inputs(nx, ou, xr)
    monkeypatch.setenv("RALIGN_FUSED", "0")
    got, path = spectra(nx, ou, xr, mode, parts, st)
    assert got.shape == (N, len(sh), rg.lcirc)
    checked, worst = 0, 0.0
    for p in range(N):
        for s in range(len(sh)):
            w = want[mode][p][s]
            if w is None:
                continue
            err = np.abs(got[p, s] - w).max() / np.abs(w).max()
            worst = max(worst, err)
            assert err < RTOL, (p, s, err, int(np.abs(got[p, s] - w).argmax()))
            checked += 1
    print("nx %d ou %d mode %d: engine path %d, %d spectra, largest error %.2e of the ring maximum" % (nx, ou, mode, path, checked, worst))
    assert checked >= N * len(sh) // 2


@pytest.mark.parametrize("mode", [api.RA_MODE_MREF, api.RA_MODE_REFFREE], ids=["mref", "reffree"])
@pytest.mark.parametrize("nx,ou,xr", GEOMETRIES)
def test_full_search_fused_path_and_kernel_pair_agree(monkeypatch, nx, ou, xr, mode):
    """the same five particles through the particle-resident search (ring jobs with the early split-step reads) and through the
    kernel pair: identical integer assignments, peaks equal to 1e-6 relative"""
    n = 5
    nref = 3 if mode == api.RA_MODE_MREF else 1
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    if mode == api.RA_MODE_MREF:
        refs_in, _ = orc.prepare_refs(refs, orc.model_circle(ou, nx, nx), orc.rings(1, ou, 1))
    else:
        refs_in = refs
    out = {}
    for fused in ("default", "0"):
        if fused == "0":
            monkeypatch.setenv("RALIGN_FUSED", "0")
        else:
            monkeypatch.delenv("RALIGN_FUSED", raising=False)
        eng = api.Engine(nx, ou, xr, xr, 1.0, nref, mode)
        eng.set_references(torch.from_numpy(np.ascontiguousarray(refs_in)).to(eng.dev))
        st, res = eng.new_state(n), eng.new_result(n)
        eng.align(torch.from_numpy(parts).to(eng.dev), st, res)
        eng.sync()
        out[fused] = eng.result_to_numpy(res).copy(), st.cpu().numpy().copy(), eng.search_path
        eng.close()
    (a, sa, pa), (b, sb, pb) = out["default"], out["0"]
    if nx <= 90:
        assert pa == 1 and pb == 0, (pa, pb)        # particle-resident kernel against polar + contraction pair
    rel = np.abs(a["peak"] - b["peak"]) / np.abs(a["peak"])
    print("nx %d ou %d mode %d: paths %d / %d, largest relative peak difference %.2e" % (nx, ou, mode, pa, pb, rel.max()))
    for fld in ("ref_id", "mirror", "angle_bin", "shift_idx"):
        np.testing.assert_array_equal(a[fld], b[fld], err_msg=fld)
    np.testing.assert_array_equal(sa, sb)
    assert rel.max() <= 1e-6, rel


@pytest.mark.parametrize("nx,ou,xr", GEOMETRIES)
def test_same_input_twice_gives_the_same_bits(monkeypatch, nx, ou, xr):
    monkeypatch.delenv("RALIGN_FUSED", raising=False)
    parts, st, sh, rg, _ = inputs(nx, ou, xr)
    a, _ = spectra(nx, ou, xr, api.RA_MODE_MREF, parts, st)
    b, _ = spectra(nx, ou, xr, api.RA_MODE_MREF, parts, st)
    assert a.tobytes() == b.tobytes()
