"""search_fused_kernel with the short rings' taps read from the particle's image in global memory (through the vector L1) instead
of the LDS image: Engine.search_l1_tap_rings says which rings (0 | 64 | 128).  Global memory has no zero border, so the cases sit
where a wrong rule or a wrong base would show: shift states at the four corners of the window (the taps closest to the image's
edges), the last particle of the buffer at the lower-right corner (a tap past it would leave the allocation), passes that hold
offsets of two particles (the global base has to follow the particle of each round), both search modes (the reference-free one
with several references: one reference and the class-resident launch keep the LDS taps), a geometry whose window refuses the
source, and the window changed under a standing engine.

Every search is held against the CPU oracle with the bar of tests/test_gpu_parity.py -- zero disagreements in (reference, mirror,
angle bin, offset), CCF peaks within 1e-4 -- and the records of runs that must agree are compared byte for byte."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cryo_ralib_amd import api, synth
from oracle import oracle as orc
from test_gpu_parity import compare_search, default_path_only, oracle_setup, run_engine

pytestmark = pytest.mark.gpu

NX, OU, XR = 90, 36, 3
MASHI = NX // 2 + 1 - OU - 2          # 8
# the four corners of the window, its centre, a fractional state just inside it; the LAST particle sits at the lower-right corner
STATES = [(MASHI, MASHI), (-MASHI, -MASHI), (MASHI, -MASHI), (-MASHI, MASHI), (0, 0), (-6.9999995, 6.9999995), (3, -8), (-8, 2)]


def planted_states(n):
    d = np.array([STATES[i % len(STATES)] for i in range(n)], np.float32)
    d[n - 1] = (MASHI, MASHI)
    return d


def reffree_params_of(d0):
    """the header values (alpha, sx, sy, mirror, -, -) from which ali2d_single_iter starts at shift state d0: its state is the
    inverse transform of the header, (-sx, -sy) at alpha = 0"""
    p = np.zeros((len(d0), 6), np.float32)
    p[:, 1:3] = -d0
    return p


@pytest.fixture(scope="module")
def mref_case():
    """one stack, its oracle search from the planted states: shared, never changed"""
    n, nref = 16, 3
    refs = synth.make_references(nref, NX, OU)
    parts, _ = synth.make_particles(refs, n, XR, XR, 0.5, ou=OU)
    rg, mask, refs_n, cref = oracle_setup(refs, OU, NX)
    d0 = planted_states(n)
    d = d0.copy()
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, XR, XR, 1.0, d, nthreads=8)
    for a in (parts, refs_n, d0, d, params):
        a.setflags(write=False)
    return parts, refs_n, d0, d, params, infos


def test_l1_source_on_at_the_window_corners_and_the_last_particle(mref_case):
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PACK", "RALIGN_GRID")
    parts, refs_n, d0, d, params, infos = mref_case
    eng, tp, st, res = run_engine(parts, refs_n, OU, XR, XR, 1.0, state=d0)
    assert eng.search_path == 1 and not eng.search_tiled
    assert eng.search_l1_tap_rings in (64, 128), eng.search_l1_tap_rings
    assert compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d) == 0
    # determinism: a second run from the same states gives the same bytes
    st2 = torch.from_numpy(d0.copy()).to(eng.dev)
    res2 = eng.new_result(len(parts))
    eng.align(tp, st2, res2)
    eng.sync()
    assert torch.equal(res, res2) and torch.equal(st, st2)
    eng.close()


def test_split_passes_follow_the_particle_of_each_round(mref_case):
    """5 particles on 2 workgroups: dense passes that hold the last offsets of one particle and the first of the next.  The same
    stack particle by particle (every pass holds one particle) must give the same bytes, and both agree with the oracle"""
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PACK", "RALIGN_GRID")
    parts, refs_n, d0, d, params, infos = mref_case
    n = 5
    sel = [0, 1, 5, 6, 15]              # corners, the fractional state, the lower-right corner last
    p5, s5 = np.ascontiguousarray(parts[sel]), np.ascontiguousarray(d0[sel])
    os.environ["RALIGN_GRID"] = "2"
    try:
        eng, tp, st, res = run_engine(p5, refs_n, OU, XR, XR, 1.0, state=s5)
        assert eng.search_l1_tap_rings in (64, 128)
        st1, res1 = torch.from_numpy(s5.copy()).to(eng.dev), eng.new_result(n)
        for i in range(n):
            eng.align(tp[i:i + 1], st1[i:i + 1], res1[i:i + 1])
        eng.sync()
    finally:
        os.environ.pop("RALIGN_GRID", None)
    assert torch.equal(res, res1) and torch.equal(st, st1)
    assert compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params[sel], [infos[i] for i in sel], d[sel]) == 0
    eng.close()


def reffree_oracle_over_references(parts, refs, d0):
    """ormq of every particle against every reference on its own (the oracle's reference-free iteration takes one), then the best
    reference per particle as the engine picks it: the highest peak, the later reference on a tie"""
    rg = orc.rings(1, OU, 1)
    n = len(parts)
    runs = []
    for c in range(len(refs)):
        _, cref = orc.prepare_refs(refs[c:c + 1], None, rg)
        d = d0.copy()
        params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, XR, XR, 1.0, (0, 0), d, reffree_params_of(d0), nthreads=8)
        runs.append((params, infos, d))
    peaks = np.stack([r[0][:, 5] for r in runs])
    best = len(refs) - 1 - np.argmax(peaks[::-1], axis=0)           # last index of the maximum
    params = np.stack([runs[best[i]][0][i] for i in range(n)])
    params[:, 4] = best
    return params, [runs[best[i]][1][i] for i in range(n)], np.stack([runs[best[i]][2][i] for i in range(n)])


def beyond_the_window(d0):
    d0[2] = (11, -12); d0[3] = (-9.5, 30); d0[len(d0) - 1] = (12, 40)       # clamped onto the edge; the last particle onto the lower-right corner
    return d0


@pytest.mark.parametrize("nref", [3, 4])
def test_reffree_mode_with_the_l1_source_clamps_onto_the_window_edge(nref):
    """RA_MODE_REFFREE clamps a state beyond the window onto its edge (RA_MODE_MREF resets it to zero), so planted states beyond
    +-mashi sample at the corners, where the taps are closest to the image's border -- with three and four references the source is on"""
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PACK", "RALIGN_GRID")
    n = 12
    refs = synth.make_references(nref, NX, OU)
    parts, _ = synth.make_particles(refs, n, XR, XR, 0.5, ou=OU)
    d0 = beyond_the_window(planted_states(n))
    params, infos, d = reffree_oracle_over_references(parts, refs, d0)
    assert len(set(params[:, 4])) > 1                                # more than one reference wins somewhere
    eng, tp, st, res = run_engine(parts, refs, OU, XR, XR, 1.0, mode=api.RA_MODE_REFFREE, state=d0)
    assert eng.search_path == 1 and eng.search_l1_tap_rings in (64, 128), eng.search_l1_tap_rings
    assert np.abs(st.cpu().numpy()).max() <= MASHI + XR
    assert compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d) == 0
    eng.close()


def test_reffree_mode_with_one_reference_keeps_the_lds_taps():
    """one reference pair: the engine keeps every tap in LDS (measured slower through the L1), whatever the containment rule admits;
    the same planted states, against the oracle"""
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PACK", "RALIGN_GRID")
    n = 12
    refs = synth.make_references(1, NX, OU)
    parts, _ = synth.make_particles(refs, n, XR, XR, 0.5, ou=OU)
    d0 = beyond_the_window(planted_states(n))
    params, infos, d = reffree_oracle_over_references(parts, refs, d0)
    eng, tp, st, res = run_engine(parts, refs, OU, XR, XR, 1.0, mode=api.RA_MODE_REFFREE, state=d0)
    assert eng.search_path == 1 and eng.search_l1_tap_rings == 0
    assert compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d) == 0
    eng.close()


def test_class_resident_launch_cannot_reach_the_l1_source():
    """ra_align_classes needs an engine of ONE reference (the class picks the B stream), and one reference pair keeps the taps in
    LDS: under the shipped host rule the class-resident launch never runs the L1 source.  This case pins that -- search_l1_tap_rings
    == 0 -- and that the launch still agrees with the oracle from the planted states, two classes"""
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PACK", "RALIGN_GRID")
    sizes = [7, 5]
    refs = synth.make_references(2, NX, OU)
    parts = np.concatenate([synth.make_particles(refs[c:c + 1], m, XR, XR, 0.5, shard=c, ou=OU)[0] for c, m in enumerate(sizes)])
    n = len(parts)
    cls = np.repeat(np.arange(2), sizes).astype(np.int32)
    d0 = planted_states(n)
    eng = api.Engine(NX, OU, XR, XR, 1.0, 1, api.RA_MODE_REFFREE)
    assert eng.search_path == 1 and eng.search_l1_tap_rings == 0
    tp = torch.from_numpy(parts).to(eng.dev)
    st, res = torch.from_numpy(d0.copy()).to(eng.dev), eng.new_result(n)
    eng.set_class_references(torch.from_numpy(refs).to(eng.dev))
    eng.align_classes(tp, st, res, torch.from_numpy(cls).to(eng.dev))
    eng.sync()
    r, s = eng.result_to_numpy(res), st.cpu().numpy()
    start = 0
    for c, m in enumerate(sizes):
        sl = slice(start, start + m)
        params, infos, d = reffree_oracle_over_references(parts[sl], refs[c:c + 1], d0[sl])
        assert compare_search(r[sl], s[sl], params, infos, d) == 0       # (records of the class-resident launch carry reference 0)
        start += m
    eng.close()


def test_l1_source_off_where_a_tap_could_leave_the_image_and_follows_the_window():
    """70 / 21 with a y range of 13: cn 36, mashi 13 -- a ring of radius 10 (the longest of 64 samples) reaches row 36 - 26 - 10 = 0
    at the window's corner, so the rule refuses every setting and all taps stay in LDS.  With the window narrowed to +-1 under the
    standing engine the rings of 64 samples qualify (those of 128 do not: 36 + 14 + 20 + 1 > 70), and widened again they do not"""
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PACK", "RALIGN_GRID")
    nx, ou, xr, yr, n, nref = 70, 21, 1, 13, 6, 3
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, 3, 0.5, ou=ou)
    rg, mask, refs_n, cref = oracle_setup(refs, ou, nx)
    mashi = nx // 2 + 1 - ou - 2
    d0 = np.array([(mashi, mashi), (-mashi, -mashi), (mashi, -mashi), (-mashi, mashi), (0, 0), (mashi, mashi)], np.float32)
    d = d0.copy()
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, yr, 1.0, d, nthreads=8)
    eng, tp, st, res = run_engine(parts, refs_n, ou, xr, yr, 1.0, state=d0)
    assert eng.search_path == 1 and not eng.search_tiled
    assert eng.search_l1_tap_rings == 0
    assert compare_search(eng.result_to_numpy(res), st.cpu().numpy(), params, infos, d) == 0
    # the narrow window under the same engine: the source comes on, at the corners of ITS window
    eng.reset_shifts(1.0, 1.0, 1.0)
    assert eng.search_l1_tap_rings == 64
    d1 = d0.copy()
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, 1, 1, 1.0, d1, nthreads=8)
    st1, res1 = torch.from_numpy(d0.copy()).to(eng.dev), eng.new_result(n)
    eng.align(tp, st1, res1)
    eng.sync()
    assert compare_search(eng.result_to_numpy(res1), st1.cpu().numpy(), params, infos, d1) == 0
    eng.reset_shifts(float(xr), float(yr), 1.0)
    assert eng.search_l1_tap_rings == 0
    st2, res2 = torch.from_numpy(d0.copy()).to(eng.dev), eng.new_result(n)
    eng.align(tp, st2, res2)
    eng.sync()
    assert torch.equal(res2, res) and torch.equal(st2, st)
    eng.close()
