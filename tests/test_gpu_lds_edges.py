"""Kernels at the edge of their LDS plan.  Almost every kernel sizes its dynamic LDS from the geometry on the host; where a kernel
also declares static __shared__ arrays the host rule has to leave room for them.  Every request goes through one helper of the
engine (raise_dynamic_lds: static size of the loaded code object + dynamic <= the device's limit, checked before a launch) and is
kept in a ledger (ra_lds_report / Engine.lds_report).  Here:

  * the sub-bin refinement (refine_winner_kernel, 1280 bytes of static LDS) at the geometries whose ring buffers are within those
    1280 bytes of 160 KB -- below, on and above the edge -- against the CPU oracle, every particle refined;
  * the two routes of the exact kernels (ring buffers in LDS / in global scratch, RALIGN_REFINE_GM=1) against each other, bitwise;
  * the ledger of every engine of the dispatch and option tables: static + dynamic <= limit.

The bar is the one of tests/test_gpu_dispatch.py and test_generic_class_in_the_iteration_loop: identical integer assignments,
CCF peaks within 1e-4, alpha to the ulp.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cryo_ralib_amd import api, synth
from oracle import oracle as orc
from test_gpu_dispatch import CASES as DISPATCH_CASES
from test_gpu_options import FAMILIES, FAMILY_IDS
from test_gpu_parity import compare_search, default_path_only, assert_alpha_equal_to_the_ulp, _log_flips

pytestmark = pytest.mark.gpu

M, F = api.RA_MODE_MREF, api.RA_MODE_REFFREE
LDS, GLOBAL = "refine_winner_kernel<false>", "refine_winner_kernel<true>"
REFINE_STATIC = 1280          # .group_segment_fixed_size of refine_winner_kernel in the gfx950 code object ("LDS ledger")
TABLE = 24                    # bytes per sample of the longest ring: f64 twiddles and CCF samples (RA_EXACT_TABLE_BYTES)

# ring buffers of the exact kernels resident: 8 lcirc + 24 maxrin bytes, + 1280 static, against 163 840
EDGES = [
    # name,                  nx, first, last, skip, mode, n, lcirc, maxrin, route
    ("below-5-63",           140, 5,  63,  1, M, 6, 18528, 512,  LDS),         # 160 512 + 1280 = 161 792
    ("tightest-1-87-skip2",  190, 1,  87,  2, M, 4, 17224, 1024, LDS),         # 162 368 + 1280 = 163 648: 192 bytes to spare
    ("edge-9-64",            140, 9,  64,  1, M, 6, 18816, 512,  GLOBAL),      # 162 816 + 1280 = 164 096 > 163 840
    ("edge-9-64-reffree",    140, 9,  64,  1, F, 6, 18816, 512,  GLOBAL),
    ("edge-18-66",           140, 18, 66,  1, M, 6, 18816, 512,  GLOBAL),
    ("edge-16-88-skip2",     190, 16, 88,  2, M, 4, 17280, 1024, GLOBAL),
    ("edge-14-106-skip3",    224, 14, 106, 3, M, 4, 17280, 1024, GLOBAL),
    ("above-5-64",           140, 5,  64,  1, M, 6, 19040, 512,  GLOBAL),      # 164 608: beyond 160 KB without the static part
]
EDGE_IDS = [c[0] for c in EDGES]
XR, TS = 2, 1.0


def _refine_rows(eng):
    return [r for r in eng.lds_report() if r["kernel"].startswith("refine_winner_kernel")]


def _assert_ledger(rows):
    assert rows, "empty LDS ledger"
    for r in rows:
        assert r["limit_bytes"] >= 64 * 1024, r
        assert r["static_bytes"] + r["dynamic_bytes"] <= r["limit_bytes"], r


@pytest.mark.parametrize("case", EDGES, ids=EDGE_IDS)
def test_refine_at_the_lds_edge(case):
    """every particle through refine_winner_kernel at a geometry whose resident ring buffers end within the kernel's static LDS of
    the 160 KB of a workgroup: the engine creates, picks the route the arithmetic above gives, and agrees with the oracle"""
    default_path_only("RALIGN_FUSED", "RALIGN_GENERIC", "RALIGN_SOLO", "RALIGN_DUO", "RALIGN_REFINE_GM", "RALIGN_REFINE")
    name, nx, ir, ou, rs, mode, n, lcirc, maxrin, route = case
    idx = EDGE_IDS.index(name)
    rg = orc.rings(ir, ou, rs)
    # the case sits where the table says: a change of the ring rule must not move it off its edge unnoticed
    assert (rg.lcirc, rg.maxrin) == (lcirc, maxrin), (rg.lcirc, rg.maxrin)
    assert nx // 2 + 1 - ou - 2 >= XR
    resident = 8 * lcirc + TABLE * maxrin
    assert route == (LDS if resident + REFINE_STATIC <= 160 * 1024 else GLOBAL)
    nref = 3 if mode == M else 1
    refs = synth.make_references(nref, nx, ou, seed=1000 + idx)
    parts, _ = synth.make_particles(refs, n, XR, XR, 0.5, shard=idx, ou=ou)
    mask = orc.model_circle(ou, nx, nx)
    refs_n, cref = orc.prepare_refs(refs, mask, rg)
    d = np.zeros((n, 2), np.float32)
    if mode == M:
        params, infos, _, _ = orc.mref_iteration(parts, cref, rg, XR, XR, TS, d, nthreads=8)
    else:
        params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, XR, XR, TS, (0, 0), d, np.zeros((n, 6), np.float32), nthreads=8)

    eng = api.Engine(nx, ou, XR, XR, TS, nref, mode, first_ring=ir, ring_skip=rs)
    assert (eng.lcirc, eng.maxrin) == (lcirc, maxrin)
    rows = eng.lds_report()
    _assert_ledger(rows)
    rr = _refine_rows(eng)
    assert [r["kernel"] for r in rr] == [route], rr
    assert rr[0]["static_bytes"] == REFINE_STATIC, rr
    assert rr[0]["dynamic_bytes"] == (resident if route == LDS else TABLE * maxrin), rr
    eng.set_refine(-1.0)
    eng.set_references(torch.from_numpy(np.ascontiguousarray(refs_n)).to(eng.dev))
    st, res = eng.new_state(n), eng.new_result(n)
    eng.align(torch.from_numpy(parts).to(eng.dev), st, res)
    eng.sync()
    assert eng.last_refine_count() == n
    r = api.Engine.result_to_numpy(res)
    flips = compare_search(r, st.cpu().numpy(), params, infos, d)
    _log_flips("refine at the LDS edge " + name, n, flips)
    assert flips == 0
    assert_alpha_equal_to_the_ulp(r["alpha"], params[:, 0])
    _assert_ledger(eng.lds_report())
    eng.close()


@pytest.mark.parametrize("nx,ou,path,default", [(90, 36, 1, LDS), (128, 60, 3, LDS), (150, 66, 2, GLOBAL), (140, 61, 2, LDS)],
                         ids=["fused-90-36", "duo-128-60", "generic-150-66", "generic-140-61"])
def test_both_routes_of_the_exact_kernels_agree(nx, ou, path, default, monkeypatch):
    """ring buffers in LDS and in global scratch (RALIGN_REFINE_GM=1) are the same kernels: every field of the result and the state
    bit for bit, and each route at the oracle's bar.  (150 / 66: 66 rings are 173 504 bytes resident, so the default route is the
    global one already and the switch changes nothing there; 140 / 61 is the size-generic geometry that crosses it.)"""
    default_path_only("RALIGN_FUSED", "RALIGN_GENERIC", "RALIGN_SOLO", "RALIGN_DUO", "RALIGN_REFINE_GM", "RALIGN_REFINE")
    nref, n, xr = 3, 16, 2
    refs = synth.make_references(nref, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    rg = orc.rings(1, ou, 1)
    mask = orc.model_circle(ou, nx, nx)
    refs_n, cref = orc.prepare_refs(refs, mask, rg)
    d = np.zeros((n, 2), np.float32)
    params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=8)
    out = {}
    assert default == (LDS if 8 * rg.lcirc + TABLE * rg.maxrin + REFINE_STATIC <= 160 * 1024 else GLOBAL)
    for gm, route in (("0", default), ("1", GLOBAL)):
        monkeypatch.setenv("RALIGN_REFINE_GM", gm)
        eng = api.Engine(nx, ou, xr, xr, 1.0, nref, M)
        assert eng.search_path == path
        assert [r["kernel"] for r in _refine_rows(eng)] == [route]
        _assert_ledger(eng.lds_report())
        eng.set_refine(-1.0)
        eng.set_references(torch.from_numpy(np.ascontiguousarray(refs_n)).to(eng.dev))
        st, res = eng.new_state(n), eng.new_result(n)
        eng.align(torch.from_numpy(parts).to(eng.dev), st, res)
        eng.sync()
        assert eng.last_refine_count() == n
        out[gm] = (api.Engine.result_to_numpy(res), st.cpu().numpy())
        eng.close()
        assert compare_search(out[gm][0], out[gm][1], params, infos, d) == 0
        assert_alpha_equal_to_the_ulp(out[gm][0]["alpha"], params[:, 0])
    assert out["0"][0].dtype.names == out["1"][0].dtype.names
    for k in out["0"][0].dtype.names:
        np.testing.assert_array_equal(out["0"][0][k], out["1"][0][k], err_msg=k)
    np.testing.assert_array_equal(out["0"][1], out["1"][1])


def test_class_references_on_the_global_route(monkeypatch):
    """ra_set_class_references prepares the exact spectra of the classes with the route the engine was planned for: with the ring
    buffers in global scratch the class-resident search agrees bitwise with the LDS route"""
    default_path_only("RALIGN_FUSED", "RALIGN_GENERIC", "RALIGN_REFINE_GM", "RALIGN_REFINE")
    nx, ou, xr, ncls, n = 64, 25, 2, 5, 20
    refs = synth.make_references(ncls, nx, ou)
    parts, _ = synth.make_particles(refs, n, xr, xr, 0.5, ou=ou)
    cls = (np.arange(n) % ncls).astype(np.int32)
    out = {}
    for gm, route in (("0", LDS), ("1", GLOBAL)):
        monkeypatch.setenv("RALIGN_REFINE_GM", gm)
        eng = api.Engine(nx, ou, xr, xr, 1.0, 1, F)
        assert [r["kernel"] for r in _refine_rows(eng)] == [route]
        eng.set_refine(-1.0)
        eng.set_class_references(torch.from_numpy(refs).to(eng.dev))
        st, res = eng.new_state(n), eng.new_result(n)
        eng.align_classes(torch.from_numpy(parts).to(eng.dev), st, res, torch.from_numpy(cls).to(eng.dev))
        eng.sync()
        out[gm] = (api.Engine.result_to_numpy(res), st.cpu().numpy())
        eng.close()
    for k in out["0"][0].dtype.names:
        np.testing.assert_array_equal(out["0"][0][k], out["1"][0][k], err_msg=k)
    np.testing.assert_array_equal(out["0"][1], out["1"][1])


def _ledger_engines():
    for c in DISPATCH_CASES:
        name, nx, ou, ir, rs, xr, yr, ts, nref, n, mode, family = c
        yield pytest.param((nx, ou, xr, yr, ts, nref, mode, ir, rs), {}, id="dispatch-" + name)
    for (nx, ou, xr, nref, n, env, want), name in zip(FAMILIES, FAMILY_IDS):
        yield pytest.param((nx, ou, xr, xr, 1.0, nref, M, 1, 1), env, id="family-" + name)
    for name, nx, ir, ou, rs, mode, n, lcirc, maxrin, route in EDGES:
        yield pytest.param((nx, ou, XR, XR, TS, 3 if mode == M else 1, mode, ir, rs), {}, id="edge-" + name)


@pytest.mark.parametrize("geom,env", list(_ledger_engines()))
def test_ledger_invariant(geom, env, monkeypatch):
    """every kernel an engine configures fits the workgroup with its static LDS; the refine kernel is among them whenever the ring
    layout has an even length (ra_set_refine)"""
    default_path_only("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PAIR", "RALIGN_SOLO", "RALIGN_DUO", "RALIGN_TCROP",
                      "RALIGN_CROP", "RALIGN_TIGHT_RINGS", "RALIGN_REFINE_GM")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nx, ou, xr, yr, ts, nref, mode, ir, rs = geom
    eng = api.Engine(nx, ou, xr, yr, ts, nref, mode, first_ring=ir, ring_skip=rs)
    rows = eng.lds_report()
    _assert_ledger(rows)
    assert len({r["kernel"] for r in rows}) == len(rows)
    rr = _refine_rows(eng)
    if eng.lcirc % 2 == 0:
        assert len(rr) == 1 and rr[0]["static_bytes"] == REFINE_STATIC, rows
    else:
        assert not rr
    eng.close()
