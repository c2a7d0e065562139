"""The decision stage of the search, record by record (tests/decision_cases.py builds the inputs and the expected outputs,
tests/test_decision_cases_cpu.py shows that every case holds what it is named for):

finalize_kernel, finalize_wave_kernel, finalize_tail     test_finalize, test_finalize_block_edges, test_finalize_without_a_list
refspec_exact_kernel                                       test_exact_references
ref_hash_kernel, ref_groups_kernel                         test_ref_dup
exact_candidate, the replay of refine_winner_kernel        test_replay
argument checks of the three diagnostic entries            test_bad_arguments

The kernels run through ra_debug_exact_references, ra_debug_finalize and ra_debug_refine with the engine's own geometry, tables and
stream.  Integer fields, peaks, states and the refine list are compared bit for bit; alpha, sx and sy of the finalize tail may be
one float32 ulp off the float64 restatement on at most 1 % of the entries (the device's double cos / sin / atan2)."""
import os

import numpy as np
import pytest
import torch

from cryo_ralib_amd import api

import decision_cases as dc
from test_decision_cases_cpu import FINALIZE_CONFIGS, N_BATCH, REPLAY_KEYS
from test_gpu_parity import assert_alpha_equal_to_the_ulp

pytestmark = pytest.mark.gpu
M, F = dc.M, dc.F
GLOBAL = "refine_winner_kernel<true>"
INT_FIELDS = ("mirror", "ref_id", "angle_bin", "shift_idx")


def make_engine(geo, refs_n, gm=False, refine=0.02):
    """an engine of the geometry with the refinement on and the references set; gm: the exact kernels on global scratch"""
    old = os.environ.get("RALIGN_REFINE_GM")
    if gm:
        os.environ["RALIGN_REFINE_GM"] = "1"
    try:
        eng = api.Engine(**geo.engine_args(len(refs_n)))
    finally:
        if gm:
            if old is None:
                del os.environ["RALIGN_REFINE_GM"]
            else:
                os.environ["RALIGN_REFINE_GM"] = old
    if gm:
        assert [r["kernel"] for r in eng.lds_report() if r["kernel"].startswith("refine_winner")] == [GLOBAL]
    eng.set_refine(refine)
    eng.set_references(torch.from_numpy(np.ascontiguousarray(refs_n, np.float32)).to(eng.dev))
    return eng


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cache = {}

    def get(key, build):
        if key not in cache:
            cache[key] = build()
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def finalize_engine(engines, xr, mode):
    geo = dc.Geo(32, 12, xr, mode)
    eng = engines(("finalize", xr, mode), lambda: make_engine(geo, dc.prepare(geo, dc.finalize_refs(32, 12))[0]))
    return geo, eng


def rec_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def sorted_list(rl):
    return rl[np.argsort(rl["p"], kind="stable")]


def run_finalize(eng, geo, cand, state, nrtile, kernel, live, thr, with_list=True):
    layout = dc.live_layout(geo, cand, state) if live else dc.dense_layout(cand, dc.ent_stride(eng.search_path, geo.nshift))
    res, st, rl = eng.debug_finalize(layout, nrtile, state, kernel, live, thr, with_list)
    return res, st, sorted_list(rl)


def check_finalize(got, want, label):
    """integer fields, peak, state and the whole refine list bit for bit; alpha, sx, sy equal or one ulp off: returns (off, total)"""
    res, st, rl = got
    wres, wst, wrl = want[:3]
    for f in INT_FIELDS:
        assert np.array_equal(res[f], wres[f]), (label, f, np.flatnonzero(res[f] != wres[f])[:8])
    assert rec_bytes(res["peak"]) == rec_bytes(wres["peak"]), label
    assert rec_bytes(st) == rec_bytes(wst), (label, np.flatnonzero((st != wst).any(1))[:8])
    assert len(rl) == len(wrl) and np.array_equal(rl["p"], wrl["p"]), (label, len(rl), len(wrl))
    for f in ("ref", "mirror", "jtot", "bs", "brt", "nalt", "sxi", "syi"):
        assert rec_bytes(rl[f]) == rec_bytes(wrl[f]), (label, f)
    assert rec_bytes(rl["alt"]) == rec_bytes(wrl["alt"]), (label, "alt", [int(r["p"]) for r, w in zip(rl, wrl) if rec_bytes(r["alt"]) != rec_bytes(w["alt"])][:8])
    off = sum(dc.one_ulp_count(res[f], wres[f]) for f in ("alpha", "sx", "sy"))
    return off, 3 * len(res)


@pytest.mark.parametrize("mode", (M, F), ids=("mref", "reffree"))
@pytest.mark.parametrize("cfg", FINALIZE_CONFIGS, ids=lambda c: "xr%d-t%d" % (c[2], c[3]))
def test_finalize(engines, cfg, mode):
    """both kernels and both layouts on the same 129 hand-built particles (every scenario of decision_cases.SCENARIOS at cut, reset
    and clamped windows), with refine_thr negative, zero and positive: each run is the sequential restatement's, the four runs are
    each other's bytes, and a second call repeats the first"""
    xr, nrtile = cfg[2], cfg[3]
    geo, eng = finalize_engine(engines, xr, mode)
    assert eng.num_shifts == geo.nshift and eng.maxrin == geo.maxrin
    refx, dup = eng.debug_exact_references()
    assert np.array_equal(dup, dc.finalize_dup())
    cand, state, names = dc.finalize_batch(geo, N_BATCH, nrtile)
    off = total = 0
    for thr in (-1.0, 0.0, 0.02):
        want = dc.finalize_ref(geo, cand, state, thr, dup)
        runs = {}
        for kernel in (0, 1):
            for live in (0, 1):
                runs[kernel, live] = got = run_finalize(eng, geo, cand, state, nrtile, kernel, live, thr)
                o, t = check_finalize(got, want, (names, thr, kernel, live))
                off, total = off + o, total + t
        first = [rec_bytes(x) for x in runs[0, 0]]
        for key, got in runs.items():
            assert [rec_bytes(x) for x in got] == first, (thr, key)
        assert [rec_bytes(x) for x in run_finalize(eng, geo, cand, state, nrtile, 1, 1, thr)] == first
    print("finalize xr %d, %d tiles, mode %d: %d of %d alpha / sx / sy entries one ulp off the float64 restatement" % (xr, nrtile, mode, off, total))
    assert off <= 0.01 * total


@pytest.mark.parametrize("n", (1, 127, 128))
def test_finalize_block_edges(engines, n):
    """finalize_kernel's blocks of 128 threads (129 particles: test_finalize): n = 1, 127, 128, every particle flagged"""
    geo, eng = finalize_engine(engines, 2, M)
    cand, state, _ = dc.finalize_batch(geo, N_BATCH, 4, seed=3)
    cand, state = cand[:n], state[:n]
    want = dc.finalize_ref(geo, cand, state, -1.0, dc.finalize_dup())
    for kernel in (0, 1):
        for live in (0, 1):
            check_finalize(run_finalize(eng, geo, cand, state, 4, kernel, live, -1.0), want, (n, kernel, live))


def test_finalize_without_a_list(engines):
    """rlist = null: results and states as with a list, and no record"""
    geo, eng = finalize_engine(engines, 2, F)
    cand, state, _ = dc.finalize_batch(geo, N_BATCH, 4)
    want = dc.finalize_ref(geo, cand, state, -1.0, dc.finalize_dup(), with_list=False)
    for kernel in (0, 1):
        for live in (0, 1):
            got = run_finalize(eng, geo, cand, state, 4, kernel, live, -1.0, with_list=False)
            assert len(got[2]) == 0
            check_finalize(got, want, (kernel, live))


# nx, ou, first_ring, ring_skip, interpolation, references, global route
EXACT_CASES = [(32, 12, 1, 1, 0, 3, False), (32, 12, 1, 1, 0, 3, True), (32, 12, 3, 2, 0, 1, False), (32, 12, 2, 1, 1, 3, False),
               (32, 12, 1, 1, 1, 2, True), (90, 36, 1, 1, 0, 3, False), (32, 12, 1, 1, 0, 257, False)]


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "%d-%d-ir%d-rs%d-%s-R%d-%s" % (c[:4] + ("quadri" if c[4] else "bilinear", c[5], "global" if c[6] else "lds")))
def test_exact_references(case):
    """d_refx is the CPU path's prepared reference (Polar2Dm, Frngs, Applyws) bit for bit, as ralign_exact.h claims; the same bytes
    after a second ra_set_references"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nx, ou, ir, rs, interp, nref, gm = case
    geo = dc.Geo(nx, ou, 1, M, first_ring=ir, skip=rs, interp=interp)
    refs_n, cref = dc.prepare(geo, dc.synth.make_references(nref, nx, ou))
    eng = make_engine(geo, refs_n, gm)
    try:
        assert eng.lcirc == geo.lcirc
        refx, dup = eng.debug_exact_references()
        diff = np.flatnonzero((refx.view(np.int32) != cref.view(np.int32)).reshape(-1))
        rel = np.abs(refx.astype(np.float64) - cref).max() / np.abs(cref).max()
        print("exact references %s: %d of %d words differ, largest difference %.3g of the largest coefficient" % (case, len(diff), cref.size, rel))
        assert len(diff) == 0, (len(diff), diff[:8] % geo.lcirc, rel)
        assert np.array_equal(dup, dc.dup_table([], nref))
        eng.set_references(torch.from_numpy(refs_n).to(eng.dev))
        again = eng.debug_exact_references()
        assert rec_bytes(again[0]) == rec_bytes(refx) and np.array_equal(again[1], dup)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(dc.DUP_CASES))
def test_ref_dup(name):
    """ref_dup rows are (first copy, next copy behind this one or -1): no copies, groups of 3, 7 and 9, every reference equal, and a
    pair across the 256-thread stride of ref_groups_kernel"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nref, groups = dc.DUP_CASES[name]
    geo = dc.Geo(32, 12, 1, M)
    eng = make_engine(geo, dc.prepare(geo, dc.dup_refs(name, 32, 12))[0])
    try:
        _, dup = eng.debug_exact_references()
        assert np.array_equal(dup, dc.dup_table(groups, nref)), np.flatnonzero((dup != dc.dup_table(groups, nref)).any(1))
        assert np.array_equal(eng.debug_exact_references()[1], dup)
    finally:
        eng.close()


def run_replay(eng, rp, cases, which):
    """one ra_debug_refine over the records of cases `which` (all with a class, or all without); returns (results, states, expected
    results, expected states)"""
    n = len(cases)
    recs = np.array([cases[k][1] for k in which], api.REFINE_DTYPE)
    cls = None
    if cases[which[0]][2] is not None:
        cls = np.array([c[2] if c[2] is not None else 0 for c in cases], np.int32)
    prior = np.zeros(n, api.RESULT_DTYPE)
    state = np.zeros((n, 2), np.float32)
    want, wstate = prior.copy(), state.copy()
    for k in range(n):
        prior[k], state[k] = dc.replay_prior(cases[k][1])
        want[k], wstate[k] = prior[k], state[k]
    for k in which:
        want[k], wstate[k] = rp.expected(cases[k][1], prior[k], state[k], cls)[:2]
    dres = torch.from_numpy(prior.view(np.int32).reshape(n, 8).copy()).to(eng.dev)
    dst = torch.from_numpy(state.copy()).to(eng.dev)
    eng.debug_refine(torch.from_numpy(rp.parts).to(eng.dev), recs, dst, dres, None if cls is None else torch.from_numpy(cls).to(eng.dev))
    return api.Engine.result_to_numpy(dres), dst.cpu().numpy(), want, wstate


# the global route (RALIGN_REFINE_GM=1) is driven on the small multi-reference geometry
REPLAY_RUNS = [(REPLAY_KEYS[0], False), (REPLAY_KEYS[0], True), (REPLAY_KEYS[1], False), (REPLAY_KEYS[2], False)]


@pytest.mark.parametrize("key,gm", REPLAY_RUNS, ids=("small-mref-lds", "small-mref-global", "small-reffree-lds", "large-mref-lds"))
def test_replay(engines, key, gm):
    """refine_winner_kernel over hand-built lists on real particles against the oracle's literal scan: ref_id, mirror, angle_bin,
    shift_idx and the state identical; peak float32(q[j]) of the oracle or one ulp off; alpha at the bar of
    assert_alpha_equal_to_the_ulp; particles without a record untouched; a second call gives the same bytes"""
    rp, cases = dc.replay_cases(*key)
    eng = engines(("replay", key, gm), lambda: make_engine(rp.geo, rp.refs_n, gm))
    assert np.array_equal(eng.debug_exact_references()[1], dc.replay_dup())
    plain = [k for k, c in enumerate(cases) if c[2] is None]
    resident = [k for k, c in enumerate(cases) if c[2] is not None]
    alpha_got, alpha_want = [], []
    for which in (plain, resident):
        if not which:
            continue
        res, st, want, wstate = run_replay(eng, rp, cases, which)
        for k in range(len(cases)):
            name = cases[k][0]
            for f in INT_FIELDS:
                assert res[f][k] == want[f][k], (name, f, res[k], want[k])
            assert rec_bytes(st[k]) == rec_bytes(wstate[k]), (name, st[k], wstate[k])
            assert dc.one_ulp_count(res["peak"][k:k + 1], want["peak"][k:k + 1]) <= 1, name
            if k not in which:
                assert rec_bytes(res[k]) == rec_bytes(want[k]), name
        same = [k for k in which if res["alpha"][k] == want["alpha"][k]]          # the same angle: sx and sy to the rounding of cos / sin
        dc.one_ulp_count(res["sx"][same], want["sx"][same]); dc.one_ulp_count(res["sy"][same], want["sy"][same])
        alpha_got += list(res["alpha"][which]); alpha_want += list(want["alpha"][which])
        again = run_replay(eng, rp, cases, which)
        assert rec_bytes(again[0]) == rec_bytes(res) and rec_bytes(again[1]) == rec_bytes(st)
    alpha_got, alpha_want = np.array(alpha_got, np.float32), np.array(alpha_want, np.float32)
    print("replay %s %s: %d of %d alpha values are the oracle's bits" % (key, "global" if gm else "lds", int((alpha_got == alpha_want).sum()), len(alpha_got)))
    assert_alpha_equal_to_the_ulp(alpha_got, alpha_want)


def test_bad_arguments(engines):
    """bad arguments and an engine without the refinement: an error code, nothing launched, nothing written"""
    geo, eng = finalize_engine(engines, 2, M)
    cand, state, _ = dc.finalize_batch(geo, 4, 1)
    dense = dc.dense_layout(cand, dc.ent_stride(eng.search_path, geo.nshift))
    for kernel, nrtile in ((2, 1), (0, -1)):
        with pytest.raises(api.EngineError):
            eng.debug_finalize(dense, nrtile, state, kernel, 0, 0.02)
    rec = dc.make_rec(4, 0, 0, 0, 1)          # particle 4 of 4
    dres = torch.full((4, 8), 7, dtype=torch.int32, device=eng.dev)
    dst = torch.full((4, 2), -9.0, device=eng.dev)
    parts = torch.zeros((4, 32, 32), device=eng.dev)
    for bad in (rec, dc.make_rec(0, geo.nshift, 0, 0, 1), dc.make_rec(0, 0, dc.FINALIZE_NREF, 0, 1), dc.make_rec(0, 0, 0, 0, 1, [(0, dc.FINALIZE_NREF, 0)])):
        with pytest.raises(api.EngineError):
            eng.debug_refine(parts, np.array([bad], api.REFINE_DTYPE), dst, dres)
    with pytest.raises(api.EngineError):
        eng.debug_refine(parts, np.array([dc.make_rec(0, 0, 0, 0, 1)], api.REFINE_DTYPE), dst, dres, torch.full((4,), dc.FINALIZE_NREF, dtype=torch.int32, device=eng.dev))
    eng.sync()
    assert torch.all(dres == 7) and torch.all(dst == -9.0)
    off = api.Engine(**geo.engine_args(dc.FINALIZE_NREF))
    try:
        off.set_refine(0.0)
        off.set_references(torch.from_numpy(dc.prepare(geo, dc.finalize_refs(32, 12))[0]).to(off.dev))
        with pytest.raises(api.EngineError):
            off.debug_exact_references()
        with pytest.raises(api.EngineError):
            off.debug_finalize(dense, 1, state, 0, 0, 0.02)
        with pytest.raises(api.EngineError):
            off.debug_refine(parts, np.array([dc.make_rec(0, 0, 0, 0, 1)], api.REFINE_DTYPE), dst, dres)
        off.sync()
        assert torch.all(dres == 7) and torch.all(dst == -9.0)
    finally:
        off.close()
