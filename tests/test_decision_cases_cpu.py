"""What tests/test_gpu_decision.py takes from tests/decision_cases.py, asserted without a GPU: every case contains what it is named
for, the restatements agree with independent formulations, and the inputs keep the float64 references away from the roundings
the GPU file leaves open."""
import numpy as np
import pytest

from cryo_ralib_amd import api
from oracle import oracle as orc

import decision_cases as dc

M, F = dc.M, dc.F
# the finalize batches of the GPU file: geometry (nx, ou, xr), record tiles per offset; 129 particles each
FINALIZE_CONFIGS = [(32, 12, 1, 1), (32, 12, 1, 7), (32, 12, 2, 1), (32, 12, 2, 4), (32, 12, 2, 8), (32, 12, 2, 11), (32, 12, 0, 1), (32, 12, 0, 63),
                    (32, 12, 0, 64), (32, 12, 0, 65), (32, 12, 0, 128), (32, 12, 0, 129)]
N_BATCH = 129


def test_record_layouts():
    assert api.CAND_DTYPE.itemsize == 40 and api.CAND_DTYPE.fields["t7"][1] == 12
    assert api.REFINE_DTYPE.itemsize == 120 and api.REFINE_DTYPE.fields["alt"][1] == 36 and api.REFINE_DTYPE["alt"].shape == (7,)
    assert dc.ALTS == 7


@pytest.mark.parametrize("mode", (M, F))
def test_windows(mode):
    """the window of every batch state is search_range's behind the reset / clamp rule (the oracle's own steps), the states cut the
    window on each side and twice, and two of them lie beyond mashi, where the modes differ"""
    geo = dc.Geo(32, 12, 2, mode)
    assert geo.mashi == 3 and geo.win_ring == 12 and geo.nshift == 25
    cut = set()
    for dx, dy in dc.STATES:
        w = geo.window(dx, dy)
        sx, sy = np.float32(dx), np.float32(dy)
        if mode == M:
            if abs(sx) > 3 or abs(sy) > 3:
                sx = sy = np.float32(0)
        else:
            sx, sy = np.clip(sx, -3, 3), np.clip(sy, -3, 3)
        assert (w[0], w[1]) == (sx, sy)
        tx, ty = orc.search_range(32, 12.0, float(sx), 2.0), orc.search_range(32, 12.0, float(sy), 2.0)
        assert w[2:] == (int(tx[0]), int(tx[1]), int(ty[0]), int(ty[1]))
        live = geo.live(w)
        assert live == sorted(live) and len(live) == (w[2] + w[3] + 1) * (w[4] + w[5] + 1) and 12 in live
        cut |= {k for k, v in zip(("left", "right", "low", "high"), w[2:]) if v < 2}
    assert cut == {"left", "right", "low", "high"}
    beyond = [geo.window(dx, dy)[:2] for dx, dy in dc.STATES if abs(dx) > 3 or abs(dy) > 3]
    assert len(beyond) == 2 and (beyond == [(0, 0), (0, 0)] if mode == M else beyond == [(3, 0), (0.25, -3)])


def batch(nx, ou, xr, nrtile, mode):
    geo = dc.Geo(nx, ou, xr, mode)
    cand, state, names = dc.finalize_batch(geo, N_BATCH, nrtile)
    return geo, cand, state, names


def test_record_counts():
    """the in-window record counts of the batches reach 1, 63, 64, 65, 128 and 129 -- through the tiles of a single offset and through
    windows (9 x 7, 16 x 4, 16 x 8) --, and both sides of the engine's rule nshift * nrtile >= 256"""
    counts, by_window = set(), set()
    for nx, ou, xr, nrtile in FINALIZE_CONFIGS:
        geo, cand, state, _ = batch(nx, ou, xr, nrtile, M)
        for p in range(N_BATCH):
            c = len(geo.live(geo.window(*state[p]))) * nrtile
            counts.add(c)
            if xr:
                by_window.add(c)
    assert {1, 63, 64, 65, 128, 129} <= counts and {63, 64, 128} <= by_window
    assert {dc.Geo(32, 12, xr, M).nshift * t >= 256 for _, _, xr, t in FINALIZE_CONFIGS} == {True, False}


@pytest.mark.parametrize("mode", (M, F))
@pytest.mark.parametrize("cfg", FINALIZE_CONFIGS, ids=lambda c: "xr%d-t%d" % (c[2], c[3]))
def test_finalize_scenarios(cfg, mode):
    """every scenario holds what its name says, the restatement's winner is the LAST maximum of the in-window records (an
    independent formulation), and out-of-window records are poisoned"""
    geo, cand, state, names = batch(*cfg, mode)
    nrtile = cfg[3]
    flags = []
    res, st, rl, v64, mag = dc.finalize_ref(geo, cand, state, 0.02, dc.finalize_dup(), flags=flags)
    listed = {int(r["p"]): r for r in rl}
    assert list(rl["p"]) == sorted(rl["p"])
    for p, name in enumerate(names):
        live = geo.live(geo.window(*state[p]))
        vals = cand[p, live]["val"].reshape(-1)
        assert np.all(cand[p, [s for s in range(geo.nshift) if s not in live]]["val"] == dc.POISON)
        ok = ~np.isnan(vals)
        fl, nrec = flags[p], len(vals)
        if ok.any():
            top = np.flatnonzero(ok & (vals == np.nanmax(vals)))
            last = int(top[-1])
            assert (fl["bs"], fl["brt"]) == (live[last // nrtile], last % nrtile) and res[p]["peak"] == vals[last]
            srt = np.sort(vals[ok])
            assert fl["second"] == (srt[-2] if len(srt) > 1 else dc.NEG)
        else:
            assert nrec <= 2 and res[p]["peak"] == dc.NEG and res[p]["shift_idx"] == 0
            continue
        raised = [k for k in ("c3", "tie_bin", "tie_rec", "runner", "copies") if fl[k]]
        if name.startswith("equal") or name == "all-equal":
            assert len(top) == nrec if name == "all-equal" else len(top) >= min(nrec, 2), (name, nrec, top)
            if name == "equal-cross-lane" and nrec > 64:
                assert {int(t) % 64 for t in top[-2:]} == {63, 0} and top[-1] == 64          # the later record in the lower lane
            if name == "equal-same-lane" and nrec > 65:
                assert list(top) == [1, 65]
            if name == "equal-first-last":
                assert top[0] == 0 and top[-1] == nrec - 1
            if name == "equal-adjacent" and nrec > 2:
                assert top[-1] - top[0] == 1
        elif name in ("nan", "nan-first"):
            assert np.isnan(vals).sum() == (1 if name == "nan" else min(2, nrec)) and raised == []
            assert name == "nan" or np.isnan(vals[0])
        elif name in ("bin-1", "bin-maxrin"):
            assert res[p]["angle_bin"] == (1 if name == "bin-1" else geo.maxrin) and raised == []
        elif name == "c3-zero":
            assert fl["c3_value"] == 0.0 and raised == ["c3"] and v64[p, 0] == pytest.approx(orc.ang_n(float(res[p]["angle_bin"]), geo.maxrin), abs=1e-9)
        elif name in ("plain", "second-below-thr"):
            assert raised == [] and p not in listed
            if name == "second-below-thr" and nrec > 1:
                assert fl["second"] == np.nextafter(fl["thr"], np.float32(-np.inf))
        elif name.startswith("flag-"):
            want = {"flag-c3": "c3", "flag-tie-bin": "tie_bin", "flag-tie-rec": "tie_rec", "flag-runner": "runner", "flag-copies": "copies"}[name]
            assert raised == ([want] if want != "tie_rec" or nrec > 1 else []), (name, raised)
            if raised:
                assert listed[p]["nalt"] == {"flag-tie-rec": 1, "flag-runner": 1}.get(name, 0)
        elif name == "second-on-thr" and nrec > 1:
            assert fl["second"] == fl["thr"] and raised == ["tie_rec"] and listed[p]["nalt"] == 1
        elif name == "ten-ties" and nrec > 10:
            assert fl["ntie"] == 10 and listed[p]["nalt"] == 7
            scan = [(s, rt) for s in live for rt in range(nrtile) if (s, rt) != (fl["bs"], fl["brt"]) and cand[p, s, rt]["val"] >= fl["thr"]]
            assert [(int(a["bs"]), int(a["rt"])) for a in listed[p]["alt"]] == scan[:7]
        elif name == "runner-on-alt" and nrec > 3:
            assert fl["ntie"] == 3 and listed[p]["nalt"] == 4 and sorted(listed[p]["alt"]["refmir"][:4])[-1] == (2 | 1 << 16)
        elif name == "runner-on-winner-and-ties" and nrec > 3:
            assert listed[p]["nalt"] == 5 and tuple(listed[p]["alt"][0]) == (fl["bs"], fl["brt"], 1)
    # refine_thr negative: every particle; zero: the c3 condition alone is gone
    assert len(dc.finalize_ref(geo, cand, state, -1.0, dc.finalize_dup())[2]) == N_BATCH
    zero = dc.finalize_ref(geo, cand, state, 0.0, dc.finalize_dup())[2]
    assert set(zero["p"]) == {p for p in listed if [k for k in ("tie_bin", "tie_rec", "runner", "copies") if flags[p][k]]}
    assert len(dc.finalize_ref(geo, cand, state, 0.02, None)[2]) < len(rl) or "flag-copies" not in names


@pytest.mark.parametrize("mode", (M, F))
def test_finalize_reference_stays_off_the_rounding_boundaries(mode):
    """alpha, sx and sy of the restatement differ from the device's by the double cos / sin / atan2 alone: at most 1 % of the float64
    values of all batches lie where one f64 ulp of those (2^-45 of the terms, with room) reaches the float32 rounding"""
    near = total = 0
    for cfg in FINALIZE_CONFIGS:
        geo, cand, state, _ = batch(*cfg, mode)
        _, _, _, v64, mag = dc.finalize_ref(geo, cand, state, 0.02, None, with_list=False)
        near += int(dc.near_f32_boundary(v64, mag).sum())
        total += v64.size
    assert near <= 0.01 * total, (near, total)


def test_layouts():
    geo, cand, state, _ = batch(32, 12, 2, 4, M)
    dense = dc.dense_layout(cand, dc.ent_stride(1, geo.nshift))
    assert dense.shape == (N_BATCH, 28, 4) and np.all(dense[:, 25:]["val"] == dc.POISON) and dense[:, :25].tobytes() == cand.tobytes()
    assert dc.dense_layout(cand, dc.ent_stride(2, geo.nshift)).shape == (N_BATCH, 25, 4)
    live = dc.live_layout(geo, cand, state)
    assert live.shape == (sum(len(geo.live(geo.window(*s))) for s in state), 4) and not np.any(live["val"] == dc.POISON)


def test_dup_tables():
    assert dc.DUP_CASES["none"][1] == [] and sorted(len(g) for g in dc.DUP_CASES["groups-3-7-9"][1]) == [3, 7, 9]
    assert dc.DUP_CASES["stride-256"] == (257, [[0, 256]]) and dc.DUP_CASES["all-equal"][1] == [list(range(11))]
    for name, (nref, groups) in dc.DUP_CASES.items():
        d = dc.dup_table(groups, nref)
        refs = dc.dup_refs(name, 32, 12)
        for r in range(nref):
            same = [r2 for r2 in range(nref) if np.array_equal(refs[r], refs[r2])]
            later = [r2 for r2 in same if r2 > r]
            assert tuple(d[r]) == (same[0], later[0] if later else -1), (name, r)
    assert np.array_equal(dc.finalize_dup(), dc.dup_table([[3, 5]], dc.FINALIZE_NREF))
    refs = dc.finalize_refs(32, 12)
    assert np.array_equal(refs[3], refs[5]) and len({refs[r].tobytes() for r in range(dc.FINALIZE_NREF)}) == dc.FINALIZE_NREF - 1


REPLAY_KEYS = [(32, 12, 2, M, True), (32, 12, 2, F, True), (90, 36, 3, M, False)]


@pytest.mark.parametrize("key", REPLAY_KEYS, ids=("small-mref", "small-reffree", "large-mref"))
def test_replay_cases(key):
    """every replay case: the scan over the listed orientations alone (what the kernel sees) is the literal scan with both
    orientations of every listed pair; every sub-bin fit the kernel may end on is well conditioned (|c3| >= 1e-3 max |b|: the f64
    rounding of the CCF samples, 1e-15 max |b|, then moves the position by less than 1e-11 bins, six decades below the float32 ulp of
    the angle); and each case holds what its name says"""
    rp, cases = dc.replay_cases(*key)
    geo, mode = rp.geo, key[3]
    assert geo.maxrin == (256 if key[0] == 90 else 128) and len(cases) == (13 if key[4] else 3)
    by_name = {}
    for k, (name, rec, cls) in enumerate(cases):
        assert int(rec["p"]) == k
        clsv = None if cls is None else np.full(len(cases), cls, np.int32)
        prior, st0 = dc.replay_prior(rec)
        out, st, v64, changed, w = rp.expected(rec, prior, st0, clsv)
        by_name[name] = (rec, out, changed, w)
        if int(rec["nalt"]) or (cls is None and len(rp.group(int(rec["ref"]))) > 1):
            assert rp.scan(rec, clsv, listed_only=True) == rp.scan(rec, clsv), name
        cands = [(int(rec["bs"]), int(rec["ref"]), int(rec["mirror"]))] + \
                [(int(a["bs"]), int(a["refmir"]) & 0xffff, int(a["refmir"]) >> 16) for a in rec["alt"][:int(rec["nalt"])]]
        for bs, ref, mir in cands:
            r = ref if cls is None else cls
            q = dc.ccf(geo, rp.cref[r], rp.spectrum(k, rec["sxi"], rec["syi"], bs), mir)
            ev = rp.evaluate(k, rec["sxi"], rec["syi"], bs, r)
            assert q.max() == pytest.approx(ev["qm" if mir else "qn"], rel=1e-12) and int(q.argmax()) + 1 == ev["jm" if mir else "jn"]
            assert np.sort(q)[-1] - np.sort(q)[-2] > 1e-9 * q.max()          # the bin is not a tie of the f64 CCF itself
            assert dc.c3_ratio(q, int(q.argmax()) + 1) >= 1e-3, (name, bs, ref, mir)
        if changed:
            assert np.all(st == [rec["sxi"] + geo.shifts[w["bs"]][0], rec["syi"] + geo.shifts[w["bs"]][1]]) and out["peak"] == np.float32(w["q"])
        else:
            assert np.all(st == dc.PRIOR_STATE) and out["peak"] == np.float32(dc.PRIOR["peak"])
    rec, out, changed, w = by_name["nalt0-correct"]
    assert rec["nalt"] == 0 and not changed
    rec, out, changed, w = by_name["nalt1-swapped"]
    assert changed and w["bs"] == rec["alt"][0]["bs"] and (rec["sxi"], rec["syi"]) == (0.5, -1.0)
    rec, out, changed, w = by_name["copies-last-wins"]
    assert w["ref"] == dc.PAIR[1] and not dc.rounded_up(w["q"]) and rec["ref"] == dc.PAIR[0]
    if not key[4]:
        return
    rec, out, changed, w = by_name["copies-first-stays"]
    assert dc.rounded_up(w["q"]) and rec["ref"] == dc.PAIR[1] and w["ref"] == (dc.PAIR[0] if mode == M else dc.PAIR[1])
    rec, out, changed, w = by_name["wrong-jtot"]
    assert changed and rec["nalt"] == 0 and w["jtot"] != rec["jtot"] and (w["bs"], w["ref"], w["mirror"]) == (rec["bs"], rec["ref"], rec["mirror"])
    rec, out, changed, w = by_name["wrong-mirror"]
    assert changed and w["mirror"] == 1 - rec["mirror"] and (w["bs"], w["ref"]) == (rec["bs"], rec["ref"]) == (rec["alt"][0]["bs"], rec["alt"][0]["refmir"] & 0xffff)
    assert not by_name["nalt1-kept"][2] and by_name["nalt1-kept"][0]["nalt"] == 1
    rec, out, changed, w = by_name["nalt7"]
    assert rec["nalt"] == 7 and changed and w["bs"] == rec["alt"][6]["bs"] and len({int(a) & 0xffff for a in rec["alt"]["refmir"]}) == 3
    assert (rec["alt"][1]["bs"], rec["alt"][1]["refmir"] ^ rec["alt"][2]["refmir"]) == (rec["alt"][2]["bs"], 1 << 16)
    rec, out, changed, w = by_name["listed-twice"]
    assert tuple(rec["alt"][0]) == tuple(rec["alt"][1]) and not changed
    # the float ties: a = the earlier offset, b = the later; the doubles and the float rule order them differently
    for want in ("up", "down"):
        rec, out, changed, w = by_name["tie-rounded-" + want]
        k = int(rec["p"])
        a, b = rp.evaluate(k, 0.0, 0.0, int(rec["alt"][0]["bs"]), 0)["qn"], rp.evaluate(k, 0.0, 0.0, int(rec["bs"]), 0)["qn"]
        assert rec["alt"][0]["bs"] < rec["bs"] and np.float32(a) == np.float32(b) and a != b
        assert dc.rounded_up(a) == (want == "up") and (b >= a) == (want == "up")
        by_float = rp.scan(rec, float_peak=True)["bs"]
        by_double = rp.scan(rec, float_peak=False)["bs"]
        assert by_float != by_double and by_double == (rec["bs"] if b >= a else rec["alt"][0]["bs"])
        assert w["bs"] == (by_float if mode == M else by_double)
    rec, out, changed, w = by_name["overflow-72"]
    groups = [rp.group(r) for r in [int(rec["ref"])] + [int(x) & 0xffff for x in rec["alt"]["refmir"]]]
    assert rec["nalt"] == 7 and all(g == dc.GROUP9 for g in groups) and len({int(rec["bs"])} | {int(x) for x in rec["alt"]["bs"]}) == 8
    short = rp.scan(rec, capacity=64)
    assert (w["bs"], w["ref"]) == (int(rec["alt"][6]["bs"]), dc.GROUP9[-1]) and (short["bs"], short["ref"]) == (w["bs"], dc.GROUP9[0])
    rec, out, changed, w = by_name["class-resident-copies"]
    assert not changed and rp.scan(rec)["ref"] == dc.PAIR[1] and out["ref_id"] == dc.PAIR[0]          # with the copies the assignment would move
