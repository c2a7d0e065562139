"""What ra_create plans, row by row: the kernel family, the search geometry and the LDS ledger of ~130 engines -- the 37 dispatch
geometries of tests/test_gpu_dispatch.py under the default environment and with RA_INTERP_QUADRI, the geometries each path switch
can move under that switch, and five engines after reset_shifts to a narrower window -- compared exactly with
tests/golden/plan_table.json.  The fixture was recorded on an MI355X from the library BEFORE the planner was gathered into
ralign_plan.h (tests/golden/make_plan_table.py): the test holds the planner to the plans of the code it replaced.  Engines are only
created, never run.  A create that fails is a row too (return code and error text)."""
import ctypes
import json
import os
import sys
import threading

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cryo_ralib_amd import api
from test_gpu_dispatch import CASES, IDS

pytestmark = pytest.mark.gpu

# every switch the plan reads: none of it may leak in from the environment of the run
SWITCHES = ["RALIGN_GENERIC", "RALIGN_FUSED", "RALIGN_TILED", "RALIGN_PAIR", "RALIGN_SOLO", "RALIGN_DUO", "RALIGN_TCROP", "RALIGN_CROP",
            "RALIGN_TIGHT_RINGS", "RALIGN_PACK", "RALIGN_ZONES", "RALIGN_LIVE_OFFSETS", "RALIGN_GCCF_SPLIT", "RALIGN_GCCF_TM",
            "RALIGN_REFINE_GM", "RALIGN_SOLO_JOBS", "RALIGN_GRID", "RALIGN_REFINE", "RALIGN_ATOMIC_SUMS"]

# two geometries with rings of 1024 samples (the split contraction, the exact kernels' rings in global scratch), which the
# dispatch list does not hold:  name, nx, ou, ir, rs, xr, yr, ts, nref, n, mode, family
EXTRA = [("box200-ou88-R50", 200, 88, 1, 1, 2, 2, 1.0, 50, 0, api.RA_MODE_MREF, None),
         ("box256-ou120-R100", 256, 120, 1, 1, 3, 3, 1.0, 100, 0, api.RA_MODE_MREF, None)]
BY_NAME = {c[0]: c for c in CASES + EXTRA}

# (switch, value, the geometries whose plan -- family, geometry or ledger -- it can move)
SWITCH_ROWS = [
    ("RALIGN_GENERIC", "1", ["box93-ou36", "box94-ou36", "box128-ou40-R8", "box100-ou41", "R15"]),
    ("RALIGN_FUSED", "0", ["box93-ou36", "R15", "box94-ou36", "box100-ou30-R17", "box128-ou25-R50"]),
    ("RALIGN_TILED", "0", ["R14", "R15", "R16-crop", "R17-crop", "box100-ou30-R17"]),
    ("RALIGN_TILED", "1", ["R14", "box93-ou36", "box128-ou36", "R16-maxrin128", "reffree-90-36"]),
    ("RALIGN_PAIR", "0", ["box128-ou40-R8", "box100-ou40-reffree", "box128-ou37-R20", "inner-radius-3-pair"]),
    ("RALIGN_SOLO", "0", ["box100-ou41", "box140-ou60", "ring-skip-2-big", "reffree-duo-128-60"]),
    ("RALIGN_DUO", "0", ["box100-ou41", "box140-ou60", "half-pixel-steps-duo"]),
    ("RALIGN_CROP", "0", ["box128-ou40-R8", "box100-ou41", "box94-ou36", "box140-ou60"]),
    ("RALIGN_TCROP", "0", ["box94-ou36", "box128-ou36", "R16-crop", "box128-ou37-tight"]),
    ("RALIGN_TIGHT_RINGS", "0", ["box128-ou37-tight", "box128-ou39-R8", "box128-ou36"]),
    ("RALIGN_PACK", "0", ["box93-ou36", "half-pixel-steps"]),
    ("RALIGN_ZONES", "0", ["box140-ou61", "box160-ou70", "generic-ir3-rs2"]),
    ("RALIGN_LIVE_OFFSETS", "0", ["box140-ou61", "generic-reffree"]),
    ("RALIGN_GCCF_SPLIT", "0", ["box200-ou88-R50", "box256-ou120-R100"]),
    ("RALIGN_REFINE_GM", "1", ["box93-ou36", "box200-ou88-R50"]),
]
# reset_shifts to xr = yr = 1, step 1: one fused, one crop, one duo, one pair and one generic engine
RESET_ROWS = ["box93-ou36", "box94-ou36", "box100-ou41", "box128-ou40-R8", "box140-ou61"]


def row_ids():
    """(id, geometry name, (switch, value) or None, quadri, reset) of every row of the table, in the order it is recorded"""
    rows = [("default/" + n, n, None, False, False) for n in IDS + [e[0] for e in EXTRA]]
    rows += [("%s=%s/%s" % (sw, v, n), n, (sw, v), False, False) for sw, v, names in SWITCH_ROWS for n in names]
    rows += [("quadri/" + n, n, None, True, False) for n in IDS]
    rows += [("reset/" + n, n, None, False, True) for n in RESET_ROWS]
    return rows


def engine_plan(eng):
    return {"search_path": eng.search_path, "search_tiled": int(eng.search_tiled), "search_offsets_per_pass": eng.search_offsets_per_pass,
            "search_skips_offsets": int(eng.search_skips_offsets), "num_shifts": eng.num_shifts, "maxrin": eng.maxrin, "lcirc": eng.lcirc,
            "lds": [[r["kernel"], r["static_bytes"], r["dynamic_bytes"]] for r in eng.lds_report()]}


def plan_row(name, quadri=False, reset=False):
    """the plan of one engine, or {"rc", "error"} of a create (or reset) that fails"""
    _, nx, ou, ir, rs, xr, yr, ts, nref, _, mode, _ = BY_NAME[name]
    lib = api.load_library()
    cfg = api.RaConfig(nx, ir, ou, rs, float(xr), float(yr), float(ts), nref, mode, 0, 0)
    h = ctypes.c_void_p()
    opt = api.RaOptions(api.RA_INTERP_QUADRI, -1)
    rc = lib.ra_create_ex(ctypes.byref(h), ctypes.byref(cfg), ctypes.byref(opt)) if quadri else lib.ra_create(ctypes.byref(h), ctypes.byref(cfg))
    if rc != 0:
        return {"rc": rc, "error": lib.ra_last_error().decode()}
    eng = api.Engine.__new__(api.Engine)           # the accessors of api.Engine on the handle made above
    eng.lib, eng.handle = lib, h
    try:
        if reset:
            rc = lib.ra_reset_shifts(h, 1.0, 1.0, 1.0)
            if rc != 0:
                return {"rc": rc, "error": lib.ra_last_error().decode()}
        return engine_plan(eng)
    finally:
        eng.close()


def build_table(setenv, delenv):
    """every row of the table; setenv(name, value) / delenv(name) change the environment of the process"""
    for name in SWITCHES:
        delenv(name)
    table = {}
    for rid, name, setting, quadri, reset in row_ids():
        if setting:
            setenv(*setting)
        table[rid] = plan_row(name, quadri, reset)
        if setting:
            delenv(setting[0])
    return table


def test_plan_table_is_the_recorded_one(golden_dir, monkeypatch):
    with open(os.path.join(golden_dir, "plan_table.json")) as f:
        want = json.load(f)
    got = build_table(monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False))
    assert list(got) == list(want)
    differ = [rid for rid in want if got[rid] != want[rid]]
    assert not differ, "%d of %d rows differ, first %s:\n  got      %s\n  recorded %s" % (
        len(differ), len(want), differ[0], got[differ[0]], want[differ[0]])
    # the table does exercise what it claims to: every family, failures aside, is in it
    fams = {(r["search_path"], r["search_tiled"], r["search_offsets_per_pass"]) for r in want.values() if "rc" not in r}
    assert {(1, 0, 0), (1, 1, 0), (0, 0, 0), (3, 0, 2), (3, 0, 1), (2, 0, 0)} <= fams


def test_threads_do_not_share_plan_state(monkeypatch):
    """two threads create engines at the same time, one with RA_INTERP_QUADRI (only the size-generic kernels implement it), one
    with the default options at the same geometry, 8 times each: every engine reports the family it reports when created alone"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    api.load_library()

    def family(interp):
        eng = api.Engine(90, 36, 3, 3, 1.0, 4, interp=interp)
        try:
            return eng.search_path
        finally:
            eng.close()

    alone = {i: family(i) for i in (api.RA_INTERP_QUADRI, api.RA_INTERP_BILINEAR)}
    assert alone == {api.RA_INTERP_QUADRI: 2, api.RA_INTERP_BILINEAR: 1}
    got = {api.RA_INTERP_QUADRI: [], api.RA_INTERP_BILINEAR: []}
    start = threading.Barrier(2)

    def work(interp):
        start.wait()
        for _ in range(8):
            got[interp].append(family(interp))

    threads = [threading.Thread(target=work, args=(i,)) for i in got]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == {api.RA_INTERP_QUADRI: [2] * 8, api.RA_INTERP_BILINEAR: [1] * 8}
