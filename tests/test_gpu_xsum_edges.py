"""The class-sum pass (csrc/ralign_xform.h; rot_shift2D + class sums without the aligned stack: transform_sum_db_kernel,
transform_sum_kernel, transform_sum_tile_kernel, class_sum_combine_kernel) entry by entry at its edges.

No search is run: the result records are written directly (as bench.py::generate_shard does), with poses chosen to hit the
mirror, shifts beyond +-nx (the wrap loops), sources outside the image (the background rule) and angles at multiples of 90
degrees.  Every sum through transform_accumulate must equal, bit for bit, the float32 restatement of the association --
per (class, parity) the member list cut into `nrun` runs at cnt * run // nrun, a run's members added in particle order into
a zero accumulator, the runs added to the sums in run order (test_gpu_parity.py::test_class_sums_are_bitwise_reproducible) --
applied to the aligned images that transform_kernel returns for the same records.

Boxes: up to 99 pixels transform_sum_db_kernel (two image copies in LDS) runs: 32 (one sweep of the workgroup over the image),
33 (two), 64 (four), 90 and 91 (nine sweeps, of which the ninth holds two or three rows, so 13 of 16 waves skip it; even and odd
box), 93 (the last box of nine sweeps in one band), 94 (ten sweeps: the first box of two row bands of five) and 99 (the last
two-copy box, 2 x 81 608 bytes of LDS).  From 100 on transform_sum_kernel (one copy) runs: 100 (two row bands), 130 (three row
bands), 140 and 141 (the last boxes whose padded image fits the LDS: 143 x 143 floats are 81 796 of 81 920 bytes); then
transform_sum_tile_kernel: 142 (the first tile box) and 161 (an odd tile box).

The engine exposes nothing that tells whether the surplus work items of a launch ran as row bands, so that path (taken where
segments x runs leaves a small surplus over whole rounds of resident workgroups and the box has at least two sweeps: the
48 x 48 case below on a 256-CU device; the 32 x 32 case has one sweep and is never cut) is asserted through its sums alone.
"""
import numpy as np
import pytest
import torch

from cryo_ralib_amd import api
from oracle import oracle as orc
from xsum_cases import edge_poses, xs_runs

pytestmark = pytest.mark.gpu

BOXES = [32, 33, 64, 90, 91, 93, 94, 99, 100, 130, 140, 141, 142, 161]
INDEX0 = 3


def edge_records(n, nx, nref, seg_counts, seed):
    """n result records: segment (class, parity) -> member count from `seg_counts` for the small classes, everything else in
    the last class; poses cycle through the edge cases with random ones in between"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, api.RESULT_DTYPE)
    rec["alpha"] = rng.uniform(0.0, 360.0, n).astype(np.float32)
    rec["sx"] = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    rec["sy"] = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    rec["mirror"] = rng.integers(0, 2, n)
    edge = edge_poses(nx)
    for i in range(n):
        if i % 3 != 1:
            a, sx, sy = edge[(i // 3 + i) % len(edge)]
            rec["alpha"][i], rec["sx"][i], rec["sy"][i] = a, sx, sy
    need = {seg: c for seg, c in seg_counts.items()}
    cls = np.full(n, nref - 1, np.int32)
    for i in range(n):
        par = (INDEX0 + i) & 1
        if i % 5 == 2:
            for (c, p), left in need.items():
                if p == par and left > 0:
                    cls[i] = c
                    need[(c, p)] = left - 1
                    break
    assert all(v == 0 for v in need.values()), need
    rec["ref_id"] = cls
    return rec


def restate(aligned, ref_id, nref, nrun, start):
    """the association of transform_sum() in float32, onto `start`"""
    n = aligned.shape[0]
    want = start.copy()
    for c in range(nref):
        for par in range(2):
            mem = [i for i in range(n) if ref_id[i] == c and (INDEX0 + i) % 2 == par]
            for run in range(nrun):
                part = np.zeros(aligned.shape[1:], np.float32)
                for i in mem[len(mem) * run // nrun:len(mem) * (run + 1) // nrun]:
                    part += aligned[i]
                want[c, par] += part
    return want


def sums_and_reference(nx, nref, rec, seed, zero_start=False):
    """(sums of two identical calls, counts, start, aligned images of transform_kernel) for one record list"""
    n = rec.shape[0]
    rng = np.random.default_rng(seed)
    parts = rng.standard_normal((n, nx, nx)).astype(np.float32)
    start = np.zeros((nref, 2, nx, nx), np.float32) if zero_start else rng.standard_normal((nref, 2, nx, nx)).astype(np.float32)
    eng = api.Engine(nx, min(nx // 2 - 4, 30), 1, 1, 1.0, nref, api.RA_MODE_MREF)
    dev = eng.dev
    tp = torch.from_numpy(parts).to(dev)
    res = torch.from_numpy(rec.view(np.int32).reshape(n, 8).copy()).to(dev)
    got = []
    for _ in range(2):
        gs = torch.from_numpy(start.copy()).to(dev)
        gc = torch.zeros(nref, dtype=torch.int32, device=dev)
        eng.transform_accumulate(tp, res, INDEX0, None, gs, gc)
        eng.sync()
        got.append((gs.cpu().numpy(), gc.cpu().numpy()))
    al = torch.zeros((n, nx, nx), device=dev)
    eng.transform_accumulate(tp, res, INDEX0, al, None, None)          # transform_kernel: the aligned images alone
    eng.sync()
    a = al.cpu().numpy()
    eng.close()
    return got, start, a


def skip_under_path_switches():
    import os
    on = [sw for sw in ("RALIGN_XSUM", "RALIGN_XTILE") if os.environ.get(sw) is not None]
    if on:
        pytest.skip("restates the default path's association; %s is set" % ", ".join(on))


# segments of 1, 2, 5, 8 and 3 members: with three runs these are runs of (0, 0, 1), (0, 1, 1), (1, 2, 2), (2, 3, 3) and
# (1, 1, 1) members -- both parities of the image copy in use, for a run's first and last member --; class 2 is empty
SEG_COUNTS = {(0, 0): 1, (0, 1): 2, (1, 0): 5, (1, 1): 8, (3, 0): 3}


@pytest.mark.parametrize("nx", BOXES)
def test_sums_equal_the_restated_association(nx):
    skip_under_path_switches()
    nref, n = 5, 260
    assert xs_runs(n, 2 * nref, nx) == 3
    rec = edge_records(n, nx, nref, SEG_COUNTS, 100 + nx)
    got, start, a = sums_and_reference(nx, nref, rec, 200 + nx)
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], np.bincount(rec["ref_id"], minlength=nref))
    np.testing.assert_array_equal(got[1][1], got[0][1])
    assert got[0][1][2] == 0
    np.testing.assert_array_equal(got[0][0][2], start[2])          # the empty class keeps what it had
    want = restate(a, rec["ref_id"], nref, 3, start)
    np.testing.assert_array_equal(got[0][0], want)


@pytest.mark.parametrize("nx", [33, 90, 93, 94, 99, 100, 161])
def test_fewer_particles_than_eight_per_segment_give_one_run(nx):
    skip_under_path_switches()
    nref, n = 5, 50
    assert n < 8 * 2 * nref and xs_runs(n, 2 * nref, nx) == 1
    rec = edge_records(n, nx, nref, {(0, 0): 1, (1, 1): 2, (3, 0): 3}, 300 + nx)
    got, start, a = sums_and_reference(nx, nref, rec, 400 + nx)
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][0], restate(a, rec["ref_id"], nref, 1, start))


@pytest.mark.parametrize("nx", [32, 48])
def test_twenty_segments_of_fifty_two_runs(nx):
    """1040 work items, every run with members: 16 more than two rounds of 512 resident workgroups (four of 256).  At 48 x 48
    (three sweeps) the surplus items run as three row bands of one sweep each; at 32 x 32 (one sweep) nothing can be cut."""
    skip_under_path_switches()
    nref, n = 10, 8500
    assert xs_runs(n, 2 * nref, nx) == 52
    rng = np.random.default_rng(500 + nx)
    rec = edge_records(n, nx, nref, {}, 600 + nx)
    rec["ref_id"] = rng.integers(0, nref, n)
    cnt = np.zeros((nref, 2), int)
    np.add.at(cnt, (rec["ref_id"], (INDEX0 + np.arange(n)) % 2), 1)
    assert cnt.min() >= 52          # at least one member in every run
    got, start, a = sums_and_reference(nx, nref, rec, 700 + nx)
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], cnt.sum(axis=1))
    np.testing.assert_array_equal(got[0][0], restate(a, rec["ref_id"], nref, 52, start))


@pytest.mark.parametrize("nx", [202, 203])
def test_both_transform_kernels_at_the_lds_edge(nx):
    """transform_kernel keeps the image in LDS up to 202 pixels (163 216 of a workgroup's 163 840 bytes); from 203 on
    transform_generic_kernel reads it from global memory: the one rule of launch_transform (ralign_engine.hip).  On both sides of
    it api.rot_shift2d (no engine) and Engine.transform_accumulate (aligned images alone) give the same bits, and those of the
    oracle's rot_shift2d, which test_oracle.py pins to tests/golden/rot_shift2d_ref.npz."""
    n = 6
    rec = edge_records(n, nx, 1, {}, 800 + nx)
    rng = np.random.default_rng(900 + nx)
    parts = rng.standard_normal((n, nx, nx)).astype(np.float32)
    eng = api.Engine(nx, 30, 1, 1, 1.0, 1, api.RA_MODE_MREF)
    tp = torch.from_numpy(parts).to(eng.dev)
    for mirror in (0, 1):
        rec["mirror"] = mirror
        res = torch.from_numpy(rec.view(np.int32).reshape(n, 8).copy()).to(eng.dev)
        al = torch.zeros((n, nx, nx), device=eng.dev)
        eng.transform_accumulate(tp, res, INDEX0, al, None, None)
        eng.sync()
        prm = np.stack([rec["alpha"], rec["sx"], rec["sy"], rec["mirror"]], axis=1)
        free = api.rot_shift2d(tp, prm)
        torch.cuda.synchronize(eng.dev)
        want = np.stack([orc.rot_shift2d(parts[i], float(rec["alpha"][i]), float(rec["sx"][i]), float(rec["sy"][i]), mirror)
                         for i in range(n)])
        np.testing.assert_array_equal(al.cpu().numpy(), free.cpu().numpy())
        np.testing.assert_array_equal(al.cpu().numpy(), want)
    eng.close()


def test_class_sum_kernel_compacts_its_own_list_beyond_256_mb_of_lists():
    """2 x 1025 member lists of a chunk of 32768 exceed the 256 MB the engine spends on them: class_sum_kernel then runs without
    class_members_wide_kernel, every workgroup compacting its segment's list into LDS (xf_compact), one run.  Aligned images
    and sums of one call against the float32 restatement on those images."""
    nx, nref, n = 32, 1025, 300
    assert 2 * nref * 32768 * 4 > 256 << 20
    rec = edge_records(n, nx, nref, {(0, 0): 1, (7, 1): 3, (1000, 0): 5}, 1100)
    rng = np.random.default_rng(1101)
    parts = rng.standard_normal((n, nx, nx)).astype(np.float32)
    start = rng.standard_normal((nref, 2, nx, nx)).astype(np.float32)
    eng = api.Engine(nx, 12, 1, 1, 1.0, nref, api.RA_MODE_MREF, chunk=32768)
    tp = torch.from_numpy(parts).to(eng.dev)
    res = torch.from_numpy(rec.view(np.int32).reshape(n, 8).copy()).to(eng.dev)
    gs = torch.from_numpy(start.copy()).to(eng.dev)
    gc = torch.zeros(nref, dtype=torch.int32, device=eng.dev)
    al = torch.zeros((n, nx, nx), device=eng.dev)
    eng.transform_accumulate(tp, res, INDEX0, al, gs, gc)
    eng.sync()
    a, got, cnt = al.cpu().numpy(), gs.cpu().numpy(), gc.cpu().numpy()
    eng.close()
    np.testing.assert_array_equal(cnt, np.bincount(rec["ref_id"], minlength=nref))
    want = start.copy()
    for i in range(n):          # one run: every member straight onto the sums, in particle order
        want[rec["ref_id"][i], (INDEX0 + i) % 2] += a[i]
    np.testing.assert_array_equal(got, want)
