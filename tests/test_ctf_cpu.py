"""CPU tests of the CTF phase flip's host side: the float64 statement of the flip against the reference tree's own CTF values
(tests/golden/ctf_ref.npz, make_ctf_pins.py), the parameter tables (.npy, RELION 3.0 / 3.1 .star), sharding and the command
line."""
import argparse
import os

import numpy as np
import pytest

from cryo_ralib_amd import ctf, dist

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctf_ref.npz")


def golden_sets():
    z = np.load(GOLD)
    return [(z["params_%d" % k], int(z["nx_%d" % k]), z["ctf_%d" % k]) for k in range(int(z["count"]))]


def test_golden_covers_the_cases_the_contract_names():
    sets = golden_sets()
    assert len(sets) >= 8
    rows = np.array([s[0] for s in sets])
    assert (rows[:, 2] != rows[:, 3]).any() and (rows[:, 4] != 0).any() and (rows[:, 8] != 0).any() and (rows[:, 7] == 0).any()
    assert any(s[1] % 2 for s in sets) and any(s[1] % 2 == 0 for s in sets)
    assert any(s[0][0] == 2 * s[1] for s in sets)                   # a binned stack


@pytest.mark.parametrize("k", range(8))
def test_flip_statement_has_the_sign_of_the_reference_ctf(k):
    """an unpadded flip of a unit impulse at (0, 0): its spectrum is m, which must be -sign(compute_ctf_np) wherever that is not
    within 1e-6 of zero (the Nyquist column of an even box excepted: irfft2 keeps only the Hermitian part of m there)"""
    row, nx, gold = golden_sets()[k]
    img = np.zeros((1, nx, nx))
    img[0, 0, 0] = 1.0
    out = ctf.flip_reference(img, row[None], pad=False)[0]
    m = np.fft.rfft2(out).real
    g = gold[:, :nx // 2 + 1]
    sel = np.abs(g) > 1e-6
    if nx % 2 == 0:
        sel[:, nx // 2] = False
    assert sel.sum() > nx
    assert (np.sign(m[sel]) == -np.sign(g[sel])).all()
    assert np.allclose(np.abs(m[sel]), 1.0, atol=1e-9)
    # the statement's own CTF grid is the reference's formula on the same frequencies (x = +nx/2 in the Nyquist column of an
    # even box, where the golden grid has fftfreq's -nx/2)
    c = ctf.ctf_grid(row, nx, nx)
    keep = nx // 2 if nx % 2 == 0 else nx // 2 + 1
    assert np.allclose(c[:, :keep], g[:, :keep], atol=1e-9)


def test_flip_with_unit_multiplier_returns_the_input():
    """a CTF that is negative everywhere (m = +1): the 2x padded flip is the identity on the window"""
    rng = np.random.default_rng(3)
    img = rng.standard_normal((2, 20, 20))
    row = np.array([20, 1.0, 0.0, 0.0, 0.0, 300.0, 0.0, 0.5, 0.0])      # df = Cs = 0: ctf = -w everywhere
    out = ctf.flip_reference(img, np.stack([row, row]), pad=True)
    assert np.allclose(out, img, atol=1e-12)


def _star30(path, n, extra_cols=(), extra=lambda i: [], names=None):
    cols = ["_rlnDefocusU", "_rlnDefocusV", "_rlnDefocusAngle", "_rlnVoltage", "_rlnSphericalAberration", "_rlnAmplitudeContrast"]
    cols += list(extra_cols)
    if names is not None:
        cols.append("_rlnImageName")
    with open(path, "w") as f:
        f.write("\n# RELION 3.0\ndata_\n\nloop_\n")
        for i, c in enumerate(cols):
            f.write("%s #%d\n" % (c, i + 1))
        for i in range(n):
            vals = [10000 + i, 9000 + i, 5.0 * i, 300, 2.7, 0.1] + list(extra(i))
            if names is not None:
                vals.append(names[i])
            f.write(" ".join(str(v) for v in vals) + "\n")


def test_npy_table(tmp_path):
    t = np.tile(np.array([64, 1.3, 10000, 9000, 12, 300, 2.7, 0.1, 0], np.float32), (5, 1))
    p = str(tmp_path / "t.npy")
    np.save(p, t)
    assert np.array_equal(ctf.load_table(p, 5, 64), t)
    with pytest.raises(ctf.CtfTableError, match="5 CTF rows for a stack of 4"):
        ctf.load_table(p, 4, 64)
    np.save(p, t[:, :8])
    with pytest.raises(ctf.CtfTableError, match=r"\[N\]\[9\]"):
        ctf.load_table(p, 5, 64)


def test_star_30_with_magnification_rule_and_phase_shift(tmp_path):
    p = str(tmp_path / "p.star")
    _star30(p, 4, ("_rlnDetectorPixelSize", "_rlnMagnification", "_rlnPhaseShift"), lambda i: [14.0, 100000.0, 10.0 * i])
    t = ctf.load_table(p, 4, 90)
    assert t.shape == (4, 9) and t.dtype == np.float32
    assert np.allclose(t[:, 0], 90) and np.allclose(t[:, 1], 1.4)
    assert np.allclose(t[:, 2], [10000, 10001, 10002, 10003]) and np.allclose(t[:, 3], [9000, 9001, 9002, 9003])
    assert np.allclose(t[:, 4], [0, 5, 10, 15]) and np.allclose(t[:, 5:8], [300, 2.7, 0.1]) and np.allclose(t[:, 8], [0, 10, 20, 30])


def test_star_pixel_size_order_and_binned_box(tmp_path):
    p = str(tmp_path / "p.star")
    # _rlnImagePixelSize wins over the magnification rule and over --apix; _rlnImageSize gives D
    _star30(p, 3, ("_rlnImagePixelSize", "_rlnDetectorPixelSize", "_rlnMagnification", "_rlnImageSize"),
            lambda i: [1.1, 14.0, 100000.0, 180])
    t = ctf.load_table(p, 3, 90, apix=3.0)
    assert np.allclose(t[:, 1], 1.1) and np.allclose(t[:, 0], 180)
    # no pixel size in the file: --apix, and without it an error (never parse_ctf_star's 1 A)
    _star30(p, 3)
    assert np.allclose(ctf.load_table(p, 3, 90, apix=2.5)[:, 1], 2.5)
    assert np.allclose(ctf.load_table(p, 3, 90, apix=2.5)[:, 0], 90) and np.allclose(ctf.load_table(p, 3, 90, apix=2.5)[:, 8], 0)
    with pytest.raises(ctf.CtfTableError, match="apix"):
        ctf.load_table(p, 3, 90)
    # the binned box: apix_eff = Apix D / nx, i.e. the frequencies of a 2x binned stack reach twice as far per index
    row = np.array([180, 1.1, 15000, 14000, 20, 300, 2.7, 0.1, 0])
    same = row.copy(); same[0], same[1] = 90, 2.2
    assert np.array_equal(ctf.ctf_grid(row, 90, 90), ctf.ctf_grid(same, 90, 90))


def test_star_31_optics_join(tmp_path):
    p = str(tmp_path / "p.star")
    with open(p, "w") as f:
        f.write("# version 30001\ndata_optics\n\nloop_\n_rlnOpticsGroupName #1\n_rlnOpticsGroup #2\n_rlnVoltage #3\n"
                "_rlnSphericalAberration #4\n_rlnAmplitudeContrast #5\n_rlnImagePixelSize #6\n_rlnImageSize #7\n"
                "opticsGroup1 1 300.0 2.7 0.1 1.06 256\nopticsGroup2 2 200.0 2.0 0.07 0.9 200\n\n"
                "# version 30001\ndata_particles\n\nloop_\n_rlnImageName #1\n_rlnDefocusU #2\n_rlnDefocusV #3\n_rlnDefocusAngle #4\n"
                "_rlnOpticsGroup #5\n_rlnPhaseShift #6\n")
        for i in range(5):
            f.write("%06d@stack.mrcs %d %d %g %d %g\n" % (i + 1, 20000 + i, 19000 + i, 10.0 * i, 1 + i % 2, 0.0))
    t = ctf.load_table(p, 5, 128)
    assert np.allclose(t[:, 5], [300, 200, 300, 200, 300]) and np.allclose(t[:, 6], [2.7, 2.0, 2.7, 2.0, 2.7])
    assert np.allclose(t[:, 7], [0.1, 0.07, 0.1, 0.07, 0.1]) and np.allclose(t[:, 1], [1.06, 0.9, 1.06, 0.9, 1.06])
    assert np.allclose(t[:, 0], [256, 200, 256, 200, 256]) and np.allclose(t[:, 2], 20000 + np.arange(5))


def test_star_count_and_order_mismatches_fail(tmp_path):
    p = str(tmp_path / "p.star")
    _star30(p, 4, ("_rlnImagePixelSize",), lambda i: [1.0], names=["%d@s.mrcs" % k for k in (1, 2, 4, 3)])
    with pytest.raises(ctf.CtfTableError, match="in order"):
        ctf.load_table(p, 4, 64)
    _star30(p, 4, ("_rlnImagePixelSize",), lambda i: [1.0], names=["%d@s.mrcs" % k for k in (1, 2, 3, 4)])
    assert ctf.load_table(p, 4, 64).shape == (4, 9)
    with pytest.raises(ctf.CtfTableError, match="4 CTF rows for a stack of 5"):
        ctf.load_table(p, 5, 64)


def test_out_of_range_rows_fail(tmp_path):
    good = np.array([64, 1.3, 10000, 9000, 12, 300, 2.7, 0.1, 0], np.float64)
    for col, val in [(0, 0), (1, -1), (5, 0), (7, 1.0), (7, -0.1), (3, np.nan), (8, np.inf)]:
        t = np.tile(good, (3, 1))
        t[1, col] = val
        p = str(tmp_path / "t.npy")
        np.save(p, t)
        with pytest.raises(ctf.CtfTableError, match="row 1"):
            ctf.load_table(p, 3, 64)


def test_table_shards_follow_the_particle_shards(tmp_path):
    n = 17
    t = np.zeros((n, 9), np.float32)
    t[:] = [64, 1.3, 10000, 9000, 12, 300, 2.7, 0.1, 0]
    t[:, 2] += np.arange(n)
    p = str(tmp_path / "t.npy")
    np.save(p, t)
    parts = []
    for rank in range(3):
        lo, hi = dist.shard_range(n, 3, rank)
        parts.append(ctf.load_table(p, n, 64, lo=lo, hi=hi))
        assert np.array_equal(parts[-1], t[lo:hi])
    assert np.array_equal(np.concatenate(parts), t)


def test_command_line_accepts_phase_flip_and_still_rejects_ctf(tmp_path):
    from cryo_ralib_amd import cli
    p = str(tmp_path / "t.npy")
    np.save(p, np.zeros((3, 9), np.float32))
    for main, pos in ((cli.main_mref, [str(tmp_path / "nostack.hdf"), str(tmp_path / "norefs.hdf"), str(tmp_path / "out")]),
                      (cli.main_reffree, [str(tmp_path / "nostack.hdf"), str(tmp_path / "out")])):
        with pytest.raises(BaseException) as e:
            main(pos + ["--phase_flip", p, "--apix", "1.2", "--phase_flip_nopad"])
        assert "not implemented" not in str(e.value)          # it fails later: no GPU here, or no stack
        with pytest.raises(SystemExit) as e:
            main(pos + ["--phase_flip", p, "--CTF"])
        assert "not implemented" in str(e.value) and "--CTF" in str(e.value)
    # the shard of the table a rank reads, with the table's own checks
    args = argparse.Namespace(phase_flip=p, apix=None)
    with pytest.raises(SystemExit, match="row 0"):
        cli._ctf_shard(args, 3, 64, 0, 3)
    np.save(p, np.tile(np.array([64, 1.3, 10000, 9000, 12, 300, 2.7, 0.1, 0], np.float32), (3, 1)))
    assert cli._ctf_shard(args, 3, 64, 1, 3).shape == (2, 9)
    assert cli._ctf_shard(argparse.Namespace(phase_flip="", apix=None), 3, 64, 0, 3) is None
