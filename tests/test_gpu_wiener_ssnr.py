"""Half-set FRC and SSNR-weighted Wiener class averages on the device (ra_wiener_frc / ra_wiener_finalize_ssnr): the FRC pass
against the float64 shell sums fed the device's own half sums, the whole path against wiener.ssnr_reference fed the device's
rot_shift2D, reproducibility and chunking with index0, the constant-snr finalize around an SSNR call, argument errors, and the
tool's and drivers' SSNR outputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, cli, ctf, stackio, wiener
from cryo_ralib_amd.mref import MrefAligner, RefFreeAligner

from test_gpu_wiener import _case, _driver_data, _star

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FLOOR = float(np.float32(1e-3))          # the value the device's float argument holds


def _halves(x, prm, lab, k, tab, pad, flipped, chunks=None):
    t = torch.from_numpy(x).to(DEV)
    num2, den2, counts2 = wiener.new_half_sums(k, x.shape[-1], pad, DEV)
    bounds = chunks or [0, len(x)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        wiener.accumulate_halves(t[a:b].contiguous(), prm[a:b], lab[a:b], k, tab[a:b], num2, den2, counts2, index0=a, pad=pad,
                                 flipped=flipped)
    return num2, den2, counts2


def _host(num2, den2, counts2):
    n = num2.double().cpu().numpy()
    return n[..., 0] + 1j * n[..., 1], den2.double().cpu().numpy(), counts2.cpu().numpy()


GEOMETRIES = [(90, True, 60), (64, False, 60), (75, True, 40), (130, True, 24), (256, True, 10),
              (91, True, 24), (113, True, 16), (114, True, 16), (171, False, 12), (172, False, 12)]


@pytest.mark.parametrize("nx,pad,n", GEOMETRIES)
def test_frc_pass_matches_the_shell_sums(nx, pad, n):
    k = 5
    x, prm, lab, tab = _case(n, nx, k, nx + 7 * pad)
    num2, den2, counts2 = _halves(x, prm, lab, k, tab, pad, True)
    f, r = wiener.frc(num2, den2, counts2, nx, pad, 1.5, 3, FLOOR)
    torch.cuda.synchronize()
    want_f, want_r = wiener.frc_from_sums(*_host(num2, den2, counts2), nx, pad, 1.5, 3, FLOOR)
    got_f, got_r = f.cpu().numpy(), r.cpu().numpy()
    assert np.abs(got_f - want_f).max() <= 1e-9
    assert np.all(np.abs(got_r - want_r) <= 1e-6 * np.abs(want_r))
    assert not got_f[k - 2].any() and not got_f[k - 1].any()        # empty, and under min_count
    assert np.abs(got_f[:k - 2]).max() > 0


@pytest.mark.parametrize("nx,pad,n", GEOMETRIES)
def test_device_matches_the_contract(nx, pad, n):
    k = 5
    x, prm, lab, tab = _case(n, nx, k, nx + pad)
    al = api.rot_shift2d(torch.from_numpy(x).to(DEV), prm).cpu().numpy()
    for flipped in (False, True):
        num2, den2, counts2 = _halves(x, prm, lab, k, tab, pad, flipped)
        f, r = wiener.frc(num2, den2, counts2, nx, pad, 1.5, 3, FLOOR)
        got = wiener.finalize_ssnr(num2, den2, counts2, r, nx, pad, 3).cpu().numpy()
        want, wc, wf, _ = wiener.ssnr_reference(x, prm, lab, k, tab, 1.5, FLOOR, pad, flipped, 3, aligned=al)
        assert counts2.sum(1).cpu().numpy().tolist() == wc.tolist()
        assert not got[k - 2].any() and not got[k - 1].any()
        assert np.abs(f.cpu().numpy() - wf).max() <= 1e-5
        for j in range(k - 2):
            assert np.abs(got[j] - want[j]).max() <= 1e-4 * np.abs(want[j]).max(), (flipped, j)


def test_reproducible_and_chunked():
    n, nx, k = 300, 90, 3
    x, prm, lab, tab = _case(n, nx, k, 11)

    def run(chunks=None):
        num2, den2, counts2 = _halves(x, prm, lab, k, tab, True, True, chunks)
        f, r = wiener.frc(num2, den2, counts2, nx, True, 2.0, 1, FLOOR)
        out = wiener.finalize_ssnr(num2, den2, counts2, r, nx, True, 1)
        torch.cuda.synchronize()
        return out.cpu().numpy(), f.cpu().numpy(), r.cpu().numpy(), counts2.cpu().numpy()
    a, b = run(), run()
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    c = run([0, 137, n])                      # an odd offset: the second chunk keeps the global parity through index0
    assert np.array_equal(c[3], a[3])
    assert np.abs(c[0] - a[0]).max() <= 1e-6 * np.abs(a[0]).max()


def test_constant_finalize_is_unchanged_around_an_ssnr_call():
    n, nx, k = 120, 64, 4
    x, prm, lab, tab = _case(n, nx, k, 13)
    t = torch.from_numpy(x).to(DEV)
    num, den, counts = wiener.new_sums(k, nx, True, DEV)
    wiener.accumulate(t, prm, lab, k, tab, num, den, counts, True, True)
    before = wiener.finalize(num, den, counts, nx, True, 2.0, 1).clone()
    num2, den2, counts2 = _halves(x, prm, lab, k, tab, True, True)
    _, r = wiener.frc(num2, den2, counts2, nx, True, 2.0, 1, FLOOR)
    wiener.finalize_ssnr(num2, den2, counts2, r, nx, True, 1)
    after = wiener.finalize(num, den, counts, nx, True, 2.0, 1)
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    # the half sums add up to the constant path's sums
    assert torch.equal(counts2.sum(1), counts)
    assert ((num2[:, 0] + num2[:, 1]) - num).abs().max() <= 1e-5 * num.abs().max()
    assert ((den2[:, 0] + den2[:, 1]) - den).abs().max() <= 1e-5 * den.abs().max()


def test_argument_errors_leave_everything_untouched():
    n, nx, k = 20, 32, 3
    x, prm, lab, tab = _case(n, nx, k, 3)
    num2, den2, counts2 = _halves(x, prm, lab, k, tab, True, True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (num2, den2, counts2)]
    S = nx + 1
    f = torch.full((k, S), 7.0, dtype=torch.float64, device=DEV)
    r = torch.full((k, S), 7.0, device=DEV)
    out = torch.full((k, nx, nx), 7.0, device=DEV)
    L = api.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kk, nxx, pad, snr, fl in [(0, nx, 1, 1.5, 1e-3), (513, nx, 1, 1.5, 1e-3), (k, 1, 1, 1.5, 1e-3), (k, 1025, 1, 1.5, 1e-3),
                                  (k, nx, 2, 1.5, 1e-3), (k, nx, 1, 0.0, 1e-3), (k, nx, 1, -1.0, 1e-3), (k, nx, 1, np.inf, 1e-3),
                                  (k, nx, 1, np.nan, 1e-3), (k, nx, 1, 1.5, 0.0), (k, nx, 1, 1.5, -1e-3), (k, nx, 1, 1.5, np.inf),
                                  (k, nx, 1, 1.5, np.nan)]:
        assert L.ra_wiener_frc(p(num2), p(den2), p(counts2), kk, nxx, pad, snr, 1, fl, p(f), p(r), s) == -1
    ptrs = [p(num2), p(den2), p(counts2), p(f), p(r)]
    for i in range(5):
        a = list(ptrs)
        a[i] = None
        assert L.ra_wiener_frc(a[0], a[1], a[2], k, nx, 1, 1.5, 1, 1e-3, a[3], a[4], s) == -1
    for kk, nxx, pad in [(0, nx, 1), (513, nx, 1), (k, 1, 1), (k, 1025, 1), (k, nx, 2)]:
        assert L.ra_wiener_finalize_ssnr(p(num2), p(den2), p(counts2), p(r), kk, nxx, pad, 1, p(out), s) == -1
    ptrs = [p(num2), p(den2), p(counts2), p(r), p(out)]
    for i in range(5):
        a = list(ptrs)
        a[i] = None
        assert L.ra_wiener_finalize_ssnr(a[0], a[1], a[2], a[3], k, nx, 1, 1, a[4], s) == -1
    with pytest.raises(api.EngineError, match="ra_wiener_frc"):
        wiener.frc(num2, den2, counts2, nx, True, 1.5, 1, 0.0)
    bad = lab.copy()
    bad[4] = k
    with pytest.raises(wiener.WienerError, match="labels"):
        wiener.accumulate_halves(torch.from_numpy(x).to(DEV), prm, bad, k, tab, num2, den2, counts2)
    torch.cuda.synchronize()
    for a, b in zip(snap, (num2, den2, counts2)):
        assert torch.equal(a, b)
    assert (f == 7).all() and (r == 7).all() and (out == 7).all()
    f2, r2 = wiener.frc(num2, den2, counts2, nx, True, 1.5, 1, FLOOR)
    o2 = wiener.finalize_ssnr(num2, den2, counts2, r2, nx, True, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(o2).all() and (f2.abs() <= 1 + 1e-12).all() and o2.abs().max() > 0


def test_tool_writes_what_the_api_computes(tmp_path):
    n, nx, k = 30, 48, 3
    x, prm, lab, tab = _case(n, nx, k, 21)
    tab[:, 0] = nx
    tab[:, 1] = 1.3                            # one pixel size: resolutions in A
    stackio.write_stack(str(tmp_path / "s.hdf"), x)
    order = np.random.default_rng(0).permutation(n)
    stackio.write_text_rows(str(tmp_path / "params.txt"), [(int(i), prm[i, 0], prm[i, 1], prm[i, 2], int(prm[i, 3]), int(lab[i]))
                                                          for i in order])
    _star(str(tmp_path / "t.star"), tab)
    assert wiener.main([str(tmp_path / "s.hdf"), str(tmp_path / "params.txt"), str(tmp_path / "t.star"), str(tmp_path / "o.npy"),
                        "--snr", "3", "--flipped", "--k", str(k), "--ssnr", "--frc", str(tmp_path / "frc.npz")]) == 0
    got = np.load(str(tmp_path / "o.npy"))
    rows = np.loadtxt(str(tmp_path / "params.txt"))
    p2 = np.empty((n, 4))
    p2[rows[:, 0].astype(int)] = rows[:, 1:5]
    want, counts, f, res = api.ssnr_averages(x, p2, lab, k, ctf.load_table(str(tmp_path / "t.star"), n, nx), snr=3.0, flipped=True)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    z = np.load(str(tmp_path / "frc.npz"))
    np.testing.assert_array_equal(z["frc"], f)
    np.testing.assert_array_equal(z["counts"], counts)
    np.testing.assert_array_equal(z["freq"], np.arange(nx + 1) / (2 * nx))
    np.testing.assert_array_equal(z["res_05"], res["res_05"])
    np.testing.assert_array_equal(z["res_0143"], res["res_0143"])
    assert str(z["units"]) == "A" and res["units"] == "A"
    assert np.isnan(res["res_0143"][1])       # the empty class


def _driver_args(tmp_path, out, mref):
    pos = [str(tmp_path / "stack.npy")] + ([str(tmp_path / "refs.npy")] if mref else []) + [str(out)]
    return pos + ["--ou", "18", "--xr", "2", "--maxit", "2", "--ext", "npy", "--phase_flip", str(tmp_path / "ctf.npy"),
                  "--wiener_averages", "--snr", "2"] + ([] if mref else ["--ts", "1"])


def _frc_txt(path):
    with open(path) as fh:
        head = fh.readline()
    return head, np.loadtxt(path, ndmin=2)


def test_mref_driver_writes_the_ssnr_averages(tmp_path):
    parts, refs, tab, ou = _driver_data(tmp_path)
    out = tmp_path / "out"
    assert cli.main_mref(_driver_args(tmp_path, out, True) + ["--wiener_ssnr"]) == 0
    got = np.load(str(out / "multi_ref_wiener_ssnr.npy"))
    rows = np.loadtxt(str(out / "params.txt"))
    prm, lab = np.empty((len(parts), 4)), np.empty(len(parts), np.int64)
    prm[rows[:, 0].astype(int)], lab[rows[:, 0].astype(int)] = rows[:, 1:5], rows[:, 5]
    al = MrefAligner(parts, refs, ou, 2, 2, 1.0, ctf=tab)
    want, counts, _, res = wiener.ssnr_averages(al.particles, prm, lab, len(refs), tab, snr=2.0, flipped=True)
    al.close()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    head, txt = _frc_txt(str(out / "multi_ref_wiener_frc.txt"))
    assert "pixels" in head and res["units"] == "px"           # the table's pixel sizes differ
    np.testing.assert_array_equal(txt[:, 0], np.arange(len(refs)))
    np.testing.assert_array_equal(txt[:, 1], counts)
    np.testing.assert_allclose(txt[:, 2], res["res_05"], rtol=1e-5)
    np.testing.assert_allclose(txt[:, 3], res["res_0143"], rtol=1e-5)
    # the constant-snr output is the one the driver writes without the flag, and nothing new appears without it
    out2 = tmp_path / "out2"
    assert cli.main_mref(_driver_args(tmp_path, out2, True)) == 0
    assert not (out2 / "multi_ref_wiener_ssnr.npy").exists() and not (out2 / "multi_ref_wiener_frc.txt").exists()
    assert sorted(os.listdir(str(out2))) == sorted(f for f in os.listdir(str(out)) if "_ssnr." not in f and "_frc." not in f)
    np.testing.assert_array_equal(np.load(str(out2 / "multi_ref_wiener.npy")), np.load(str(out / "multi_ref_wiener.npy")))


def test_reffree_driver_writes_the_ssnr_average(tmp_path):
    parts, _, tab, ou = _driver_data(tmp_path)
    tab[:, 0], tab[:, 1] = parts.shape[-1], 1.7
    np.save(str(tmp_path / "ctf.npy"), tab)
    out = tmp_path / "out"
    assert cli.main_reffree(_driver_args(tmp_path, out, False) + ["--wiener_ssnr"]) == 0
    got = np.load(str(out / "aqfinal_wiener_ssnr.npy"))
    prm = np.loadtxt(str(out / "initial2Dparams.txt"))
    al = RefFreeAligner(parts, ou, 2, 2, 1.0, ctf=tab)
    want, counts, _, res = wiener.ssnr_averages(al.particles, prm, np.zeros(len(parts), np.int64), 1, tab, snr=2.0, flipped=True)
    al.close()
    assert got.shape == (1,) + parts.shape[1:]
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    head, txt = _frc_txt(str(out / "aqfinal_wiener_frc.txt"))
    assert "(A)" in head and res["units"] == "A"
    assert txt.shape == (1, 4) and txt[0, 1] == len(parts) == counts[0]
    np.testing.assert_allclose(txt[0, 2:], [res["res_05"][0], res["res_0143"][0]], rtol=1e-5)
    assert not (out / "multi_ref_wiener_ssnr.npy").exists()


def test_wiener_ssnr_needs_the_wiener_averages(tmp_path):
    _driver_data(tmp_path, n=8)
    for main, pos in ((cli.main_mref, [str(tmp_path / "stack.npy"), str(tmp_path / "refs.npy"), str(tmp_path / "o")]),
                      (cli.main_reffree, [str(tmp_path / "stack.npy"), str(tmp_path / "o")])):
        with pytest.raises(SystemExit) as e:
            main(pos + ["--phase_flip", str(tmp_path / "ctf.npy"), "--wiener_ssnr"])
        assert e.value.code == 2


def test_wiener_ssnr_refuses_too_many_references_before_aligning(tmp_path):
    _driver_data(tmp_path, n=8)
    np.save(str(tmp_path / "refs513.npy"), np.zeros((513, 48, 48), np.float32))
    out = tmp_path / "o"
    with pytest.raises(SystemExit) as e:
        cli.main_mref([str(tmp_path / "stack.npy"), str(tmp_path / "refs513.npy"), str(out), "--ou", "18", "--maxit", "1",
                       "--ext", "npy", "--phase_flip", str(tmp_path / "ctf.npy"), "--wiener_averages", "--wiener_ssnr"])
    assert e.value.code == 2
    assert not out.exists() or not os.listdir(str(out))
