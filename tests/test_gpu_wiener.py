"""CTF-corrected (Wiener) class averages on the device (ra_wiener_accumulate / ra_wiener_finalize): against the float64 contract
(wiener.wiener_reference) fed with the device's own rot_shift2D, reproducibility and chunking, errors found on the host and on the
device, recovery of a truth against the plain class average, the tool, and the drivers' --wiener_averages outputs."""
import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, cli, ctf, kmeans, stackio, synth, wiener
from cryo_ralib_amd.mref import MrefAligner, RefFreeAligner

from test_wiener_cpu import masked_corr, physical_case, table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _case(n, nx, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.integers(0, 2, n)])
    lab = rng.integers(0, k - 2, n)          # class k - 2 and k - 1 empty ...
    lab[:2] = k - 1                          # ... then k - 1 gets two members: below min_count = 3
    return x, prm, lab, table(n, nx, seed).astype(np.float32)


def _device(x, prm, lab, k, tab, snr, pad, flipped, min_count, chunks=None):
    t = torch.from_numpy(x).to(DEV)
    num, den, counts = wiener.new_sums(k, x.shape[-1], pad, DEV)
    bounds = chunks or [0, len(x)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        wiener.accumulate(t[a:b].contiguous(), prm[a:b], lab[a:b], k, tab[a:b], num, den, counts, pad, flipped)
    out = wiener.finalize(num, den, counts, x.shape[-1], pad, snr, min_count)
    torch.cuda.synchronize()
    return out.cpu().numpy(), counts.cpu().numpy(), num


@pytest.mark.parametrize("nx,pad,n", [(90, True, 60), (64, False, 60), (75, True, 40), (130, True, 24), (256, True, 10),
                                     (91, True, 24), (113, True, 16), (114, True, 16), (171, False, 12), (172, False, 12)])
def test_device_matches_the_contract(nx, pad, n):
    k = 5
    x, prm, lab, tab = _case(n, nx, k, nx + pad)
    al = api.rot_shift2d(torch.from_numpy(x).to(DEV), prm).cpu().numpy()
    for flipped in (False, True):
        got, counts, _ = _device(x, prm, lab, k, tab, 1.5, pad, flipped, 3)
        want, wc = wiener.wiener_reference(x, prm, lab, k, tab, 1.5, pad, flipped, 3, aligned=al)
        assert counts.tolist() == wc.tolist()
        assert not got[k - 2].any() and not got[k - 1].any()
        for j in range(k - 2):
            assert np.abs(got[j] - want[j]).max() <= 1e-4 * np.abs(want[j]).max(), (flipped, j)


def test_reproducible_and_chunked():
    n, nx, k = 300, 90, 3
    x, prm, lab, tab = _case(n, nx, k, 11)
    a, _, _ = _device(x, prm, lab, k, tab, 2.0, True, True, 1)
    b, _, _ = _device(x, prm, lab, k, tab, 2.0, True, True, 1)
    assert np.array_equal(a, b)
    c, counts, _ = _device(x, prm, lab, k, tab, 2.0, True, True, 1, chunks=[0, 137, n])
    assert counts.tolist() == np.bincount(lab, minlength=k).tolist()
    assert np.abs(c - a).max() <= 1e-6 * np.abs(a).max()


def test_errors_leave_the_sums_untouched_and_the_stream_usable():
    n, nx, k = 20, 32, 3
    x, prm, lab, tab = _case(n, nx, k, 3)
    t = torch.from_numpy(x).to(DEV)
    num, den, counts = wiener.new_sums(k, nx, True, DEV)
    bad_lab = lab.copy()
    bad_lab[7] = k
    with pytest.raises(api.EngineError, match="particle 7 has class label 3"):
        wiener.accumulate(t, prm, bad_lab, k, tab, num, den, counts)
    bad_tab = tab.copy()
    bad_tab[5, 2] = np.nan
    with pytest.raises(api.EngineError, match="CTF row 5"):
        wiener.accumulate(t, prm, lab, k, bad_tab, num, den, counts)
    nan_prm = prm.copy()
    nan_prm[9, 1] = np.nan
    with pytest.raises(api.EngineError, match="particle 9 has non-finite"):
        wiener.accumulate(t, nan_prm, lab, k, tab, num, den, counts)
    torch.cuda.synchronize()
    assert not num.any() and not den.any() and not counts.any()
    wiener.accumulate(t, prm, lab, k, tab, num, den, counts)
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == np.bincount(lab, minlength=k).tolist() and num.abs().max() > 0


def test_recovery_beats_the_plain_class_average():
    fl, prm, tab, truth, mask = physical_case(2000, seed=8)
    lab = np.zeros(len(fl), np.int64)
    avg, _ = wiener.wiener_averages(fl.astype(np.float32), prm, lab, 1, tab, snr=2.0, flipped=True)
    plain = kmeans.class_averages(fl.astype(np.float32), prm, lab, 1, 26, preprocess=False)
    c_w, c_p = masked_corr(avg[0].astype(np.float64), truth, mask), masked_corr(plain[0].astype(np.float64), truth, mask)
    print("1 - corr with truth: wiener %.3g, class average %.3g" % (1 - c_w, 1 - c_p))
    assert 1 - c_w < 0.5 * (1 - c_p)


def _star(path, tab):
    with open(path, "w") as f:
        f.write("data_\nloop_\n_rlnDefocusU\n_rlnDefocusV\n_rlnDefocusAngle\n_rlnVoltage\n_rlnSphericalAberration\n"
                "_rlnAmplitudeContrast\n_rlnPhaseShift\n_rlnImagePixelSize\n")
        for r in tab:
            f.write("%r %r %r %r %r %r %r %r\n" % tuple(float(v) for v in (r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[1])))


def test_tool_writes_what_the_api_computes(tmp_path):
    n, nx, k = 30, 48, 3
    x, prm, lab, tab = _case(n, nx, k, 21)
    tab[:, 0] = nx
    stackio.write_stack(str(tmp_path / "s.hdf"), x)
    order = np.random.default_rng(0).permutation(n)
    stackio.write_text_rows(str(tmp_path / "params.txt"), [(int(i), prm[i, 0], prm[i, 1], prm[i, 2], int(prm[i, 3]), int(lab[i]))
                                                          for i in order])
    _star(str(tmp_path / "t.star"), tab)
    assert wiener.main([str(tmp_path / "s.hdf"), str(tmp_path / "params.txt"), str(tmp_path / "t.star"), str(tmp_path / "o.npy"),
                        "--snr", "3", "--flipped", "--k", str(k)]) == 0
    got = np.load(str(tmp_path / "o.npy"))
    rows = np.loadtxt(str(tmp_path / "params.txt"))
    p2 = np.empty((n, 4))
    p2[rows[:, 0].astype(int)] = rows[:, 1:5]
    want, _ = api.wiener_averages(x, p2, lab, k, ctf.load_table(str(tmp_path / "t.star"), n, nx), snr=3.0, flipped=True)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def _driver_data(tmp_path, n=80, nx=48, ou=18, nref=3):
    refs = synth.make_references(nref, nx, ou, seed=9)
    parts, _ = synth.make_particles(refs, n, 2, 2, 0.5, ou=ou)
    tab = table(n, nx, 31).astype(np.float32)
    np.save(str(tmp_path / "stack.npy"), parts)
    np.save(str(tmp_path / "refs.npy"), refs)
    np.save(str(tmp_path / "ctf.npy"), tab)
    return parts, refs, tab, ou


def test_mref_driver_writes_the_wiener_averages(tmp_path):
    parts, refs, tab, ou = _driver_data(tmp_path)
    out = tmp_path / "out"
    assert cli.main_mref([str(tmp_path / "stack.npy"), str(tmp_path / "refs.npy"), str(out), "--ou", str(ou), "--xr", "2",
                          "--maxit", "2", "--ext", "npy", "--phase_flip", str(tmp_path / "ctf.npy"), "--wiener_averages",
                          "--snr", "2"]) == 0
    got = np.load(str(out / "multi_ref_wiener.npy"))
    rows = np.loadtxt(str(out / "params.txt"))
    prm, lab = np.empty((len(parts), 4)), np.empty(len(parts), np.int64)
    prm[rows[:, 0].astype(int)], lab[rows[:, 0].astype(int)] = rows[:, 1:5], rows[:, 5]
    al = MrefAligner(parts, refs, ou, 2, 2, 1.0, ctf=tab)           # the driver's particles: masked mean subtracted, then flipped
    want, _ = wiener.wiener_averages(al.particles, prm, lab, len(refs), tab, snr=2.0, flipped=True)
    al.close()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_reffree_driver_writes_the_wiener_average(tmp_path):
    parts, _, tab, ou = _driver_data(tmp_path)
    out = tmp_path / "out"
    assert cli.main_reffree([str(tmp_path / "stack.npy"), str(out), "--ou", str(ou), "--xr", "2", "--ts", "1", "--maxit", "2",
                             "--ext", "npy", "--phase_flip", str(tmp_path / "ctf.npy"), "--wiener_averages", "--snr", "2"]) == 0
    got = np.load(str(out / "aqfinal_wiener.npy"))
    prm = np.loadtxt(str(out / "initial2Dparams.txt"))
    al = RefFreeAligner(parts, ou, 2, 2, 1.0, ctf=tab)
    want, _ = wiener.wiener_averages(al.particles, prm, np.zeros(len(parts), np.int64), 1, tab, snr=2.0, flipped=True)
    al.close()
    assert got.shape == (1,) + parts.shape[1:]
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_wiener_averages_need_the_phase_flip(tmp_path):
    _driver_data(tmp_path, n=8)
    for main, pos in ((cli.main_mref, [str(tmp_path / "stack.npy"), str(tmp_path / "refs.npy"), str(tmp_path / "o")]),
                      (cli.main_reffree, [str(tmp_path / "stack.npy"), str(tmp_path / "o")])):
        with pytest.raises(SystemExit) as e:
            main(pos + ["--wiener_averages"])
        assert e.value.code == 2
        with pytest.raises(SystemExit) as e:
            main(pos + ["--wiener_averages", "--phase_flip", str(tmp_path / "ctf.npy"), "--snr", "0"])
        assert e.value.code == 2
