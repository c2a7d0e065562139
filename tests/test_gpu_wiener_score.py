"""Per-particle agreement scores on the device (ra_wiener_score): against wiener.score_reference fed the device's own rot_shift2D
and class sums, bitwise reproducibility under repetition, splitting and permutation, read-only sums and untouched outputs on
errors, the seeded pruning case end to end through the API and the tool, and the drivers' --wiener_scores file."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cryo_ralib_amd import api, cli, wiener
from cryo_ralib_amd.mref import MrefAligner, RefFreeAligner

from test_gpu_wiener import _case, _driver_data, table
from test_gpu_wiener_ssnr import _driver_args
from test_wiener_score_cpu import junk_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SNR = float(np.float32(1.5))             # the value the device's float argument holds


def _sums(x, prm, lab, k, tab, pad, flipped, halves=False):
    """the device's class sums of the stack; halves: through the half sums and the FRC, with the per-shell term"""
    t = torch.from_numpy(x).to(DEV)
    nx = x.shape[-1]
    if not halves:
        num, den, counts = wiener.new_sums(k, nx, pad, DEV)
        wiener.accumulate(t, prm, lab, k, tab, num, den, counts, pad, flipped)
        return t, num, den, counts, None
    num2, den2, counts2 = wiener.new_half_sums(k, nx, pad, DEV)
    wiener.accumulate_halves(t, prm, lab, k, tab, num2, den2, counts2, 0, pad, flipped)
    _, reg = wiener.frc(num2, den2, counts2, nx, pad, SNR, 1, wiener.SSNR_FLOOR)
    return (t, (num2[:, 0] + num2[:, 1]).contiguous(), (den2[:, 0] + den2[:, 1]).contiguous(),
            counts2.sum(1).to(torch.int32).contiguous(), reg)


def _host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("nx,pad,n", [(90, True, 60), (64, False, 60), (75, True, 40), (130, True, 24), (256, True, 10),
                                     (91, True, 24), (113, True, 16), (114, True, 16), (171, False, 12), (172, False, 12)])
def test_device_matches_the_contract(nx, pad, n):
    """classes: k - 3 populated ones, one of a single member, one empty, one of two members (under min_count = 3).  The bar is
    1e-4 on cc and 1e-4 of sqrt(E F) on each sum; the measured maxima are printed"""
    k = 6
    x, prm, lab, tab = _case(n, nx, k - 1, nx + pad)         # classes 0 .. k - 4 populated, k - 3 empty, k - 2 of two
    lab = lab.copy()
    lab[2] = k - 1                                           # ... and k - 1 of one
    al = _host(api.rot_shift2d(torch.from_numpy(x).to(DEV), prm))
    P = 2 * nx if pad else nx
    worst_cc = worst_sum = 0.0
    for flipped, halves, band, loo in ((False, False, None, True), (True, True, None, True), (True, False, (3, P // 8), True),
                                       (False, True, (0, P // 2), False)):
        t, num, den, counts, reg = _sums(x, prm, lab, k, tab, pad, flipped, halves)
        got = wiener.score(t, prm, lab, k, tab, num, den, counts, SNR, reg, loo, band, pad, flipped, 3)
        want = wiener.score_reference(x, prm, lab, k, tab, _host(num), _host(den), _host(counts), SNR,
                                      None if reg is None else _host(reg).astype(np.float64), loo, band, pad, flipped, 3, aligned=al)
        assert _host(counts).tolist() == np.bincount(lab, minlength=k).tolist()
        unscored = np.bincount(lab, minlength=k)[lab] < 3
        assert unscored[np.isin(lab, [k - 2, k - 1])].all() and (~unscored).sum() >= 3
        assert np.isnan(got["cc"][unscored]).all() and np.isnan(want["cc"][unscored]).all()
        assert np.isfinite(got["cc"][~unscored]).all()
        alone = np.bincount(lab, minlength=k)[lab] == 1       # particle 2 (class k - 1), and whoever the draw of a small n left alone
        assert alone[2]
        if loo:                                               # a class of one has nobody to be compared with
            assert (got["sums"][alone, 0] == 0).all() and (got["sums"][alone, 2] == 0).all() and (got["sums"][alone, 1] > 0).all()
            assert (want["sums"][alone, 1] * want["sums"][alone, 2] == 0).all()
        live = ~alone if loo else np.ones(n, bool)
        norm = np.sqrt(want["sums"][live, 1] * want["sums"][live, 2])
        assert (norm > 0).all()
        e_sum = (np.abs(got["sums"][live] - want["sums"][live]).max(1) / norm).max()
        e_cc = np.abs(got["cc"][~unscored] - want["cc"][~unscored]).max()
        worst_cc, worst_sum = max(worst_cc, e_cc), max(worst_sum, e_sum)
        assert e_cc <= 1e-4 and e_sum <= 1e-4, (flipped, halves, band, loo, e_cc, e_sum)
        assert np.abs(got["scale"][~unscored] - want["scale"][~unscored]).max() <= 1e-4 * np.abs(want["scale"][~unscored]).max()
    print("nx %d pad %d: max |cc - ref| = %.3g, max |sums - ref| / sqrt(E F) = %.3g" % (nx, pad, worst_cc, worst_sum))


def test_bitwise_reproducible_split_and_permuted():
    n, nx, k = 300, 90, 4
    x, prm, lab, tab = _case(n, nx, k, 11)
    for halves in (False, True):
        t, num, den, counts, reg = _sums(x, prm, lab, k, tab, True, True, halves)
        run = lambda idx: wiener.score(t[idx].contiguous(), prm[idx], lab[idx], k, tab[idx], num, den, counts, SNR, reg,
                                       pad=True, flipped=True)["sums"]
        every = np.arange(n)
        a, b = run(every), run(every)
        assert np.array_equal(a, b)
        assert np.array_equal(np.concatenate([run(every[:137]), run(every[137:])]), a)
        perm = np.random.default_rng(3).permutation(n)
        assert np.array_equal(run(perm), a[perm])
        assert np.abs(a[:, 0]).max() > 0


def test_a_call_of_several_chunks_is_bitwise_the_calls_of_its_parts():
    """8 x 8 at 2x: a chunk holds 1 GiB / (16 * 9 * 8 + 8 * 8 * 4) = 762 600 particles, so this call runs the chunk loop twice
    (offsets into the class order, labels, constants and sums of the second chunk); cut elsewhere, into two one-chunk calls, every
    particle's sums are the same doubles"""
    nx, k = 8, 5
    C = (1 << 30) // (16 * 9 * 8 + nx * nx * 4)
    n = C + 3000
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, nx, nx)).astype(np.float32)
    prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.integers(0, 2, n)])
    lab = rng.integers(0, k, n)
    tab = np.tile(table(1, nx, 17).astype(np.float32), (n, 1))
    tab[:, 4] = rng.uniform(-90, 90, n)
    t, num, den, counts, _ = _sums(x, prm, lab, k, tab, True, True)
    run = lambda a, b: wiener.score(t[a:b], prm[a:b], lab[a:b], k, tab[a:b], num, den, counts, SNR, None, pad=True, flipped=True)["sums"]
    whole = run(0, n)
    cut = n // 2
    assert np.array_equal(np.concatenate([run(0, cut), run(cut, n)]), whole)
    assert np.isfinite(whole).all() and (whole[C:, 1] > 0).all() and np.abs(whole[C:, 0]).min() > 0


def test_sums_are_read_only_and_errors_leave_the_output_untouched():
    n, nx, k = 20, 32, 3
    x, prm, lab, tab = _case(n, nx, k, 3)
    t, num, den, counts, _ = _sums(x, prm, lab, k, tab, True, True)
    _, _, _, _, reg = _sums(x, prm, lab, k, tab, True, True, True)
    torch.cuda.synchronize()
    snap = [v.clone() for v in (num, den, counts, reg)]
    wiener.score(t, prm, lab, k, tab, num, den, counts, SNR, None, pad=True, flipped=True)
    wiener.score(t, prm, lab, k, tab, num, den, counts, SNR, reg, False, (2, 9), True, True)
    torch.cuda.synchronize()
    for a, b in zip(snap, (num, den, counts, reg)):
        assert torch.equal(a, b)

    sums = torch.full((n, 3), 7.0, dtype=torch.float64, device=DEV)
    rec = np.zeros(n, api.RESULT_DTYPE)
    rec["alpha"], rec["sx"], rec["sy"], rec["mirror"], rec["ref_id"] = prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3] != 0, lab
    d_rec = torch.from_numpy(rec.view(np.uint8)).to(DEV)
    L = api.load_library()
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(api.float_ptr)

    def call(nn=n, nxx=nx, pad=1, fl=1, kk=k, snr=SNR, r=None, loo=1, lo=1, hi=nx, rec_=d_rec, tab_=tab, ptrs=None):
        a = ptrs or [p(t), p(rec_), p(num), p(den), p(counts), p(sums)]
        return L.ra_wiener_score(a[0], nn, nxx, a[1], h(tab_) if tab_ is not None else None, pad, fl, kk, a[2], a[3], a[4], snr, r, loo,
                                 lo, hi, a[5], s)
    bad_tab = tab.copy()
    bad_tab[5, 2] = np.nan
    for kw in (dict(nn=-1), dict(nxx=1), dict(nxx=1025), dict(pad=2), dict(fl=2), dict(kk=0), dict(kk=1025), dict(loo=2),
               dict(lo=-1), dict(lo=5, hi=4), dict(hi=nx + 1), dict(pad=0, hi=nx // 2 + 1), dict(snr=0.0), dict(snr=-1.0),
               dict(snr=np.inf), dict(snr=np.nan), dict(kk=513, r=p(reg)), dict(tab_=None), dict(tab_=bad_tab)):
        assert call(**kw) == -1, kw
    for i in range(6):
        a = [p(t), p(d_rec), p(num), p(den), p(counts), p(sums)]
        a[i] = None
        assert call(ptrs=a) == -1
    for field, value in (("ref_id", k), ("ref_id", -1), ("alpha", np.nan), ("sx", np.inf)):
        r2 = rec.copy()
        r2[field][7] = value
        assert call(rec_=torch.from_numpy(r2.view(np.uint8)).to(DEV)) == -1
    assert call(nn=0) == 0
    torch.cuda.synchronize()
    assert (sums == 7).all()
    for a, b in zip(snap, (num, den, counts, reg)):
        assert torch.equal(a, b)
    assert call(snr=np.nan, r=p(reg)) == 0                   # with a per-shell term snr is ignored
    torch.cuda.synchronize()
    assert torch.isfinite(sums).all() and (sums != 7).all()
    # the Python layer refuses what it can see before anything is launched
    for kw in (dict(band=(0, nx + 1)), dict(band=(4, 3)), dict(snr=0.0), dict(reg=reg[:, :-1].contiguous()), dict(reg=_host(reg))):
        with pytest.raises(wiener.WienerError):
            wiener.score(t, prm, lab, k, tab, num, den, counts, **kw)
    with pytest.raises(api.EngineError, match="particle 7 has non-finite"):
        bad = prm.copy()
        bad[7, 1] = np.nan
        wiener.score(t, bad, lab, k, tab, num, den, counts)


def test_pruning_end_to_end_through_the_api_and_the_tool(tmp_path):
    x, prm, lab, tab, bad = junk_case()
    x = x.astype(np.float32)
    for ssnr in (False, True):
        res, counts = api.particle_scores(x, prm, lab, 2, tab, snr=2.0, ssnr=ssnr, flipped=True)
        assert counts.tolist() == [60, 60]
        print("ssnr %d: replaced max cc %.3f, members min cc %.3f" % (ssnr, res["cc"][bad].max(), res["cc"][~bad].min()))
        assert np.array_equal(~wiener.select(res["cc"], lab, 2, keep=0.9), bad)
    np.save(str(tmp_path / "s.npy"), x)
    np.save(str(tmp_path / "t.npy"), tab)
    with open(str(tmp_path / "params.txt"), "w") as fh:
        for i in range(len(x)):
            fh.write("%d %r %r %r %d %d\n" % (i, float(prm[i, 0]), float(prm[i, 1]), float(prm[i, 2]), int(prm[i, 3]), int(lab[i])))
    base = [str(tmp_path / "s.npy"), str(tmp_path / "params.txt"), str(tmp_path / "t.npy")]
    opts = ["--snr", "2", "--flipped", "--ssnr", "--frc"]
    assert wiener.main(base + [str(tmp_path / "o.npy")] + opts + [str(tmp_path / "f.npz"), "--scores", str(tmp_path / "sc.npz"),
                                                                   "--keep", "0.9"]) == 0
    z = np.load(str(tmp_path / "sc.npz"))
    assert np.array_equal(~z["keep"], bad)
    np.testing.assert_array_equal(z["cc"], res["cc"])
    np.testing.assert_array_equal(z["sums"], res["sums"])
    assert z["counts"].tolist() == [60, 60] and z["band"].tolist() == [1, 32] and bool(z["leave_one_out"]) and bool(z["ssnr"])
    kept = np.nonzero(~bad)[0]
    want, wc, wf, _ = wiener.ssnr_averages(x[kept], prm[kept], lab[kept], 2, tab[kept], snr=2.0, flipped=True, index=kept)
    got = np.load(str(tmp_path / "o.npy"))
    assert wc.tolist() == [54, 54]
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    f = np.load(str(tmp_path / "f.npz"))
    assert np.abs(f["frc"] - wf).max() <= 1e-6 and f["counts"].tolist() == [54, 54]
    # the halves follow the original index: re-numbering the kept particles gives other half sets
    other, _, of, _ = wiener.ssnr_averages(x[kept], prm[kept], lab[kept], 2, tab[kept], snr=2.0, flipped=True)
    assert np.abs(of - wf).max() > 1e-3
    # without the new flags the tool writes what it wrote before
    assert wiener.main(base + [str(tmp_path / "a.npy")] + opts + [str(tmp_path / "fa.npz")]) == 0
    full, _, ff, _ = wiener.ssnr_averages(x, prm, lab, 2, tab, snr=2.0, flipped=True)
    np.testing.assert_array_equal(np.load(str(tmp_path / "a.npy")), full)
    np.testing.assert_array_equal(np.load(str(tmp_path / "fa.npz"))["frc"], ff)
    assert wiener.main(base + [str(tmp_path / "c.npy"), "--snr", "2", "--flipped"]) == 0
    const, _ = wiener.wiener_averages(x, prm, lab, 2, tab, snr=2.0, flipped=True)
    np.testing.assert_array_equal(np.load(str(tmp_path / "c.npy")), const)
    # scores alone leave OUT as it is without them
    assert wiener.main(base + [str(tmp_path / "d.npy"), "--snr", "2", "--flipped", "--scores", str(tmp_path / "sd.npz"),
                               "--band", "2", "20", "--no_leave_one_out"]) == 0
    np.testing.assert_array_equal(np.load(str(tmp_path / "d.npy")), const)
    zd = np.load(str(tmp_path / "sd.npz"))
    assert "keep" not in zd.files and zd["band"].tolist() == [2, 20] and not bool(zd["leave_one_out"])


def _scores_txt(path, n):
    rows = np.loadtxt(path, ndmin=2)
    assert rows.shape == (n, 4)
    np.testing.assert_array_equal(rows[:, 0], np.arange(n))
    return rows


@pytest.mark.parametrize("ssnr", [False, True])
def test_mref_driver_writes_the_scores(tmp_path, ssnr):
    parts, refs, tab, ou = _driver_data(tmp_path)
    n, k = len(parts), len(refs)
    extra = ["--wiener_ssnr"] if ssnr else []
    out, out2 = tmp_path / "out", tmp_path / "out2"
    assert cli.main_mref(_driver_args(tmp_path, out, True) + extra + ["--wiener_scores"]) == 0
    assert cli.main_mref(_driver_args(tmp_path, out2, True) + extra) == 0
    rows = _scores_txt(str(out / "multi_ref_wiener_scores.txt"), n)
    p = np.loadtxt(str(out / "params.txt"))
    prm, lab = np.empty((n, 4)), np.empty(n, np.int64)
    prm[p[:, 0].astype(int)], lab[p[:, 0].astype(int)] = p[:, 1:5], p[:, 5]
    np.testing.assert_array_equal(rows[:, 1], lab)
    al = MrefAligner(parts, refs, ou, 2, 2, 1.0, ctf=tab)
    want, _ = wiener.particle_scores(al.particles, prm, lab, k, tab, snr=2.0, ssnr=ssnr, flipped=True)
    al.close()
    scored = ~np.isnan(want["cc"])
    assert np.array_equal(np.isnan(rows[:, 2]), ~scored) and scored.sum() > n // 2
    assert np.abs(rows[scored, 2] - want["cc"][scored]).max() <= 1e-4
    # every other output is what the driver writes without the flag
    assert sorted(os.listdir(str(out2))) == sorted(f for f in os.listdir(str(out)) if "_scores." not in f)
    for f in os.listdir(str(out2)):
        with open(str(out / f), "rb") as a, open(str(out2 / f), "rb") as b:
            assert a.read() == b.read(), f


def test_reffree_driver_writes_the_scores(tmp_path):
    parts, _, tab, ou = _driver_data(tmp_path)
    n = len(parts)
    out = tmp_path / "out"
    assert cli.main_reffree(_driver_args(tmp_path, out, False) + ["--wiener_scores"]) == 0
    rows = _scores_txt(str(out / "aqfinal_wiener_scores.txt"), n)
    prm = np.loadtxt(str(out / "initial2Dparams.txt"))
    al = RefFreeAligner(parts, ou, 2, 2, 1.0, ctf=tab)
    want, counts = wiener.particle_scores(al.particles, prm, np.zeros(n, np.int64), 1, tab, snr=2.0, flipped=True)
    al.close()
    assert counts.tolist() == [n] and not rows[:, 1].any()
    assert np.abs(rows[:, 2] - want["cc"]).max() <= 1e-4
    assert np.abs(rows[:, 3] - want["scale"]).max() <= 1e-4 * np.abs(want["scale"]).max()
    assert not (out / "multi_ref_wiener_scores.txt").exists()
