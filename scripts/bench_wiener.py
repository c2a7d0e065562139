"""Timing of the CTF-corrected (Wiener) class averages (ra_wiener_accumulate + ra_wiener_finalize) on one GPU; prints one JSON line.

Rows (the phase flip's): 50 000 x 90^2 at 2x with k = 50 and k = 1, 32 768 x 100^2, 5 000 x 130^2, 8 192 x 256^2 (2x, k = 50).
Per row, on the same stack: ms per accumulate + finalize (median of --reps device-event timings after --warmup calls), a torch.fft
route (ra_rot_shift2d, pad, rfft2, weights, index_add_ per class, irfft2, crop; the CTF of that route is computed outside its
timing, so it is a lower bound on what a torch.fft user pays), ra_phase_flip of the stack, and a device-to-device copy of the
stack (the HBM floor of reading it once).  The torch route runs in batches that keep its arrays within a few GB.

    python scripts/bench_wiener.py [--reps 5] [--warmup 1] [--rows 90k50,90k1,100,130,256] [--no_torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import api, wiener  # noqa: E402

ROWS = {"90k50": (50000, 90, 50), "90k1": (50000, 90, 1), "100": (32768, 100, 50), "130": (5000, 130, 50), "256": (8192, 256, 50)}


def table(n, nx, seed=0):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 9), np.float32)
    t[:] = [nx, 1.5, 0, 0, 0, 300.0, 2.7, 0.1, 0.0]
    t[:, 2] = rng.uniform(10000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(0, 2000, n)
    t[:, 4] = rng.uniform(-90, 90, n)
    return t


def torch_ctf(tab, nx, P, dev):
    """ctf_np of the aligned-frame table on the rfft2 grid, [n][P][P/2 + 1] float32, in float64 torch arithmetic"""
    t = torch.from_numpy(tab.astype(np.float64)).to(dev)
    D, apix, dfu, dfv, ang, volt, cs, w, ps = [t[:, i, None, None] for i in range(9)]
    a = apix * D / nx
    x = torch.arange(P // 2 + 1, device=dev, dtype=torch.float64)[None, None, :] / (P * a)
    y = (torch.fft.fftfreq(P, device=dev, dtype=torch.float64) * P)[None, :, None] / (P * a)
    volt = volt * 1000
    lam = 12.2639 / torch.sqrt(volt + 0.97845e-6 * volt ** 2)
    s2 = x ** 2 + y ** 2
    df = .5 * (dfu + dfv + (dfu - dfv) * torch.cos(2 * (torch.atan2(y, x) - ang * np.pi / 180)))
    g = 2 * np.pi * (-.5 * df * lam * s2 + .25 * cs * 1e7 * lam ** 3 * s2 ** 2) - ps * np.pi / 180
    return (torch.sqrt(1 - w ** 2) * torch.sin(g) - w * torch.cos(g)).float()


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no_torch", action="store_true", help="skip the torch.fft comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wiener needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "snr": 2.0, "flipped": True, "rows": []}
    for name in args.rows.split(","):
        n, nx, k = ROWS[name]
        P, o, H = 2 * nx, nx // 2, nx + 1
        rng = np.random.default_rng(1)
        tab = table(n, nx)
        prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.integers(0, 2, n)])
        lab = rng.integers(0, k, n)
        x = torch.randn((n, nx, nx), device=dev)
        num, den, counts = wiener.new_sums(k, nx, True, dev)
        out = torch.empty((k, nx, nx), device=dev)

        def run():
            num.zero_(); den.zero_(); counts.zero_()
            wiener.accumulate(x, prm, lab, k, tab, num, den, counts, True, True)
            wiener.finalize(num, den, counts, nx, True, 2.0, 1, out)
        ms = time_ms(run, args.reps, args.warmup)
        work = x.clone()
        ms_flip = time_ms(lambda: api.phase_flip(work, tab, True), args.reps, args.warmup)
        del work
        dst = torch.empty_like(x)
        ms_copy = time_ms(lambda: dst.copy_(x), args.reps, args.warmup)
        del dst
        row = {"row": name, "n": n, "nx": nx, "pad": 2, "k": k, "ms": round(ms, 3), "particles_per_s": round(n / ms * 1e3),
               "phase_flip_ms": round(ms_flip, 3), "copy_ms": round(ms_copy, 3),
               "spectra_gb": round(n * P * H * 8 * 2 / 1e9, 2)}
        if not args.no_torch:
            bt = max(1, min(n, (2 << 30) // (P * H * 8 * 4)))
            tab_al = wiener.aligned_table(tab, prm).astype(np.float32)
            cs = [torch_ctf(tab_al[lo:lo + bt], nx, P, dev) for lo in range(0, n, bt)]
            lab_t = torch.from_numpy(lab).to(dev)

            def tf():
                al = api.rot_shift2d(x, prm)
                N = torch.zeros((k, P, H), dtype=torch.complex64, device=dev)
                Dn = torch.zeros((k, P, H), device=dev)
                for b, lo in enumerate(range(0, n, bt)):
                    hi = min(n, lo + bt)
                    big = torch.zeros((hi - lo, P, P), device=dev)
                    big[:, o:o + nx, o:o + nx] = al[lo:hi]
                    c = cs[b]
                    N.index_add_(0, lab_t[lo:hi], torch.fft.rfft2(big) * c.abs())
                    Dn.index_add_(0, lab_t[lo:hi], c * c)
                return torch.fft.irfft2(N / (Dn + 0.5), s=(P, P))[:, o:o + nx, o:o + nx]
            ms_t = time_ms(tf, max(1, args.reps // 2), 1)
            ref = tf()
            row["torch_fft_ms"] = round(ms_t, 3)
            row["max_rel_diff_vs_torch"] = float((out - ref).abs().max() / ref.abs().max())
            del cs, ref
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del x, num, den, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
