"""Timing of the CTF phase flip (api.phase_flip / ra_phase_flip) on one GPU; prints one JSON line.

Rows: 50 000 x 90^2 with pad 2 and 1, 5 000 x 130^2, 32 768 x 100^2, 8 192 x 256^2 (pad 2 unless named).  Per row: ms per call
(median of --reps device-event timings after --warmup calls), particles/s, the HBM floor (2 n nx^2 4 B -- every image read and
written once -- at the bandwidth a device-to-device copy of the same stack achieves, measured here the same way), and the same flip with torch.fft (pad, rfft2,
multiply by the precomputed multiplier, irfft2, crop) on the same GPU as a comparison only; the multiplier of that route is
computed outside its timing, so it is a lower bound on what a torch.fft user pays.

    python scripts/bench_phase_flip.py [--reps 10] [--warmup 2] [--rows 90p2,90p1,130,100,256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import api  # noqa: E402

ROWS = {"90p2": (50000, 90, True), "90p1": (50000, 90, False), "130": (5000, 130, True), "100": (32768, 100, True),
        "256": (8192, 256, True)}


def table(n, nx, seed=0):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 9), np.float32)
    t[:] = [nx, 1.5, 0, 0, 0, 300.0, 2.7, 0.1, 0.0]
    t[:, 2] = rng.uniform(10000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(0, 2000, n)
    t[:, 4] = rng.uniform(-90, 90, n)
    return t


def torch_multiplier(tab, nx, P, dev):
    """m = -sign(ctf) on the rfft2 grid, [n][P][P/2 + 1] float32, in float64 torch arithmetic"""
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
    c = torch.sqrt(1 - w ** 2) * torch.sin(g) - w * torch.cos(g)
    return torch.where(c > 0, -1.0, 1.0).float()


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no_torch", action="store_true", help="skip the torch.fft comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_phase_flip needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    for name in args.rows.split(","):
        n, nx, pad = ROWS[name]
        P, o = (2 * nx if pad else nx), (nx // 2 if pad else 0)
        tab = table(n, nx)
        x = torch.randn((n, nx, nx), device=dev)
        work = x.clone()
        ms = time_ms(lambda: api.phase_flip(work, tab, pad), args.reps, args.warmup)
        dst = torch.empty_like(x)
        ms_copy = time_ms(lambda: dst.copy_(x), args.reps, args.warmup)
        del dst
        nbytes = 2 * n * nx * nx * 4
        row = {"row": name, "n": n, "nx": nx, "pad": 2 if pad else 1, "ms": round(ms, 3), "particles_per_s": round(n / ms * 1e3),
               "hbm_floor_ms": round(ms_copy, 3), "copy_gb_per_s": round(nbytes / ms_copy / 1e6, 1)}
        if not args.no_torch:
            # batches that keep the padded float32 image and its spectrum within a few GB
            bt = max(1, min(n, (2 << 30) // (P * P * 4 * 3)))
            ms_t = 0.0
            for lo in range(0, n, bt):
                hi = min(n, lo + bt)
                m = torch_multiplier(tab[lo:hi], nx, P, dev)
                xs = x[lo:hi]

                def tf():
                    big = torch.zeros((hi - lo, P, P), device=dev)
                    big[:, o:o + nx, o:o + nx] = xs
                    return torch.fft.irfft2(torch.fft.rfft2(big) * m, s=(P, P))[:, o:o + nx, o:o + nx].contiguous()
                ms_t += time_ms(tf, max(1, args.reps // 2), 1)
                if lo == 0:
                    ref = tf()
                    got = x[lo:hi].clone()
                    api.phase_flip(got, tab[lo:hi], pad)
                    row["max_rel_diff_vs_torch"] = float((got - ref).abs().max() / ref.abs().max())
                del m
            row["torch_fft_ms"] = round(ms_t, 3)
        res["rows"].append(row)
        del x, work
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
