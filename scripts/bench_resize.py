"""Timing of Fourier resizing (api.fourier_resize / ra_fourier_resize) on one GPU; prints one JSON line.

Rows: 50 000 x 360^2 -> 90, 50 000 x 180^2 -> 90, 16 384 x 512^2 -> 128, 4 096 x 1024^2 -> 256 and one upsampling row,
512 x 90^2 -> 360.  Per row: ms per call (median of --reps device-event timings after --warmup calls), particles/s, and the HBM
floor: the bytes read and written (n (nx^2 + m^2) 4 B, every image read once and its output written once) at the bandwidth a
device-to-device copy of the input stack achieves, measured here the same way.  As comparisons only, on the same GPU: the
torch.fft route (rfft2, the centring as a phase ramp, crop / fold or pad / split, irfft2) and the torch.matmul route (A x A^T
as two batched matmuls with resize.operator rounded to float32), both in batches that keep their intermediates within a few GB;
each row also records the largest difference of either route from the kernel, relative to max |y|.

    python scripts/bench_resize.py [--reps 10] [--warmup 2] [--rows 360,180,512,1024,up90]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import api, resize  # noqa: E402

ROWS = {"360": (50000, 360, 90), "180": (50000, 180, 90), "512": (16384, 512, 128), "1024": (4096, 1024, 256),
        "up90": (512, 90, 360)}
TORCH_BYTES = 3 << 30           # bound on one batch's float32 input of the torch routes


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


def axis_map(nx, m, half_axis):
    """(source index, target index, complex weight) of one axis of the centred resize on the (r)fft grid: the input centre
    nx//2 and the output centre m//2 become a phase ramp; crop with +-m/2 folded (m < nx) or pad with an even nx's Nyquist
    split (m > nx); times m / nx.  half_axis: the rfft axis (k >= 0 only; a fold or split there is the factor 2 or 1/2 on the
    bin the c2r transform reads as real)."""
    src, tgt, w = [], [], []
    ks = range(0, nx // 2 + 1) if half_axis else [((a + nx // 2) % nx) - nx // 2 for a in range(nx)]
    for k in ks:
        if 2 * abs(k) > min(nx, m) and not (m > nx and 2 * abs(k) == nx):
            continue
        ph_in = complex(math.cos(2 * math.pi * k * (nx // 2) / nx), math.sin(2 * math.pi * k * (nx // 2) / nx))
        targets = [(k, 1.0)]
        if m < nx and m % 2 == 0 and 2 * abs(k) == m:
            targets = [(m // 2, 2.0 if half_axis else 1.0)]           # fold: both signs land on the m/2 bin
        elif m > nx and nx % 2 == 0 and 2 * abs(k) == nx:
            targets = [(nx // 2, 0.5)] if half_axis else [(-nx // 2, 0.5), (nx // 2, 0.5)]
        for kt, f in targets:
            ph_out = complex(math.cos(2 * math.pi * kt * (m // 2) / m), -math.sin(2 * math.pi * kt * (m // 2) / m))
            src.append(k % nx)
            tgt.append(kt % m)
            w.append(f * ph_in * ph_out * m / nx)
    return src, tgt, w


def torch_fft_route(nx, m, dev):
    rs, rt, rw = (torch.tensor(v, device=dev) for v in axis_map(nx, m, False))
    cs, ct, cw = (torch.tensor(v, device=dev) for v in axis_map(nx, m, True))
    rw, cw = rw.to(torch.complex64), cw.to(torch.complex64)

    def run(x):
        X = torch.fft.rfft2(x)
        R = torch.zeros((x.shape[0], m, X.shape[2]), dtype=X.dtype, device=dev)
        R.index_add_(1, rt, X[:, rs, :] * rw[None, :, None])
        Y = torch.zeros((x.shape[0], m, m // 2 + 1), dtype=X.dtype, device=dev)
        Y.index_add_(2, ct, R[:, :, cs] * cw[None, None, :])
        return torch.fft.irfft2(Y, s=(m, m))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no_torch", action="store_true", help="skip the torch.fft and torch.matmul comparisons")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    for name in args.rows.split(","):
        n, nx, m = ROWS[name]
        x = torch.randn((n, nx, nx), device=dev)
        y = torch.empty((n, m, m), device=dev)
        ms = time_ms(lambda: api.fourier_resize(x, m, out=y), args.reps, args.warmup)
        dst = torch.empty_like(x)
        ms_copy = time_ms(lambda: dst.copy_(x), args.reps, args.warmup)
        del dst
        rate = 2 * n * nx * nx * 4 / ms_copy / 1e6                        # GB/s of the copy
        nbytes = n * (nx * nx + m * m) * 4
        row = {"row": name, "n": n, "nx": nx, "m": m, "ms": round(ms, 3), "particles_per_s": round(n / ms * 1e3),
               "hbm_floor_ms": round(nbytes / rate / 1e6, 3), "copy_gb_per_s": round(rate, 1),
               "mflop_per_particle": round(2 * (nx * nx * m + nx * m * m) / 1e6, 2)}
        if not args.no_torch:
            bt = max(1, min(n, TORCH_BYTES // (nx * max(nx, m) * 4 * 4)))
            fft_run = torch_fft_route(nx, m, dev)
            A = torch.from_numpy(resize.operator(nx, m)).float().to(dev)
            At = A.t().contiguous()
            mm_run = lambda xs: torch.matmul(torch.matmul(A, xs), At)      # noqa: E731
            for key, fn in (("torch_fft", fft_run), ("torch_matmul", mm_run)):
                total = 0.0
                for lo in range(0, n, bt):
                    xs = x[lo:min(n, lo + bt)]
                    total += time_ms(lambda: fn(xs), max(1, args.reps // 2), 1)
                    if lo == 0:
                        ref = y[:xs.shape[0]]
                        row["max_rel_diff_%s" % key] = float((fn(xs) - ref).abs().max() / ref.abs().max())
                row["%s_ms" % key] = round(total, 3)
            del A, At
        res["rows"].append(row)
        del x, y
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
