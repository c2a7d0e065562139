"""Timing of the 2SDR reconstruction (ra_sdr_reconstruct: x^ = mean + A reshape(G f) B^T, optionally with |x - x^|^2) on one
GPU; writes profiles/sdr_denoise_bench.json and prints the same JSON line.

Rows: 50 000 x 90^2 and 125 000 x 90^2 with (p0, q0, r) = (25, 25, 50), 8 192 x 256^2 with (40, 40, 50); each without and with
residuals.  The model is an orthonormal random one and the factors are the transform of a seeded noise stack: the kernel's time
does not depend on the values.  Per row and side, device events around one call, 2 warm-up calls of every side first, the sides
alternating within each of --reps rounds, the median over the rounds:
    kernel   one ra_sdr_reconstruct call on operands already on the device
    torch    (a) the same three products restated with torch float32 matmul on the same tensors (c = F G^T, T = C B^T,
             x^ = A T + mean; with residuals ((x - x^) in double)^2 summed per image)
    copy     (b) a device-to-device copy that moves the bytes the kernel must move (the stack written once, with residuals
             also read once: a copy of half that many bytes reads and writes the same total)
The expectation is kernel <= torch; "met" records it per row.

    python scripts/bench_sdr_denoise.py [--reps 5] [--rows 90,90x125k,256] [--no_torch] [--out profiles/sdr_denoise_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cryo_ralib_amd import sdr  # noqa: E402
from cryo_ralib_amd._common import Launcher, ptr  # noqa: E402

ROWS = {"90": (50000, 90, 25, 25, 50), "90x125k": (125000, 90, 25, 25, 50), "256": (8192, 256, 40, 40, 50)}


def orthonormal(rows, cols, dev, g):
    return torch.linalg.qr(torch.randn((rows, cols), device=dev, generator=g))[0].contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no_torch", action="store_true", help="skip the torch restatement (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdr_denoise_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdr_denoise needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "method": "device events, 2 warm-up calls, sides alternating, median of %d" % args.reps,
           "rows": []}
    for name in args.rows.split(","):
        n, nx, p0, q0, r = ROWS[name]
        g = torch.Generator(device=dev).manual_seed(1)
        A, B, G = orthonormal(nx, p0, dev, g), orthonormal(nx, q0, dev, g), orthonormal(p0 * q0, r, dev, g)
        mean = torch.randn((nx, nx), device=dev, generator=g)
        x = torch.randn((n, nx, nx), device=dev, generator=g)
        model = sdr.SdrModel(mean.cpu().numpy(), A.cpu().numpy(), B.cpu().numpy(), G.cpu().numpy())
        F = sdr.transform(x, model)
        out, resid = torch.empty_like(x), torch.empty(n, dtype=torch.float64, device=dev)
        L = Launcher(x)

        def kernel(with_resid):
            L.call("ra_sdr_reconstruct", ptr(F), n, r, ptr(G), p0, q0, ptr(A), nx, ptr(B), nx, ptr(mean),
                   ptr(x) if with_resid else None, ptr(out), ptr(resid) if with_resid else None)

        def restated(with_resid):
            xh = torch.matmul(A, torch.matmul((F @ G.T).view(n, p0, q0), B.T)) + mean
            return ((x - xh).double() ** 2).sum(dim=(1, 2)) if with_resid else xh

        for with_resid in (False, True):
            moved = x.numel() * 4 * (2 if with_resid else 1) + F.numel() * 4 + (n * 8 if with_resid else 0)
            half = moved // 8                                        # floats of a copy that reads and writes `moved` bytes in all
            src, dst = x.view(-1)[:half], out.view(-1)[:half]
            sides = {"kernel": lambda: kernel(with_resid), "copy": lambda: dst.copy_(src)}
            if not args.no_torch:
                sides["torch"] = lambda: restated(with_resid)
            for _ in range(2):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in sides}
            for _ in range(args.reps):
                for k, fn in sides.items():
                    ms[k].append(timed(fn))
            row = {"row": name, "n": n, "p": nx, "q": nx, "p0": p0, "q0": q0, "r": r, "residuals": with_resid, "bytes_moved": moved}
            row.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
            row.update({k + "_ms_all": [round(t, 3) for t in v] for k, v in ms.items()})
            row["kernel_tb_per_s"] = round(moved / (row["kernel_ms"] * 1e-3) / 1e12, 3)
            if "torch_ms" in row:
                row["kernel_over_torch"] = round(row["kernel_ms"] / row["torch_ms"], 3)
                row["met"] = row["kernel_ms"] <= row["torch_ms"]
            row["kernel_over_copy"] = round(row["kernel_ms"] / row["copy_ms"], 3)
            if with_resid and not args.no_torch:
                kernel(True)
                want = restated(True)
                row["resid_max_rel_diff_vs_torch"] = float(((resid - want).abs() / want).max())
            res["rows"].append(row)
        del x, out, F, resid
        torch.cuda.empty_cache()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
