"""Cost of the SSNR-weighted Wiener class averages against the constant-snr ones on one GPU; prints one JSON line.

Rows (those of bench_wiener.py): 50 000 x 90^2 at 2x with k = 50 and k = 1, 32 768 x 100^2, 5 000 x 130^2, 8 192 x 256^2 (2x,
k = 50).  Per row, on the same stack, alternating in the same run: ms per accumulate_halves + frc + finalize_ssnr (the SSNR path)
and per accumulate + finalize (the constant path), each the median of --reps device-event timings after --warmup calls, their
ratio against the 1.10x target, and the bytes the FRC pass reads (2k P (P/2 + 1) 12).  Writes the result to --out as well.

    python scripts/bench_wiener_ssnr.py [--reps 5] [--warmup 1] [--rows 90k50,90k1,100,130,256] [--out profiles/wiener_ssnr_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import wiener  # noqa: E402

from bench_wiener import ROWS, table  # noqa: E402

TARGET = 1.10


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "wiener_ssnr_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wiener_ssnr needs a GPU")
    dev = torch.device("cuda", 0)
    snr, floor = 2.0, wiener.SSNR_FLOOR
    res = {"device": torch.cuda.get_device_name(0), "snr": snr, "ssnr_floor": floor, "flipped": True, "target_ratio": TARGET,
           "rows": []}
    for name in args.rows.split(","):
        n, nx, k = ROWS[name]
        P, H = 2 * nx, nx + 1
        rng = np.random.default_rng(1)
        tab = table(n, nx)
        prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.integers(0, 2, n)])
        lab = rng.integers(0, k, n)
        x = torch.randn((n, nx, nx), device=dev)
        num, den, counts = wiener.new_sums(k, nx, True, dev)
        num2, den2, counts2 = wiener.new_half_sums(k, nx, True, dev)
        out_c = torch.empty((k, nx, nx), device=dev)
        out_s = torch.empty((k, nx, nx), device=dev)

        def const():
            num.zero_(); den.zero_(); counts.zero_()
            wiener.accumulate(x, prm, lab, k, tab, num, den, counts, True, True)
            wiener.finalize(num, den, counts, nx, True, snr, 1, out_c)

        def ssnr():
            num2.zero_(); den2.zero_(); counts2.zero_()
            wiener.accumulate_halves(x, prm, lab, k, tab, num2, den2, counts2, 0, True, True)
            _, reg = wiener.frc(num2, den2, counts2, nx, True, snr, 1, floor)
            wiener.finalize_ssnr(num2, den2, counts2, reg, nx, True, 1, out_s)
        for _ in range(args.warmup):
            const()
            ssnr()
        torch.cuda.synchronize()
        tc, ts = [], []
        for _ in range(args.reps):
            tc.append(event_ms(const))
            ts.append(event_ms(ssnr))
        mc, ms = float(np.median(tc)), float(np.median(ts))
        row = {"row": name, "n": n, "nx": nx, "pad": 2, "k": k, "ssnr_ms": round(ms, 3), "const_ms": round(mc, 3),
               "ratio": round(ms / mc, 4), "within_target": ms / mc <= TARGET, "frc_read_mb": round(2 * k * P * H * 12 / 1e6, 1),
               "ssnr_ms_all": [round(t, 3) for t in ts], "const_ms_all": [round(t, 3) for t in tc],
               "counts_agree": bool(torch.equal(counts2.sum(1), counts))}
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del x, num, den, num2, den2, out_c, out_s
        torch.cuda.empty_cache()
    res["command"] = "python scripts/bench_wiener_ssnr.py (reps %d, warmup %d)" % (args.reps, args.warmup)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
