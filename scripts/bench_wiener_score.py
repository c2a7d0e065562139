"""Cost of the per-particle agreement scores (ra_wiener_score) on one GPU; prints one JSON line.

Rows (those of bench_wiener.py): 50 000 x 90^2 at 2x with k = 50 and k = 1, 32 768 x 100^2, 5 000 x 130^2, 8 192 x 256^2 (2x,
k = 50).  Per row, on the same stack and its own class sums, alternating in the same run: ms per score (leave-one-out, full band,
flipped weights, constant snr), per ra_wiener_accumulate alone (the yardstick: the same rot_shift2D and forward pass, a reduce in
place of the score) and per torch route (ra_rot_shift2d, pad, rfft2, gathered class sums, the same arithmetic in float32 with
float64 sums; its CTF is computed outside the timing and it runs in batches that keep its arrays within a few GB), each the
median of --reps device-event timings after --warmup calls; the ratios against the 1.10x target; and the largest difference
between the torch route's cc and the device's.  Writes the result to --out as well.

    python scripts/bench_wiener_score.py [--reps 5] [--warmup 1] [--rows 90k50,90k1,100,130,256] [--out profiles/wiener_score_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import api, wiener  # noqa: E402

from bench_wiener import ROWS, table, torch_ctf  # noqa: E402
from bench_wiener_ssnr import event_ms  # noqa: E402

TARGET = 1.10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "wiener_score_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wiener_score needs a GPU")
    dev = torch.device("cuda", 0)
    snr = 2.0
    res = {"device": torch.cuda.get_device_name(0), "snr": snr, "flipped": True, "leave_one_out": True, "target_ratio": TARGET,
           "rows": []}
    for name in args.rows.split(","):
        n, nx, k = ROWS[name]
        P, o, H = 2 * nx, nx // 2, nx + 1
        rng = np.random.default_rng(1)
        tab = table(n, nx)
        prm = np.column_stack([rng.uniform(0, 360, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.integers(0, 2, n)])
        lab = rng.integers(0, k, n)
        x = torch.randn((n, nx, nx), device=dev)
        num, den, counts = wiener.new_sums(k, nx, True, dev)
        wiener.accumulate(x, prm, lab, k, tab, num, den, counts, True, True)
        num_a, den_a, counts_a = wiener.new_sums(k, nx, True, dev)
        out = {}

        def score():
            out["dev"] = wiener.score(x, prm, lab, k, tab, num, den, counts, snr, None, True, None, True, True)

        def accumulate():
            num_a.zero_(); den_a.zero_(); counts_a.zero_()
            wiener.accumulate(x, prm, lab, k, tab, num_a, den_a, counts_a, True, True)
        sides = [("score_ms", score), ("accumulate_ms", accumulate)]
        if not args.no_torch:
            bt = max(1, min(n, (1 << 30) // (P * H * 8 * 4)))
            tab_al = wiener.aligned_table(tab, prm).astype(np.float32)
            cs = [torch_ctf(tab_al[lo:lo + bt], nx, P, dev) for lo in range(0, n, bt)]
            lab_t = torch.from_numpy(lab).to(dev)
            s_np, g_np = wiener.shells(P)
            gsel = torch.from_numpy(np.where((s_np >= 1) & (s_np <= P // 2), g_np, 0.0)).to(dev)
            numc = torch.view_as_complex(num)

            def tf():
                al = api.rot_shift2d(x, prm)
                parts = []
                for b, lo in enumerate(range(0, n, bt)):
                    hi = min(n, lo + bt)
                    big = torch.zeros((hi - lo, P, P), device=dev)
                    big[:, o:o + nx, o:o + nx] = al[lo:hi]
                    Y, c = torch.fft.rfft2(big), cs[b]
                    w = c.abs()
                    M = w * (numc[lab_t[lo:hi]] - w * Y) / ((den[lab_t[lo:hi]] - c * c).clamp_min(0) + 1.0 / snr)
                    parts.append(torch.stack([(gsel * (Y * M.conj()).real.double()).sum((1, 2)), (gsel * Y.abs().double() ** 2).sum((1, 2)),
                                              (gsel * M.abs().double() ** 2).sum((1, 2))], 1))
                out["torch"] = torch.cat(parts)
            sides.append(("torch_ms", tf))
        for _ in range(args.warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        times = {key: [] for key, _ in sides}
        for _ in range(args.reps):
            for key, fn in sides:
                times[key].append(event_ms(fn))
        med = {key: float(np.median(v)) for key, v in times.items()}
        row = {"row": name, "n": n, "nx": nx, "pad": 2, "k": k}
        row.update({key: round(v, 3) for key, v in med.items()})
        row["ratio_to_accumulate"] = round(med["score_ms"] / med["accumulate_ms"], 4)
        row["within_target"] = med["score_ms"] / med["accumulate_ms"] <= TARGET
        row["sums_read_mb"] = round(k * P * H * 12 / 1e6, 1)
        row.update({key + "_all": [round(t, 3) for t in v] for key, v in times.items()})
        if not args.no_torch:
            row["torch_over_score"] = round(med["torch_ms"] / med["score_ms"], 2)
            cc_t, _ = wiener.scores_from_sums(out["torch"].cpu().numpy(), lab, counts.cpu().numpy())
            row["max_cc_diff_vs_torch"] = float(np.nanmax(np.abs(cc_t - out["dev"]["cc"])))
            del cs
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        out.clear()
        del x, num, den, num_a, den_a
        torch.cuda.empty_cache()
    res["command"] = "python scripts/bench_wiener_score.py (reps %d, warmup %d)" % (args.reps, args.warmup)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
