"""Timing of the particle preprocessing (prep.normalize / prep.fourier_filter) on one GPU; writes profiles/prep_bench.json.

Rows: 50 000 x 90^2, 32 768 x 100^2, 5 000 x 130^2, 8 192 x 256^2.  Every figure is the median of --reps device-event timings
after --warmup calls, the two sides of a comparison alternating call by call in one run.

  normalise (ramp, in place)  against a device copy of the same bytes (a ratio, no bar), and against the same contract restated
                              in torch ops on the same tensor (double sums over the masked background, theta = m G^-1, one
                              rounding to float32): expectation kernel <= torch x 1.0.
  filter at pad=True          against ra_phase_flip on the same inputs (the same passes, a table read instead of the CTF
                              arithmetic): expectation filter <= flip x (1 + r), r = (max - min) / median of the flip's own timings.

    python scripts/bench_prep.py [--reps 5] [--warmup 2] [--rows 90,100,130,256] [--out profiles/prep_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cryo_ralib_amd import api, prep  # noqa: E402

ROWS = {"90": (50000, 90), "100": (32768, 100), "130": (5000, 130), "256": (8192, 256)}


def table(n, nx, seed=0):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 9), np.float32)
    t[:] = [nx, 1.5, 0, 0, 0, 300.0, 2.7, 0.1, 0.0]
    t[:, 2] = rng.uniform(10000, 30000, n)
    t[:, 3] = t[:, 2] - rng.uniform(0, 2000, n)
    t[:, 4] = rng.uniform(-90, 90, n)
    return t


def alternate(fns, reps, warmup):
    """[len(fns)][reps] ms: the functions called in turn, each call between two device events"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def torch_normalize(x, B, u, v, Ginv, nb):
    """N with ramp, restated in torch ops, in place on x"""
    xd = x.double()
    xb = xd * B
    m = torch.stack([xb.sum((1, 2)), (xb * u).sum((1, 2)), (xb * v).sum((1, 2))], 1)
    th = m @ Ginv
    e = xd - (th[:, 0, None, None] + th[:, 1, None, None] * u + th[:, 2, None, None] * v)
    mu = ((e * B).sum((1, 2)) / nb)[:, None, None]
    d = e - mu
    sigma = torch.sqrt((d * d * B).sum((1, 2)) / nb)[:, None, None]
    x.copy_(d / sigma)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prep needs a GPU")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "rows": []}
    for name in args.rows.split(","):
        n, nx = ROWS[name]
        R = nx / 2.0 - 5.0
        x = 100.0 + 7.0 * torch.randn((n, nx, nx), device=dev)
        # normalise against a copy and against torch
        Bn, un, vn = prep.background(nx, R)
        B, u, v = (torch.from_numpy(a.astype(np.float64)).to(dev) for a in (Bn, un, vn))
        A = np.stack([np.ones(int(Bn.sum())), un[Bn], vn[Bn]])
        Ginv = torch.from_numpy(np.linalg.inv(A @ A.T)).to(dev)
        w1, w2, dst = x.clone(), x.clone(), torch.empty_like(x)
        t_k, t_c, t_t = alternate([lambda: prep.normalize(w1, R, ramp=True), lambda: dst.copy_(x),
                                   lambda: torch_normalize(w2, B, u, v, Ginv, float(Bn.sum()))], args.reps, args.warmup)
        w1.copy_(x); w2.copy_(x)
        prep.normalize(w1, R, ramp=True)
        torch_normalize(w2, B, u, v, Ginv, float(Bn.sum()))
        diff = float((w1 - w2).abs().max())
        del w2, dst, B, u, v
        row = {"row": name, "n": n, "nx": nx, "bg_radius": R,
               "normalize_ms": round(med(t_k), 3), "copy_ms": round(med(t_c), 3), "normalize_over_copy": round(med(t_k) / med(t_c), 3),
               "torch_normalize_ms": round(med(t_t), 3), "max_abs_diff_vs_torch": diff,
               "normalize_le_torch": "met" if med(t_k) <= med(t_t) else "missed"}
        # filter at pad=True against the phase flip
        tab = table(n, nx)
        w2 = x.clone()
        t_f, t_p = alternate([lambda: prep.fourier_filter(w1, ("tanl", 0.2, 0.1), ("gauss", 0.01), pad=True),
                              lambda: api.phase_flip(w2, tab, True)], args.reps, args.warmup)
        r = (max(t_p) - min(t_p)) / med(t_p)
        row.update({"filter_ms": round(med(t_f), 3), "phase_flip_ms": round(med(t_p), 3), "phase_flip_spread": round(r, 4),
                    "filter_le_flip": "met" if med(t_f) <= med(t_p) * (1.0 + r) else "missed"})
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del x, w1, w2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
