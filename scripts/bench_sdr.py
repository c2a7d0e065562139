"""Timing of the two-stage dimension reduction (sdr.two_sdr on the ra_sdr_* kernels) on one GPU; prints one JSON line.

Rows: 50 000 x 90^2 and 125 000 x 90^2 with (p0, q0, r) = (25, 25, 50) (notebook 03's setting), 8 192 x 256^2 with (40, 40, 50).
The stack is a rank-8 x 8 signal under noise, made on the device from a seed.  Per row: ms of each stage -- mean, initial Gram,
one iteration (its two projected Grams and its eigen solves), projection, second-stage Gram, factors, and all host eigen
solves together -- from a host clock around work that ends in a device synchronise (one warm-up run first, then the median of
--reps runs with the iteration count of the warm-up run forced); the iteration count; the achieved FLOP/s and bytes/s of the
Gram passes and their floor max(FLOPs / 155 TF, bytes / 6.0 TB/s); and, as a comparison only, the same algorithm restated with
torch matmul / einsum in float32 on the same GPU (mean, centred copy, the same iteration count, projection, second stage),
end to end.

    python scripts/bench_sdr.py [--reps 3] [--rows 90,90x125k,256] [--no_torch]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import sdr  # noqa: E402

ROWS = {"90": (50000, 90, 25, 25, 50), "90x125k": (125000, 90, 25, 25, 50), "256": (8192, 256, 40, 40, 50)}
PEAK_FLOPS, PEAK_BYTES = 155e12, 6.0e12


def make_stack(n, nx, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    U0 = torch.linalg.qr(torch.randn((nx, 8), device=dev, generator=g))[0]
    C = torch.randn((n, 8, 8), device=dev, generator=g) * torch.logspace(1, -1, 8, device=dev)[:, None]
    x = torch.einsum("pa,iab,qb->ipq", U0, C, U0) + 0.5 * torch.randn((n, nx, nx), device=dev, generator=g)
    return x.contiguous()


class Clock:
    def __init__(self):
        self.t = {}

    def __call__(self, key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.t[key] = self.t.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
        return out


def staged_run(x, p0, q0, r, iters):
    """sdr._device_run with a clock around every stage and the iteration count forced"""
    D = sdr._Device(x)
    n, p, q, m = D.n, D.p, D.q, p0 * q0
    ck = Clock()
    mean = ck("mean", D.mean)
    SA = ck("gram_initial", lambda: D.gram(x, n, p, q, mean, 0))
    t_loop = time.perf_counter()
    for k in range(iters):
        _, B = ck("eig", lambda: sdr.top_eig(SA, q0))
        SB = ck("gram_b", lambda: D.gram(x, n, p, q, mean, 1, B))
        _, A = ck("eig", lambda: sdr.top_eig(SB, p0))
        if k + 1 < iters:
            SA = ck("gram_a", lambda: D.gram(x, n, p, q, mean, 2, A))
    loop_ms = (time.perf_counter() - t_loop) * 1e3
    U = ck("project", lambda: D.project(mean, A, B))
    C = ck("gram_second", lambda: D.gram(U, n, 1, m, None, 0))
    _, G = ck("eig", lambda: sdr.top_eig(C, r))
    F = ck("factors", lambda: D.factors(U, G))
    ck.t["iteration"] = loop_ms / iters
    return ck.t, F


def torch_restatement(x, p0, q0, r, iters):
    """the same algorithm with torch float32 matmul / einsum (host eigh as in sdr); returns F"""
    n, p, q = x.shape
    Xc = x - x.mean(0)
    Z = Xc.reshape(n * p, q)
    SA = (Z.T @ Z).double().cpu().numpy()
    for k in range(iters):
        B = torch.from_numpy(sdr.top_eig(SA, q0)[1]).float().to(x.device)
        T = torch.matmul(Xc, B).permute(1, 0, 2).reshape(p, -1)
        A = torch.from_numpy(sdr.top_eig((T @ T.T).double().cpu().numpy(), p0)[1]).float().to(x.device)
        if k + 1 < iters:
            S = torch.matmul(A.T, Xc).reshape(-1, q)
            SA = (S.T @ S).double().cpu().numpy()
    U = torch.matmul(torch.matmul(A.T, Xc), B).reshape(n, -1)
    G = torch.from_numpy(sdr.top_eig((U.T @ U).double().cpu().numpy(), r)[1]).float().to(x.device)
    return U @ G


def gram_cost(n, p, q, k, form):
    """(FLOPs, HBM bytes) one Gram pass needs: the products (2 per multiply-add) and one read of the stack"""
    if form == 0:
        return 2.0 * n * p * q * q, 4.0 * n * p * q
    d = p if form == 1 else q
    return 2.0 * n * (p * q * k + d * d * k), 4.0 * n * p * q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no_torch", action="store_true", help="skip the torch comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdr needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    for name in args.rows.split(","):
        n, nx, p0, q0, r = ROWS[name]
        m = p0 * q0
        x = make_stack(n, nx, dev)
        warm = sdr.two_sdr(x, p0, q0, r)                           # warm-up; sets the iteration count
        iters = warm.iterations
        runs = [staged_run(x, p0, q0, r, iters) for _ in range(args.reps)]
        ms = {k: float(np.median([t[k] for t, _ in runs])) for k in runs[0][0]}
        F = runs[-1][1]
        row = {"row": name, "n": n, "p": nx, "q": nx, "p0": p0, "q0": q0, "r": r, "iterations": iters,
               "stage_ms": {k: round(v, 3) for k, v in ms.items()}}
        row["end_to_end_ms"] = round(sum(v for k, v in ms.items() if k != "iteration"), 3)
        # the Gram passes: per-pass time of each form, achieved rates and floors
        passes = {}
        for key, form, k, cnt in (("gram_initial", 0, 0, 1), ("gram_b", 1, q0, iters), ("gram_a", 2, p0, iters - 1)):
            if cnt < 1:
                continue
            t = ms[key] / cnt / 1e3
            fl, by = gram_cost(n, nx, nx, k, form)
            passes[key] = {"ms_per_pass": round(t * 1e3, 3), "tflops": round(fl / t / 1e12, 2), "tb_per_s": round(by / t / 1e12, 2),
                           "floor_ms": round(max(fl / PEAK_FLOPS, by / PEAK_BYTES) * 1e3, 3),
                           "bound": "flops" if fl / PEAK_FLOPS > by / PEAK_BYTES else "bytes"}
        fl, by = gram_cost(n, 1, m, 0, 0)
        t = ms["gram_second"] / 1e3
        passes["gram_second"] = {"ms_per_pass": round(t * 1e3, 3), "tflops": round(fl / t / 1e12, 2), "tb_per_s": round(by / t / 1e12, 2),
                                 "floor_ms": round(max(fl / PEAK_FLOPS, by / PEAK_BYTES) * 1e3, 3)}
        row["gram_passes"] = passes
        fb, fa = gram_cost(n, nx, nx, q0, 1), gram_cost(n, nx, nx, p0, 2)
        row["iteration_floor_ms"] = round((max(fb[0] / PEAK_FLOPS, fb[1] / PEAK_BYTES) + max(fa[0] / PEAK_FLOPS, fa[1] / PEAK_BYTES)) * 1e3, 3)
        if not args.no_torch:
            Ft = torch_restatement(x, p0, q0, r, iters)            # warm-up
            tt = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                Ft = torch_restatement(x, p0, q0, r, iters)
                torch.cuda.synchronize()
                tt.append((time.perf_counter() - t0) * 1e3)
            row["torch_end_to_end_ms"] = round(float(np.median(tt)), 3)
            # the same subspace up to signs: compare |F^T F_t| column norms
            Fn, Ftn = F / F.norm(dim=0), Ft / Ft.norm(dim=0)
            row["min_abs_cos_vs_torch_first10"] = round(float((Fn[:, :10] * Ftn[:, :10]).sum(0).abs().min()), 6)
        res["rows"].append(row)
        del x, warm, runs, F
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
