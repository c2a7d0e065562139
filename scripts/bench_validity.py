"""Timing of the silhouette (ra_kmeans_silhouette behind kmeans.silhouette_samples) on one GPU; prints one JSON line and writes it
to profiles/validity_bench.json (--out).

Rows (n x d, k; Gaussian clusters, labels from one kmeans.kmeans fit):
  notebook  50 000 x 50, k = 12
  embed     50 000 x 2, k = 12
  large     262 144 x 50, k = 50
Sides of every row, on the same device tensors:
  kernel    the whole entry point (member lists, padded columns, the pair kernel) by device events;
  torch     the same values restated in float32 torch: row chunks of torch.cdist, the sums per label by index_add_ along the
            columns, then a, b and s.  The two sides alternate in one run; each figure is the median of --reps after a warm-up;
  sklearn   sklearn.metrics.silhouette_samples on the host CPUs (OMP_NUM_THREADS of the environment), rows up to --sklearn_max_n;
  copy      a device copy of X, for scale.
flop_fraction is 3 n^2 d (a subtraction and a fused multiply-add per pair and feature) over the kernel time and the f32 vector
peak of 157.3 TFLOP/s: the entry point's share, list building included.

    python scripts/bench_validity.py [--rows notebook,embed,large] [--reps 5] [--sklearn_max_n 50000] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cryo_ralib_amd import api, kmeans  # noqa: E402

ROWS = {"notebook": (50000, 50, 12), "embed": (50000, 2, 12), "large": (262144, 50, 50)}
PEAK_F32 = 157.3e12


def make_factors(n, d, ncl, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 3.0, (ncl, d))
    return (c[rng.integers(0, ncl, n)] + rng.normal(size=(n, d))).astype(np.float32)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return out, a.elapsed_time(b)


def torch_silhouette(x, lab, k, chunk_bytes=1 << 30):
    """silhouette_samples in float32 torch: chunked cdist, per-label sums by index_add_"""
    n = x.shape[0]
    cnt = torch.bincount(lab, minlength=k).to(x.dtype)
    ch = max(1, chunk_bytes // (4 * n))
    out = torch.empty(n, dtype=x.dtype, device=x.device)
    rows = torch.arange(n, device=x.device)
    for s0 in range(0, n, ch):
        D = torch.cdist(x[s0:s0 + ch], x)
        S = torch.zeros((D.shape[0], k), dtype=x.dtype, device=x.device).index_add_(1, lab, D)
        own = lab[s0:s0 + ch]
        r = rows[:D.shape[0]]
        a = S[r, own] / (cnt[own] - 1).clamp_(min=1)
        M = S / cnt[None, :]
        M[:, cnt == 0] = float("inf")
        M[r, own] = float("inf")
        b = M.min(1).values
        out[s0:s0 + ch] = torch.nan_to_num((b - a) / torch.maximum(a, b)) * (cnt[own] > 1)
    return out


def bench_row(name, dev, reps, sklearn_max_n):
    n, d, k = ROWS[name]
    X = make_factors(n, d, k)
    x = torch.from_numpy(X).to(dev)
    fit = kmeans.kmeans(x, k, random_state=0)
    lab32 = torch.from_numpy(fit.labels.astype(np.int32)).to(dev)
    lab64 = lab32.to(torch.int64)
    lib = api.load_library()
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    near = torch.empty(n, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def kernel():
        api._check(lib.ra_kmeans_silhouette(P(x), n, d, P(lab32), k, P(out), P(near), stream), "ra_kmeans_silhouette")
        return out

    kernel()
    ref = torch_silhouette(x, lab64, k)
    torch.cuda.synchronize(dev)
    tk, tt, tc = [], [], []
    for _ in range(reps):
        tk.append(timed(kernel, dev)[1])
        tt.append(timed(lambda: torch_silhouette(x, lab64, k), dev)[1])
        tc.append(timed(x.clone, dev)[1])
    kernel_ms, torch_ms = float(np.median(tk)), float(np.median(tt))
    row = dict(row=name, n=n, d=d, k=k, kernel_ms=kernel_ms, kernel_ms_all=tk, torch_ms=torch_ms, torch_ms_all=tt,
               copy_ms=float(np.median(tc)), torch_over_kernel=torch_ms / kernel_ms,
               flop_fraction=3.0 * n * n * d / (kernel_ms * 1e-3) / PEAK_F32,
               silhouette=float(out[:, 0].mean().item()),
               max_abs_kernel_minus_torch=float((out[:, 0] - ref.to(torch.float64)).abs().max().item()))
    if n <= sklearn_max_n:
        try:
            from sklearn.metrics import silhouette_samples
            t0 = time.perf_counter()
            sv = silhouette_samples(X.astype(np.float64), fit.labels, metric="euclidean")
            row["sklearn_s"] = time.perf_counter() - t0
            row["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0"))
            row["max_abs_kernel_minus_sklearn"] = float(np.abs(out[:, 0].cpu().numpy() - sv).max())
        except ImportError:
            row["sklearn_s"] = None
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="notebook,embed,large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn_max_n", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validity_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_validity.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = dict(bench="validity", device=torch.cuda.get_device_name(dev), reps=args.reps,
               rows=[bench_row(r, dev, args.reps, args.sklearn_max_n) for r in args.rows.split(",")])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
