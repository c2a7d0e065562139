"""Timing of k-means (kmeans.kmeans on the ra_kmeans_* kernels) on one GPU; prints one JSON line and writes it to
profiles/kmeans_bench.json (--out).

Rows:
  notebook  50 000 x 50 factors in 12 Gaussian clusters, k = 12, k-means++, n_init = 1: the whole fit end to end from a host clock
            (median of --fits runs after a warm-up), with its n_iter; the same fit restated in torch (float32 mm + argmin +
            index_add_, the same seeds and iteration count); and, where sklearn is installed, sklearn's KMeans(algorithm="lloyd")
            on the host CPUs (OMP_NUM_THREADS of the environment).
  large     n = 1 048 576, d = 256, k = 256: one Lloyd iteration (ra_kmeans_lloyd, mean of --steps after a warm-up, device
            events) and its E-step alone (ra_kmeans_labels), against the f32 MFMA floor 2 n k d / 155 TFLOP/s and the HBM floor
            n d 4 B / 6.3 TB/s; and one iteration restated in torch (float32 mm + argmin + index_add_).

    python scripts/bench_kmeans.py [--rows notebook,large] [--steps 20] [--fits 5] [--no_sklearn] [--out FILE]

A kernel trace of the same rows: rocprofv3 --kernel-trace --stats -- python scripts/bench_kmeans.py --out ''
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
from cryo_ralib_amd import kmeans  # noqa: E402


def make_factors(n, d, ncl, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 3.0, (ncl, d))
    return (c[rng.integers(0, ncl, n)] + rng.normal(size=(n, d))).astype(np.float32)


def timed(fn, dev, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return out, a.elapsed_time(b) / reps


def torch_lloyd(x, C):
    """one Lloyd iteration in float32 torch: |c|^2 - 2 x c^T by mm, argmin, member means by index_add_"""
    D = (C * C).sum(1)[None, :] - 2.0 * (x @ C.t())
    lab = D.argmin(1)
    k = C.shape[0]
    cnt = torch.bincount(lab, minlength=k).clamp_(min=1).to(x.dtype)
    return torch.zeros_like(C).index_add_(0, lab, x) / cnt[:, None], lab


def notebook_row(dev, fits, with_sklearn):
    n, d, k = 50000, 50, 12
    X = make_factors(n, d, k)
    x = torch.from_numpy(X).to(dev)
    row = {"row": "notebook", "n": n, "d": d, "k": k, "init": "k-means++", "n_init": 1}
    kmeans.kmeans(x, k, random_state=0)                                   # warm-up (code load)
    torch.cuda.synchronize(dev)
    ts = []
    for i in range(fits):
        t0 = time.perf_counter()
        r = kmeans.kmeans(x, k, random_state=i)
        ts.append(time.perf_counter() - t0)
    row["fit_ms_median"], row["fit_ms_min"] = float(np.median(ts) * 1e3), float(np.min(ts) * 1e3)
    r = kmeans.kmeans(x, k, random_state=0)
    row["n_iter"], row["inertia"] = r.n_iter, r.inertia
    t0 = time.perf_counter()
    kmeans.kmeans(x, k, init=r.centers, max_iter=1)
    row["one_iteration_fit_ms"] = (time.perf_counter() - t0) * 1e3
    # the torch restatement from the same seeds, the same number of iterations
    C = x[torch.as_tensor(r.init_indices, device=dev)].clone()
    torch_lloyd(x, C)                                                     # warm-up
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(r.n_iter):
        C, lab = torch_lloyd(x, C)
    torch.cuda.synchronize(dev)
    row["torch_lloyd_ms"] = (time.perf_counter() - t0) * 1e3
    if with_sklearn:
        try:
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            KMeans(k, algorithm="lloyd", n_init=1, random_state=0).fit(X.astype(np.float64))
            row["sklearn_ms"] = (time.perf_counter() - t0) * 1e3
            row["sklearn_threads"] = os.environ.get("OMP_NUM_THREADS", "unset")
        except ImportError:
            row["sklearn_ms"] = "sklearn not installed"
    return row


def large_row(dev, steps):
    n, d, k = 1048576, 256, 256
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, d, device=dev, generator=g)
    x += torch.randn(k, d, device=dev, generator=g)[torch.randint(0, k, (n,), device=dev, generator=g)] * 3.0
    C = x[:k].double().contiguous()
    row = {"row": "large", "n": n, "d": d, "k": k}
    with torch.cuda.device(dev):
        B = kmeans._Device(x)
        B.lloyd(C)                                                            # warm-up
        Cn, _, _ = B.lloyd(C)
        torch.cuda.synchronize(dev)
        lib, s = B.lib, B.stream
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        out = torch.empty_like(C)

        def lloyd():
            lib.ra_kmeans_lloyd(P(x), n, d, P(B.nrm), P(Cn), k, P(out), P(B.labels), P(B.stats), s)
        _, row["lloyd_ms"] = timed(lloyd, dev, steps)
        inert = torch.empty(1, dtype=torch.float64, device=dev)

        def estep():
            lib.ra_kmeans_labels(P(x), n, d, P(B.nrm), P(Cn), k, P(B.labels), 1, P(inert), s)
        _, row["estep_ms"] = timed(estep, dev, steps)
        xc = x.clone()
        Cf = Cn.float()
        torch_lloyd(xc, Cf)
        _, row["torch_lloyd_ms"] = timed(lambda: torch_lloyd(xc, Cf), dev, steps)
    row["mfma_floor_ms"] = 2.0 * n * k * d / 155e12 * 1e3
    row["hbm_floor_ms"] = n * d * 4 / 6.3e12 * 1e3
    row["fraction_of_mfma_floor"] = row["mfma_floor_ms"] / row["lloyd_ms"]
    row["estep_fraction_of_mfma_floor"] = row["mfma_floor_ms"] / row["estep_ms"]
    row["speedup_vs_torch"] = row["torch_lloyd_ms"] / row["lloyd_ms"]
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="notebook,large")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--fits", type=int, default=5)
    ap.add_argument("--no_sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "rows": []}
    for name in args.rows.split(","):
        row = notebook_row(dev, args.fits, not args.no_sklearn) if name == "notebook" else large_row(dev, args.steps)
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
