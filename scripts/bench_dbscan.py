"""Timing of DBSCAN (ra_dbscan_count / ra_dbscan_step behind dbscan.dbscan) on one GPU; prints one JSON line and writes it to
profiles/dbscan_bench.json (--out).

Rows (n x d; min_samples = 5, eps = the 90 % quantile of dbscan.kdistances(X, 5)):
  embed     50 000 x 2: three Gaussian islands of different sizes plus 10 % uniform scatter, the look of a t-SNE embedding (seeded)
  large     262 144 x 2, the same generator
  factors   50 000 x 50: Gaussian clusters, the look of 2SDR factors (seeded)
Figures of every row, by device events, each the median of --reps after a warm-up, the sides alternating in one run:
  call      the whole dbscan.dbscan (count pass, every merging round with its host read of one int, the map to 0 .. c - 1);
  count     ra_dbscan_count alone;
  step      one ra_dbscan_step (the first round, from the count pass's labels: core list, minimum, hook, compress);
  torch     the count pass restated in torch on the same tensor: row chunks of float64 torch.cdist(...) <= eps, summed;
  sklearn   sklearn.cluster.DBSCAN(n_jobs=16).fit on the host CPUs (rows named by --sklearn; "not available" when sklearn does
            not import), with the number of labels that differ from the device's.
flop_fraction_count is 3 n^2 d (a subtraction and a fused multiply-add per pair and feature) over the count time by events and
the f64 vector peak (--peak_f64, TFLOP/s; default 78.6, half the 157.3 TFLOP/s f32 vector rate).  --profile ROW runs only the
count pass of one row a few times, for a kernel trace taken in a run of its own.

    python scripts/bench_dbscan.py [--rows embed,large,factors] [--reps 5] [--sklearn embed,large,factors] [--out FILE]
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
from cryo_ralib_amd import api, dbscan  # noqa: E402

ROWS = {"embed": (50000, 2), "large": (262144, 2), "factors": (50000, 50)}
MIN_SAMPLES = 5


def make_embedding(n, seed=0):
    rng = np.random.default_rng(seed)
    ns = n // 10
    sizes = [(n - ns) // 2, (n - ns) // 3, 0]
    sizes[2] = n - ns - sizes[0] - sizes[1]
    centres, sig = np.array([[-30.0, -10.0], [25.0, 20.0], [10.0, -35.0]]), (9.0, 6.0, 3.0)
    parts = [centres[j] + sig[j] * rng.normal(size=(sizes[j], 2)) for j in range(3)]
    parts.append(rng.uniform(-70.0, 70.0, (ns, 2)))
    return np.concatenate(parts)[rng.permutation(n)].astype(np.float32)


def make_factors(n, d, ncl=12, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 3.0, (ncl, d))
    return (c[rng.integers(0, ncl, n)] + rng.normal(size=(n, d))).astype(np.float32)


def make_row(name):
    n, d = ROWS[name]
    return make_embedding(n) if d == 2 else make_factors(n, d)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return out, a.elapsed_time(b)


def torch_count(x, eps, chunk_bytes=1 << 30):
    n = x.shape[0]
    x64 = x.to(torch.float64)
    ch = max(1, chunk_bytes // (8 * n))
    out = torch.empty(n, dtype=torch.int64, device=x.device)
    for s0 in range(0, n, ch):
        out[s0:s0 + ch] = (torch.cdist(x64[s0:s0 + ch], x64) <= eps).sum(1)
    return out


def entries(x, eps, dev):
    lib = api.load_library()
    n, d = (int(s) for s in x.shape)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    ch = torch.empty(1, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def count():
        api._check(lib.ra_dbscan_count(P(x), n, d, eps, MIN_SAMPLES, P(cnt), P(lab), stream), "ra_dbscan_count")
        return cnt

    def step():
        api._check(lib.ra_dbscan_step(P(x), n, d, eps, P(cnt), MIN_SAMPLES, P(lab), P(out), P(ch), stream), "ra_dbscan_step")
        return out

    return count, step


def bench_row(name, dev, reps, with_sklearn, peak_f64):
    X = make_row(name)
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    eps = float(np.quantile(dbscan.kdistances(x, MIN_SAMPLES), 0.9))
    count, step = entries(x, eps, dev)
    res = dbscan.dbscan(x, eps, MIN_SAMPLES)               # warm-up of every side
    cnt = count().clone()
    step()
    ref = torch_count(x, eps)
    torch.cuda.synchronize(dev)
    tc, tk, ts, tt = [], [], [], []
    for _ in range(reps):
        tc.append(timed(lambda: dbscan.dbscan(x, eps, MIN_SAMPLES), dev)[1])
        tk.append(timed(count, dev)[1])
        tt.append(timed(lambda: torch_count(x, eps), dev)[1])
        ts.append(timed(step, dev)[1])
    med = lambda v: float(np.median(v))
    row = dict(row=name, n=n, d=d, eps=eps, min_samples=MIN_SAMPLES, n_clusters=res.n_clusters, n_noise=res.n_noise,
               n_core=int(res.core_mask.sum()), n_rounds=res.n_rounds, call_ms=med(tc), call_ms_all=tc, count_ms=med(tk),
               count_ms_all=tk, step_ms=med(ts), step_ms_all=ts, torch_count_ms=med(tt), torch_count_ms_all=tt,
               torch_over_count=med(tt) / med(tk), counts_differ_from_torch=int((cnt.to(torch.int64) != ref).sum().item()),
               flop_fraction_count=3.0 * n * n * d / (med(tk) * 1e-3) / (peak_f64 * 1e12))
    row["count_vs_torch"] = "met" if row["count_ms"] <= row["torch_count_ms"] else "missed"
    if with_sklearn:
        try:
            from sklearn.cluster import DBSCAN
            t0 = time.perf_counter()
            fit = DBSCAN(eps=eps, min_samples=MIN_SAMPLES, n_jobs=16).fit(X.astype(np.float64))
            row["sklearn_s"] = time.perf_counter() - t0
            row["labels_differ_from_sklearn"] = int(np.count_nonzero(fit.labels_ != res.labels))
            row["call_vs_sklearn"] = "met" if row["call_ms"] * 1e-3 < row["sklearn_s"] else "missed"
        except ImportError:
            row["sklearn_s"] = "not available"
    else:
        row["sklearn_s"] = "not measured"
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="embed,large,factors")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn", default="embed,large,factors", help="rows that also run sklearn on the CPU ('' for none)")
    ap.add_argument("--peak_f64", type=float, default=78.6, help="f64 vector peak in TFLOP/s")
    ap.add_argument("--profile", default=None, help="ROW: only its count pass, 3 times, for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_dbscan.py needs a GPU")
    dev = torch.device("cuda", 0)
    if args.profile:
        x = torch.from_numpy(make_row(args.profile)).to(dev)
        eps = float(np.quantile(dbscan.kdistances(x, MIN_SAMPLES), 0.9))
        count, _ = entries(x, eps, dev)
        for _ in range(3):
            count()
        torch.cuda.synchronize(dev)
        print(json.dumps(dict(profile=args.profile, n=int(x.shape[0]), d=int(x.shape[1]), eps=eps, flop=3.0 * x.shape[0] ** 2 * x.shape[1])))
        return
    sk = set(s for s in args.sklearn.split(",") if s)
    res = dict(bench="dbscan", device=torch.cuda.get_device_name(dev), reps=args.reps, peak_f64_tflops=args.peak_f64,
               rows=[bench_row(r, dev, args.reps, r in sk, args.peak_f64) for r in args.rows.split(",")])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
