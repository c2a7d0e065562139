"""Timing of HDBSCAN (ra_hdbscan_core / ra_hdbscan_round behind hdbscan.hdbscan) on one GPU; prints one JSON line and writes it to
profiles/hdbscan_bench.json (--out).

Rows (n x d; min_cluster_size = 25, min_samples = 5), bench_dbscan.py's generators:
  embed     50 000 x 2: three Gaussian islands of different sizes plus 10 % uniform scatter, the look of a t-SNE embedding (seeded)
  large     262 144 x 2, the same generator
  factors   50 000 x 50: Gaussian clusters, the look of 2SDR factors (seeded)
Figures of every row, each the median of --reps after a warm-up, the sides alternating in one run:
  call      the whole hdbscan.hdbscan by the wall clock around a synchronised device (it holds host work: the union-find of every
            round and the tree of clusters), with n_rounds;
  core      ra_hdbscan_core alone, by device events;
  round     one ra_hdbscan_round (the first round, all singletons), by device events;
  count     dbs_count_kernel through ra_dbscan_count in the same run, by device events: the same tiles and the same distance
            chain, so round / count prices the selection logic (reported without a bar);
  tree      the host time of rules 6 - 9 inside the call (HdbscanResult.tree_seconds), and its share of the call;
  sklearn   sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, n_jobs=16).fit on the host CPUs (rows named by --sklearn; "not
            available" when sklearn does not import), with the number of non-tie points whose partition differs.  When the
            50 000 x 2 row's time times (262144 / 50000)^2 passes ten minutes, the large row skips sklearn and says so.
call_vs_sklearn is "met" when the call is faster than sklearn (margin 1.0 x), "missed" otherwise.

    python scripts/bench_hdbscan.py [--rows embed,large,factors] [--reps 5] [--sklearn embed,large,factors] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cryo_ralib_amd import api, hdbscan  # noqa: E402
from bench_dbscan import ROWS, make_row, timed  # noqa: E402

MIN_CLUSTER_SIZE, MIN_SAMPLES = 25, 5
SKLEARN_LIMIT_S = 600.0


def entries(x, dev):
    lib = api.load_library()
    n, d = (int(s) for s in x.shape)
    core2 = torch.empty(n, dtype=torch.float64, device=dev)
    comp = torch.arange(n, dtype=torch.int32, device=dev)
    w2 = torch.empty(n, dtype=torch.float64, device=dev)
    lo = torch.empty(n, dtype=torch.int32, device=dev)
    hi = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def core():
        api._check(lib.ra_hdbscan_core(P(x), n, d, MIN_SAMPLES, P(core2), stream), "ra_hdbscan_core")
        return core2

    def round_():
        api._check(lib.ra_hdbscan_round(P(x), n, d, P(core2), P(comp), P(w2), P(lo), P(hi), stream), "ra_hdbscan_round")
        return w2

    def count():
        api._check(lib.ra_dbscan_count(P(x), n, d, 1.0, MIN_SAMPLES, P(cnt), P(lab), stream), "ra_dbscan_count")
        return cnt

    return core, round_, count


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3


def same_partition(a, b):
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def bench_row(name, dev, reps, with_sklearn, sk_embed_s):
    X = make_row(name)
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    core, round_, count = entries(x, dev)
    call = lambda: hdbscan.hdbscan(x, MIN_CLUSTER_SIZE, MIN_SAMPLES)
    res = call()                                                    # warm-up of every side
    core()
    round_()
    count()
    torch.cuda.synchronize(dev)
    tc, tk, tr, tn, tt = [], [], [], [], []
    for _ in range(reps):
        r, ms = wall(call, dev)
        tc.append(ms)
        tt.append(r.tree_seconds * 1e3)
        tk.append(timed(core, dev)[1])
        tn.append(timed(count, dev)[1])
        tr.append(timed(round_, dev)[1])
    med = lambda v: float(np.median(v))
    row = dict(row=name, n=n, d=d, min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES, n_clusters=res.n_clusters,
               n_noise=res.n_noise, n_tie=int(res.tie_mask.sum()), n_rounds=res.n_rounds, call_ms=med(tc), call_ms_all=tc,
               core_ms=med(tk), core_ms_all=tk, round_ms=med(tr), round_ms_all=tr, count_ms=med(tn), count_ms_all=tn,
               round_over_count=med(tr) / med(tn), tree_ms=med(tt), tree_ms_all=tt, tree_share_of_call=med(tt) / med(tc))
    if with_sklearn and name == "large" and sk_embed_s is not None and sk_embed_s * (n / 50000.0) ** 2 > SKLEARN_LIMIT_S:
        row["sklearn_s"] = "skipped: the 50 000-point row's %.1f s times (n / 50000)^2 passes ten minutes" % sk_embed_s
    elif with_sklearn:
        try:
            from sklearn.cluster import HDBSCAN
            t0 = time.perf_counter()
            fit = HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES, n_jobs=16, copy=True).fit(X.astype(np.float64))
            row["sklearn_s"] = time.perf_counter() - t0
            T = res.tie_mask
            row["partition_equals_sklearn_outside_T"] = bool(same_partition(res.labels[~T], fit.labels_[~T]))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_hdbscan.py needs a GPU")
    dev = torch.device("cuda", 0)
    sk = set(s for s in args.sklearn.split(",") if s)
    rows, sk_embed_s = [], None
    for r in args.rows.split(","):
        assert r in ROWS, r
        rows.append(bench_row(r, dev, args.reps, r in sk, sk_embed_s))
        if r == "embed" and isinstance(rows[-1].get("sklearn_s"), float):
            sk_embed_s = rows[-1]["sklearn_s"]
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = dict(bench="hdbscan", device=torch.cuda.get_device_name(dev), reps=args.reps, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
