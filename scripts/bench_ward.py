"""Timing of Ward clustering (ra_ward_nearest / ra_ward_merge behind ward.linkage) on one GPU; prints one JSON line and writes it to
profiles/ward_bench.json (--out).

Rows (n x d), bench_dbscan.py's generators:
  factors   50 000 x 50: Gaussian clusters, the look of 2SDR factors (seeded)
  embed     50 000 x 2: three Gaussian islands of different sizes plus 10 % uniform scatter, the look of a t-SNE embedding (seeded)
  large     262 144 x 2, the same generator
Figures of every row, by device events, after --warmup warm-ups of every side, the sides alternating in one run, the median of
--reps:
  linkage   the whole ward.linkage (it holds the host work of every round and its one synchronisation), with n_rounds and
            rows_evaluated / n;
  nearest   the round-0 ra_ward_nearest: every row listed, every size 1;
  round     one ra_hdbscan_round (the first round, all singletons) at the same (n, d): the same tile with half the staged bytes
            and without the size factor.  nearest_over_round <= 1.5 is the expectation, reported as "met" or "missed", not asserted;
  scipy     scipy.cluster.hierarchy.ward on the host CPU at 20 000 x 50 only (its n^2 / 2 doubles: 1.6 GB there, 10 GB at 50 000),
            against ward.linkage at that shape ("not available" when scipy does not import, "not measured" with --no-scipy).

    python scripts/bench_ward.py [--rows factors,embed,large] [--reps 5] [--warmup 2] [--no-scipy] [--out FILE]
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
from cryo_ralib_amd import api, ward  # noqa: E402
from bench_dbscan import ROWS, make_factors, make_row, timed  # noqa: E402

EXPECTED_RATIO = 1.5
SCIPY_SHAPE = (20000, 50)


def entries(x, dev):
    lib = api.load_library()
    n, d = (int(s) for s in x.shape)
    c = x.double().contiguous()
    size = torch.ones(n, dtype=torch.int32, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    nn = torch.empty(n, dtype=torch.int32, device=dev)
    w2 = torch.empty(n, dtype=torch.float64, device=dev)
    core2 = torch.zeros(n, dtype=torch.float64, device=dev)
    comp = torch.arange(n, dtype=torch.int32, device=dev)
    lo = torch.empty(n, dtype=torch.int32, device=dev)
    hi = torch.empty(n, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def nearest():
        api._check(lib.ra_ward_nearest(P(c), P(size), n, d, P(rows), n, P(nn), P(w2), stream), "ra_ward_nearest")
        return nn

    def round_():
        api._check(lib.ra_hdbscan_round(P(x), n, d, P(core2), P(comp), P(w2), P(lo), P(hi), stream), "ra_hdbscan_round")
        return w2

    return nearest, round_


def bench_row(name, dev, reps, warmup):
    X = make_row(name)
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    nearest, round_ = entries(x, dev)
    call = lambda: ward.linkage(x)
    for _ in range(warmup):
        tree = call()
        nearest()
        round_()
    torch.cuda.synchronize(dev)
    tl, tn, tr = [], [], []
    for _ in range(reps):
        tl.append(timed(call, dev)[1])
        tn.append(timed(nearest, dev)[1])
        tr.append(timed(round_, dev)[1])
    med = lambda v: float(np.median(v))
    ratio = med(tn) / med(tr)
    return dict(row=name, n=n, d=d, n_rounds=tree.n_rounds, rows_evaluated_over_n=tree.rows_evaluated / n, linkage_ms=med(tl),
                linkage_ms_all=tl, nearest_ms=med(tn), nearest_ms_all=tn, round_ms=med(tr), round_ms_all=tr, nearest_over_round=ratio,
                expectation="nearest <= %.1f x round: %s" % (EXPECTED_RATIO, "met" if ratio <= EXPECTED_RATIO else "missed"))


def bench_scipy(dev, reps, warmup, with_scipy):
    n, d = SCIPY_SHAPE
    X = make_factors(n, d)
    x = torch.from_numpy(X).to(dev)
    for _ in range(warmup):
        tree = ward.linkage(x)
    tl = [timed(lambda: ward.linkage(x), dev)[1] for _ in range(reps)]
    row = dict(row="scipy", n=n, d=d, n_rounds=tree.n_rounds, rows_evaluated_over_n=tree.rows_evaluated / n,
               linkage_ms=float(np.median(tl)), linkage_ms_all=tl)
    if not with_scipy:
        row["scipy_s"] = "not measured"
        return row
    try:
        from scipy.cluster.hierarchy import ward as scipy_ward
    except ImportError:
        row["scipy_s"] = "not available"
        return row
    t0 = time.perf_counter()
    Z = scipy_ward(X.astype(np.float64))
    row["scipy_s"] = time.perf_counter() - t0
    row["merges_equal_scipy"] = bool(np.array_equal(Z[:, :2], tree.Z[:, :2]))
    row["heights_vs_scipy_rel"] = float(np.max(np.abs(Z[:, 2] - tree.heights) / Z[:, 2]))
    row["scipy_over_linkage"] = row["scipy_s"] * 1e3 / row["linkage_ms"]
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="factors,embed,large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ward_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ward.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for r in [s for s in args.rows.split(",") if s]:
        assert r in ROWS, r
        rows.append(bench_row(r, dev, args.reps, args.warmup))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    rows.append(bench_scipy(dev, args.reps, args.warmup, not args.no_scipy))
    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = dict(bench="ward", device=torch.cuda.get_device_name(dev), reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
