"""Timing of UMAP (ra_umap_smooth_knn, ra_umap_epochs and ra_umap_place behind cryo_ralib_amd.umap) on one GPU; prints one JSON line
and writes it to profiles/umap_bench.json (--out).

Rows (n x d), bench_dbscan.py's generators, n_neighbors = 15:
  factors   50 000 x 50: Gaussian clusters, the look of 2SDR factors (seeded)
  embed     50 000 x 2: three Gaussian islands of different sizes plus 10 % uniform scatter (seeded)
Figures of every row, by device events, after --warmup warm-ups of every side, the sides alternating in one run, the median of
--reps:
  epoch     (a) one epoch (ra_umap_epochs, count = 1, at the middle of a schedule of 200, from the positions the start gives) against
            the same epoch restated in torch on the same device: the firing entries (their list is made outside the timed part),
            gathers of the positions, the moves in float64, torch.randint for the negatives, index_add_ into float64 sums and one
            rounding.  The expectation epoch <= torch (margin 1.0 x) is reported as "met" or "missed", not asserted.
  call      (b) the whole umap.umap call (kNN, calibration, union, start, 200 epochs) next to tsne.tsne (its defaults, 1000
            iterations) on the same row in the same run.  The expectation call <= t-SNE's is reported, not asserted.
  place     (c) factors only: umap.transform's parts for --place-rows new rows (default 1 048 576 x 50) into the 50 000 fitted ones,
            in batches of 65536 after one warm-up batch, run once: the kNN query, the calibration, the start and ra_umap_place
            (100 epochs) timed separately and summed over the batches.

    python scripts/bench_umap.py [--rows factors,embed] [--reps 5] [--warmup 2] [--no-tsne] [--place-rows N] [--out FILE]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cryo_ralib_amd import _graph, tsne, umap  # noqa: E402
from bench_dbscan import ROWS, make_factors, make_row, timed  # noqa: E402

N_NEIGHBORS, N_EPOCHS, NEG, SEED, BATCH = 15, 200, 5, 42, 65536


def torch_epoch(y, rows, cols, alpha, a, b, n):
    """rule 6 on the firing entries (rows, cols) restated in torch: returns the new float32 positions"""
    def clip(v):
        return torch.clamp(v, -4.0, 4.0)

    def epoch():
        Y = y.to(torch.float64)
        yi = Y[rows]
        d = yi - Y[cols]
        q = (d * d).sum(dim=1)
        qb = torch.pow(q, b)
        c = torch.where(q > 0, (-2.0 * a * b) * qb / q / (1.0 + a * qb), torch.zeros_like(q))
        move = 2.0 * clip(c[:, None] * d)
        for _ in range(NEG):
            k = torch.randint(0, n, (rows.numel(),), device=y.device)
            d = yi - Y[k]
            q = (d * d).sum(dim=1)
            g = (2.0 * b) / ((0.001 + q) * (1.0 + a * torch.pow(q, b)))
            move = move + torch.where((k != rows)[:, None], clip(g[:, None] * d), torch.zeros_like(d))
        S = torch.zeros_like(Y).index_add_(0, rows, move)
        return (Y + alpha * S).to(torch.float32)
    return epoch


def bench_epoch(D, ip, ix, s, y0, a, b, dev, reps, warmup):
    n, t = int(y0.shape[0]), N_EPOCHS // 2
    rate = (s / s.max()).contiguous()
    fire = torch.floor(t * rate) > torch.floor((t - 1) * rate)
    p = torch.nonzero(fire)[:, 0]
    rows = torch.arange(n, device=dev).repeat_interleave((ip[1:] - ip[:-1]).long())[p]
    cols = ix.long()[p]
    y = y0.clone()
    ours = lambda: D.epochs(y, ip, ix, rate, a, b, 1.0, NEG, 1.0, N_EPOCHS, t, 1, SEED)
    theirs = torch_epoch(y0, rows, cols, umap.alpha_at(1.0, t, N_EPOCHS), a, b, n)
    for _ in range(warmup):
        ours()
        theirs()
    torch.cuda.synchronize(dev)
    to, tt = [], []
    for _ in range(reps):
        to.append(timed(ours, dev)[1])
        tt.append(timed(theirs, dev)[1])
    mo, mt = float(np.median(to)), float(np.median(tt))
    return dict(nnz=int(ix.numel()), firing=int(p.numel()), epoch_ms=mo, epoch_ms_all=to, torch_epoch_ms=mt, torch_epoch_ms_all=tt,
                epoch_over_torch=mo / mt, expectation_epoch="epoch <= torch: %s" % ("met" if mo <= mt else "missed"))


def bench_place(Xf, Yf, a, b, dev, n_new):
    X_new = make_factors(n_new, Xf.shape[1], seed=1)
    D = umap._Device(dev)
    xf, yf = torch.from_numpy(Xf).to(dev), torch.from_numpy(Yf).to(dev)
    parts = dict(knn_query_ms=0.0, calibration_ms=0.0, start_ms=0.0, place_ms=0.0)

    def batch(s, keep):
        xb = torch.from_numpy(X_new[s:s + BATCH]).to(dev)
        (idx, d2), t1 = timed(lambda: _graph.knn_query(D, xb, xf, N_NEIGHBORS), dev)
        w, t2 = timed(lambda: D.smooth_knn(d2, N_NEIGHBORS)[2], dev)
        y, t3 = timed(lambda: D.start(yf, idx, w), dev)
        rate = (w / w.max(dim=1).values[:, None]).contiguous()
        _, t4 = timed(lambda: D.place(y, s, yf, idx, rate, a, b, 1.0, NEG, 1.0, 100, SEED), dev)
        if keep:
            for k, v in zip(parts, (t1, t2, t3, t4)):
                parts[k] += v
    batch(0, False)
    for s in range(0, n_new, BATCH):
        batch(s, True)
    parts.update(place_rows=n_new, place_total_ms=sum(parts.values()), place_batch=BATCH)
    return parts


def bench_row(name, dev, reps, warmup, with_tsne, place_rows):
    X = make_row(name)
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    row = dict(row=name, n=n, d=d, n_neighbors=N_NEIGHBORS, n_epochs=N_EPOCHS)
    a, b = umap.find_ab()
    D, ip, ix, s, _, _ = umap._graph_device(x, N_NEIGHBORS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", umap.UmapWarning)
        graph = (ip.cpu().numpy(), ix.cpu().numpy(), s.cpu().numpy())
        Y0, used = umap.initial_embedding(x, graph, "spectral", SEED, "device")
        row.update(bench_epoch(D, ip, ix, s, torch.from_numpy(Y0).to(dev), a, b, dev, reps, warmup))
        ours = lambda: umap.umap(x, n_neighbors=N_NEIGHBORS, n_epochs=N_EPOCHS)
        theirs = (lambda: tsne.tsne(x)) if with_tsne else None
        for _ in range(warmup):
            res = ours()
            if theirs:
                theirs()
        to, tt = [], []
        for _ in range(reps):
            to.append(timed(ours, dev)[1])
            if theirs:
                tt.append(timed(theirs, dev)[1])
    row.update(call_ms=float(np.median(to)), call_ms_all=to, init=res.init)
    if theirs:
        row.update(tsne_ms=float(np.median(tt)), tsne_ms_all=tt, call_over_tsne=row["call_ms"] / float(np.median(tt)),
                   expectation_call="call <= t-SNE: %s" % ("met" if row["call_ms"] <= float(np.median(tt)) else "missed"))
    else:
        row["tsne_ms"] = "not measured"
    if name == "factors" and place_rows > 0:
        row.update(bench_place(X, res.embedding, a, b, dev, place_rows))
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="factors,embed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-tsne", action="store_true")
    ap.add_argument("--place-rows", type=int, default=1048576)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umap_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_umap.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for r in [s for s in args.rows.split(",") if s]:
        assert r in ROWS, r
        rows.append(bench_row(r, dev, args.reps, args.warmup, not args.no_tsne, args.place_rows))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = dict(bench="umap", device=torch.cuda.get_device_name(dev), reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
