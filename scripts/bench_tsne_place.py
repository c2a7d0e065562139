"""Timing of the out-of-sample t-SNE placement (tsne.transform on ra_tsne_knn_query, ra_tsne_affinity_rows and ra_tsne_place) on
one GPU; prints one JSON line and writes it to profiles/tsne_place_bench.json (--out).

Rows (new points x features into fitted points): 50 000 x 50 into 50 000, 1 048 576 x 50 into 50 000, 1 000 x 50 into 50 000.  The
factors are bench_tsne.py's Gaussian clusters; the fitted embedding is a seeded normal cloud of span about 80 (a placement does not
depend on how the embedding was made).  Per row, each from device events as the median of --reps timings after --warmup warm-ups,
the two sides of a comparison alternating: ms of the kNN query, of the affinities, of one placement iteration (ra_tsne_place with
--steps iterations and no KL pass, divided by --steps), of the whole transform (250 iterations, host copies included) and of the
same placement iteration restated in float32 torch (chunked all-pairs).  On the first row also ms per iteration of ra_tsne_step
at n = 50 000 on the fit's own kernels, alternating with the placement.  Expectations, reported as met or missed with the ratio:
(a) placement per iteration at 50 000 into 50 000 <= 1.0 x ra_tsne_step per iteration; (b) placement <= torch on every row.

    python scripts/bench_tsne_place.py [--rows 50k,1m,1k] [--steps 20] [--reps 5] [--warmup 2] [--no_torch] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cryo_ralib_amd import _graph, tsne  # noqa: E402
from cryo_ralib_amd._common import ptr  # noqa: E402
from bench_tsne import make_factors  # noqa: E402

ROWS = {"50k": 50000, "1m": 1048576, "1k": 1000, "4k": 4096}
M_FIT, D_FEAT, PERPLEXITY = 50000, 50, 30.0


def event_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def alternate(sides, dev, reps, warmup):
    """median ms of each side, the sides taking turns: warmup rounds, then reps timed rounds"""
    times = [[] for _ in sides]
    for r in range(warmup + reps):
        for i, fn in enumerate(sides):
            t = event_ms(fn, dev)
            if r >= warmup:
                times[i].append(t)
    return [statistics.median(t) for t in times]


def torch_place_iteration(y, yfit, idx, p, update, gains, exag, mom, lr, chunk=2048):
    """one placement iteration restated in float32 torch: per-point Z and repulsion in row chunks, attraction by a gather"""
    rep = torch.empty_like(y)
    for s in range(0, y.shape[0], chunk):
        D = y[s:s + chunk, None, :] - yfit[None, :, :]
        w = 1.0 / (1.0 + (D * D).sum(-1))
        rep[s:s + chunk] = ((w * w)[..., None] * D).sum(1) / w.sum(1, keepdim=True)
    for s in range(0, y.shape[0], 65536):
        D = y[s:s + 65536, None, :] - yfit[idx[s:s + 65536]]
        w = 1.0 / (1.0 + (D * D).sum(-1))
        rep[s:s + 65536] = ((exag * p[s:s + 65536] * w)[..., None] * D).sum(1) - rep[s:s + 65536]
    g = 4.0 * rep
    gains.copy_(torch.where(update * g < 0, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    update.mul_(mom).sub_(lr * (g * gains))
    y.add_(update)


def new_points(n):
    """n held-out draws of the clusters make_factors(M_FIT, D_FEAT, seed=0) drew the fitted rows from"""
    c = np.random.default_rng(0).normal(0.0, 3.0, (10, D_FEAT))
    rng = np.random.default_rng(1)
    return (c[rng.integers(0, 10, n)] + rng.normal(size=(n, D_FEAT))).astype(np.float32)


def run_row(name, n, xf, yf, dev, args):
    X = new_points(n)
    m, k = int(xf.shape[0]), tsne.n_neighbors_query(int(xf.shape[0]), PERPLEXITY)
    row = {"row": name, "n_new": n, "m_fit": m, "d": D_FEAT, "k": k, "steps": args.steps}
    with torch.cuda.device(dev):
        D = tsne._Device(dev)
        x = torch.from_numpy(X).to(dev)
        (row["knn_query_ms"],) = alternate([lambda: _graph.knn_query(D, x, xf, k)], dev, args.reps, args.warmup)
        idx, d2 = _graph.knn_query(D, x, xf, k)
        (row["affinity_ms"],) = alternate([lambda: D.affinity_rows(d2, PERPLEXITY)], dev, args.reps, args.warmup)
        p = D.affinity_rows(d2, PERPLEXITY).to(torch.float32)
        y0 = tsne._initial_placement_device(torch, "weighted", yf, idx, p)
        y = y0.clone()

        def place():
            y.copy_(y0)
            D.call("ra_tsne_place", ptr(y), n, ptr(yf), m, ptr(idx), ptr(p), k, 1.0, 0.8, 0.1, args.steps, None)
        sides, names = [place], ["place_ms"]
        if not args.no_torch:
            yt, upd, gains, il = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0), idx.long()

            def torch_side():
                torch_place_iteration(yt, yf, il, p, upd, gains, 1.0, 0.8, 0.1)
            sides.append(torch_side)
            names.append("torch_ms")
        if name == "50k":
            # the fit's own step on the same fitted rows, from its own affinities
            fi, fd2 = _graph.knn(D, xf, tsne.n_neighbors(m, PERPLEXITY))
            indptr, indices, P = D.symmetrize(fi, D.affinity(fd2, PERPLEXITY))
            st = tsne._DeviceState(D, yf.clone(), indptr, indices, P.to(torch.float32))
            st.reset()

            def fit_steps():
                for _ in range(args.steps):
                    st.step(1.0, 0.8, 1.0, False)
            sides.append(fit_steps)
            names.append("fit_ms")
        got = dict(zip(names, alternate(sides, dev, args.reps, args.warmup)))
        row["place_iter_ms"] = got["place_ms"] / args.steps
        row["pairs_per_s"] = n * m / (row["place_iter_ms"] * 1e-3)
        if "torch_ms" in got:
            row["torch_iter_ms"] = got["torch_ms"]
            row["b_place_over_torch"] = row["place_iter_ms"] / row["torch_iter_ms"]
            row["b"] = "met" if row["b_place_over_torch"] <= 1.0 else "missed"
        if "fit_ms" in got:
            row["fit_step_ms"] = got["fit_ms"] / args.steps
            row["a_place_over_fit_step"] = row["place_iter_ms"] / row["fit_step_ms"]
            row["a"] = "met" if row["a_place_over_fit_step"] <= 1.0 else "missed"
        del x, idx, d2, p, y0, y
        (row["transform_ms"],) = alternate([lambda: tsne.transform(X, xf, yf)], dev, args.reps, args.warmup)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="50k,1m,1k")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_torch", action="store_true", help="skip the torch restatement (profiling)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_place_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne_place needs a GPU")
    dev = torch.device("cuda", 0)
    xf = torch.from_numpy(make_factors(M_FIT, D_FEAT, seed=0)).to(dev)
    yf = torch.from_numpy((np.random.default_rng(2).normal(size=(M_FIT, 2)) * 13.0).astype(np.float32)).to(dev)
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup, "rows": []}
    for name in args.rows.split(","):
        res["rows"].append(run_row(name, ROWS[name], xf, yf, dev, args))
        print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
