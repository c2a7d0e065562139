"""Timing of the t-SNE (tsne.tsne on the ra_tsne_* kernels) on one GPU; prints one JSON line and writes it to
profiles/tsne_bench.json (--out).

Rows: 50 000 x 50 (notebook 03's r = 50), 125 000 x 50 and 8 192 x 625.  The factors are Gaussian clusters made from a seed.
Per row: ms of the kNN (ra_tsne_knn), of the perplexity search (ra_tsne_affinity) and of symmetrising P; ms per iteration of
ra_tsne_step (mean of --steps launches after a warm-up, device events), and of its repulsion part's floor at 10 VALU slots per
64 pairs on 1024 SIMDs at 2.4 GHz; end to end for tsne.tsne(max_iter=1000) from a host clock (kNN, init and the
host checks included), with its n_iter; and, as a comparison only, the same iteration restated in torch on the same GPU (exact,
chunked all-pairs repulsion, sparse attraction, the same update), per iteration and extrapolated to 1000.  With --sklearn,
sklearn's default TSNE (Barnes-Hut, angle 0.5) on the host CPUs for the 50 000 row, if sklearn is installed.

    python scripts/bench_tsne.py [--rows 50k,125k,625] [--steps 50] [--torch_steps 5] [--sklearn] [--no_e2e] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cryo_ralib_amd import _graph, tsne  # noqa: E402

ROWS = {"50k": (50000, 50), "125k": (125000, 50), "625": (8192, 625), "4k": (4096, 50)}


def make_factors(n, d, seed=0, ncl=10):
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


def torch_iteration(y, rows, cols, p, update, gains, exag, mom, lr, chunk=2048):
    """one iteration of the same loop restated in torch: exact repulsion in row chunks, attraction by index_add"""
    n = y.shape[0]
    rep = torch.empty_like(y)
    Z = torch.zeros((), dtype=torch.float64, device=y.device)
    for s in range(0, n, chunk):
        D = y[s:s + chunk, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (D * D).sum(-1))
        Z += w.sum(dtype=torch.float64) - min(chunk, n - s)
        rep[s:s + chunk] = ((w * w)[..., None] * D).sum(1)
    D = y[rows] - y[cols]
    w = 1.0 / (1.0 + (D * D).sum(-1))
    attr = torch.zeros_like(y).index_add_(0, rows, (exag * p * w)[:, None] * D)
    g = 4.0 * (attr - rep / Z.float())
    inc = update * g < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    g = g * gains
    update.mul_(mom).sub_(lr * g)
    return y + update


def run_row(name, n, d, dev, steps, torch_steps, with_sklearn, e2e=True):
    X = make_factors(n, d)
    x = torch.from_numpy(X).to(dev)
    k = tsne.n_neighbors(n, 30.0)
    row = {"row": name, "n": n, "d": d, "k": k}
    with torch.cuda.device(dev):
        D = tsne._Device(dev)
        _graph.knn(D, x, k)                                                   # warm-up (code load)
        torch.cuda.synchronize(dev)
        (idx, d2), row["knn_ms"] = timed(lambda: _graph.knn(D, x, k), dev)
        pc, row["affinity_ms"] = timed(lambda: D.affinity(d2, 30.0), dev)
        (indptr, indices, P), row["symmetrize_ms"] = timed(lambda: D.symmetrize(idx, pc), dev)
        p32 = P.to(torch.float32)
        y0 = torch.from_numpy(tsne.random_init(n, 0)).to(dev)
        st = tsne._DeviceState(D, y0, indptr, indices, p32)
        st.reset()
        lr = tsne.resolve_learning_rate("auto", n, 12.0)
        for _ in range(5):
            st.step(12.0, 0.5, lr, False)
        torch.cuda.synchronize(dev)

        def steps_fn():
            for _ in range(steps):
                st.step(12.0, 0.5, lr, False)
        _, t = timed(steps_fn, dev)
        row["step_ms"] = t / steps
        row["step_floor_ms"] = n * n * 10 * 4 / 64 / 1024 / 2.4e9 * 1e3
        row["pairs_per_s"] = n * n / (row["step_ms"] * 1e-3)
        torch.cuda.synchronize(dev)
        if e2e:
            t0 = time.perf_counter()
            r = tsne.tsne(x, max_iter=1000)
            torch.cuda.synchronize(dev)
            row["end_to_end_s"] = time.perf_counter() - t0
            row["n_iter"], row["kl"] = r.n_iter, r.kl_divergence
        if torch_steps > 0:
            rows_ = torch.repeat_interleave(torch.arange(n, device=dev), indptr[1:].long() - indptr[:-1].long())
            cols = indices.long()
            y, upd, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
            y = torch_iteration(y, rows_, cols, p32, upd, gains, 12.0, 0.5, lr)
            torch.cuda.synchronize(dev)

            def torch_fn():
                yy = y
                for _ in range(torch_steps):
                    yy = torch_iteration(yy, rows_, cols, p32, upd, gains, 12.0, 0.5, lr)
                return yy
            _, t = timed(torch_fn, dev)
            row["torch_step_ms"] = t / torch_steps
            row["torch_1000_s"] = row["torch_step_ms"] * 1000 / 1e3 + (row["knn_ms"] + row["affinity_ms"]) / 1e3
            row["speedup_vs_torch"] = row["torch_step_ms"] / row["step_ms"]
    if with_sklearn and name == "50k":
        try:
            from sklearn.manifold import TSNE
            t0 = time.perf_counter()
            TSNE().fit_transform(X)
            row["sklearn_default_s"] = time.perf_counter() - t0
            row["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
        except ImportError:
            row["sklearn_default_s"] = "sklearn not installed"
    elif name == "50k":
        row["sklearn_default_s"] = "not run (pass --sklearn)"
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="50k,125k,625")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--torch_steps", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--no_e2e", action="store_true", help="skip the end-to-end run (profiling)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.json"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "rows": []}
    for name in args.rows.split(","):
        n, d = ROWS[name]
        res["rows"].append(run_row(name, n, d, dev, args.steps, args.torch_steps, args.sklearn, not args.no_e2e))
        print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
