"""Timing of the spectral embedding (ra_spectral_lanczos and its neighbours behind spectral.embedding) on one GPU; prints one JSON
line and writes it to profiles/spectral_bench.json (--out).

Rows (n x d), bench_dbscan.py's generators, n_neighbors = 15, 8 components:
  factors   50 000 x 50: Gaussian clusters, the look of 2SDR factors (seeded)
  embed     50 000 x 2: three Gaussian islands of different sizes plus 10 % uniform scatter (seeded)
Figures of every row, by device events, after --warmup warm-ups of every side, the sides alternating in one run, the median of
--reps:
  step      (a) one Lanczos step (ra_spectral_lanczos, steps = 1) at basis sizes 64 and 256 on the operator of the WHOLE graph (all
            n rows, whatever its components: a step's cost does not depend on them), against the same step restated in torch on the
            same device: a sparse CSR mv, then twice h = Q w, w -= Q^T h as float64 matmuls, the norm and the scale.  The
            expectation step <= torch (margin 1.0 x: the restatement moves the same bytes) is reported as "met" or "missed", not
            asserted.  "not available" when torch's sparse CSR product does not run on the device.
  call      (b) the whole spectral.embedding call (kNN, graph, components, solve, Ritz vectors, residuals), with n_steps, the rows
            embedded and left out, converged and the largest residual, against scikit-learn's SpectralEmbedding(
            affinity="nearest_neighbors") on the CPUs of the same machine, run once in a child process of its own with a time
            limit (--sklearn-limit seconds; "not finished" past it, "not available" when sklearn does not import, "not measured"
            with --no-sklearn).  The expectation call < sklearn is reported, not asserted.

    python scripts/bench_spectral.py [--rows factors,embed] [--reps 5] [--warmup 2] [--no-sklearn] [--sklearn-limit 240] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cryo_ralib_amd import spectral  # noqa: E402
from bench_dbscan import ROWS, make_row, timed  # noqa: E402

N_NEIGHBORS, N_COMPONENTS = 15, 8
BASIS = (64, 256)

SKLEARN_CHILD = """
import sys, time, json, warnings
import numpy as np
sys.path.insert(0, %r)
from bench_dbscan import make_row
from sklearn.manifold import SpectralEmbedding
X = make_row(%r).astype(np.float64)
warnings.simplefilter("ignore")
t0 = time.perf_counter()
SpectralEmbedding(%d, affinity="nearest_neighbors", n_neighbors=%d, random_state=0).fit(X)
print(json.dumps(dict(sklearn_s=time.perf_counter() - t0)))
"""


def torch_step(M, Q, j):
    """rule 6's step j on Q = [q0, v_0 .. v_j, ...] [m + 2][n]: writes v_{j+1}; nothing is read by the host"""
    def step():
        Qj = Q[:j + 2]
        w = torch.mv(M, Q[j + 1])
        alpha = Q[j + 1] @ w
        for _ in range(2):
            w = w - Qj.T @ (Qj @ w)
        beta = torch.linalg.vector_norm(w)
        Q[j + 2] = w / beta
        return alpha, beta
    return step


def bench_steps(x, dev, reps, warmup):
    D, indptr, indices, a, _ = spectral._graph_device(x, N_NEIGHBORS, "connectivity", 7, 0.0)
    op = spectral._DeviceOperator(D, indptr, indices, a)
    n, m = op.n, max(BASIS) + 1
    q0 = np.sqrt(op.deg) / np.sqrt(np.sum(op.deg))
    v0 = np.random.RandomState(0).uniform(-1.0, 1.0, n)
    v0 -= (q0 @ v0) * q0
    op.start(q0, v0 / np.linalg.norm(v0), m)
    op.run(0, m - 1)                                        # a real basis: v_0 .. v_256
    Q = torch.cat([op.q0[None], op.V])
    try:
        M = torch.sparse_csr_tensor(indptr.long(), indices.long(), op.val, size=(n, n))
        torch_step(M, Q.clone(), 1)()
        torch.cuda.synchronize(dev)
    except Exception as e:                                   # noqa: BLE001 -- whatever the sparse backend raises
        M, why = None, "%s: %s" % (type(e).__name__, e)
    out = dict(nnz=int(op.val.numel()))
    for b in BASIS:
        ours = lambda: op.run(b, 1)
        theirs = torch_step(M, Q, b) if M is not None else None
        for _ in range(warmup):
            ours()
            if theirs:
                theirs()
        torch.cuda.synchronize(dev)
        to, tt = [], []
        for _ in range(reps):
            to.append(timed(ours, dev)[1])
            if theirs:
                tt.append(timed(theirs, dev)[1])
        med = lambda v: float(np.median(v))
        out["step_ms_%d" % b], out["step_ms_%d_all" % b] = med(to), to
        if theirs:
            out["torch_step_ms_%d" % b], out["torch_step_ms_%d_all" % b] = med(tt), tt
            out["step_over_torch_%d" % b] = med(to) / med(tt)
            out["expectation_step_%d" % b] = "step <= torch: %s" % ("met" if med(to) <= med(tt) else "missed")
        else:
            out["torch_step_ms_%d" % b] = "not available (%s)" % why
    return out


def bench_row(name, dev, reps, warmup, with_sklearn, limit):
    X = make_row(name)
    n, d = X.shape
    x = torch.from_numpy(X).to(dev)
    row = dict(row=name, n=n, d=d, n_neighbors=N_NEIGHBORS, n_components=N_COMPONENTS)
    row.update(bench_steps(x, dev, reps, warmup))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", spectral.SpectralWarning)
        call = lambda: spectral.embedding(x, N_COMPONENTS, n_neighbors=N_NEIGHBORS)
        for _ in range(warmup):
            res = call()
        tc = [timed(call, dev)[1] for _ in range(reps)]
    row.update(call_ms=float(np.median(tc)), call_ms_all=tc, n_steps=res.n_steps, converged=res.converged, rows_embedded=len(res.rows),
               n_dropped=res.n_dropped, n_graph_components=int(res.component.max()) + 1, largest_residual=float(res.residuals.max()))
    if not with_sklearn:
        row["sklearn_s"] = "not measured"
        return row
    try:
        import sklearn  # noqa: F401
    except ImportError:
        row["sklearn_s"] = "not available"
        return row
    code = SKLEARN_CHILD % (os.path.dirname(os.path.abspath(__file__)), name, N_COMPONENTS, N_NEIGHBORS)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit)
        if p.returncode == 0:
            row["sklearn_s"] = json.loads(p.stdout.strip().splitlines()[-1])["sklearn_s"]
            row["sklearn_over_call"] = row["sklearn_s"] * 1e3 / row["call_ms"]
            row["expectation_call"] = "call < sklearn: %s" % ("met" if row["call_ms"] < row["sklearn_s"] * 1e3 else "missed")
        else:
            row["sklearn_s"] = "failed: %s" % p.stderr.strip().splitlines()[-1:]
    except subprocess.TimeoutExpired:
        row["sklearn_s"] = "not finished in %d s" % limit
        row["expectation_call"] = "call < sklearn: met (sklearn was stopped at its limit after %.0f s)" % (time.perf_counter() - t0)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="factors,embed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for r in [s for s in args.rows.split(",") if s]:
        assert r in ROWS, r
        rows.append(bench_row(r, dev, args.reps, args.warmup, not args.no_sklearn, args.sklearn_limit))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = dict(bench="spectral", device=torch.cuda.get_device_name(dev), reps=args.reps, warmup=args.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
