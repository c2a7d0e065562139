"""Times the Gaussian mixture kernels against a torch float64 restatement on the same device, a device copy of the bytes moved and
(row 1) scikit-learn on the CPU, and writes profiles/gmm_bench.json.

    python scripts/bench_gmm.py [--rows 1,2,3,4] [--reps 5] [--out profiles/gmm_bench.json] [--no-sklearn]

Rows: 1) 50 000 x 50, k = 12, full, a whole fit; 2) 50 000 x 50, k = 50, full; 3) 1 048 576 x 64, k = 64, full; 4) 1 048 576 x 256,
k = 256, diag -- rows 2 to 4 one EM iteration (E-step, M-step and the host's Cholesky step, which both sides share).  The sides
alternate inside one run and the median of --reps is kept.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cryo_ralib_amd import gmm  # noqa: E402

ROWS = {1: (50000, 50, 12, "full", "fit"), 2: (50000, 50, 50, "full", "iteration"), 3: (1048576, 64, 64, "full", "iteration"),
        4: (1048576, 256, 256, "diag", "iteration")}


def blobs(n, d, k, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    cent = torch.randn(k, d, generator=g) * 3.0
    scale = 0.5 + torch.rand(k, d, generator=g)
    lab = torch.randint(0, k, (n,), generator=g)
    return (cent[lab] + torch.randn(n, d, generator=g) * scale[lab]).float().contiguous(), lab.numpy()


class TorchSide:
    """the E- and M-step in float64 torch on the device: (X - mu_c) @ PC_c per component, torch.logsumexp, resp.T @ X and a
    per-component weighted diff^T diff"""

    def __init__(self, X, k, cov):
        self.X, self.k, self.ct = X.double(), k, cov
        self.n, self.d = X.shape

    def estep(self, p):
        dev = self.X.device
        mu, pc, off = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p.means, p.pc, p.offset))
        lp = torch.empty((self.n, self.k), dtype=torch.float64, device=dev)
        for c in range(self.k):
            y = (self.X - mu[c]) @ pc[c] if self.ct == "full" else (self.X - mu[c]) * pc[c]
            lp[:, c] = off[c] - 0.5 * (y * y).sum(dim=1)
        lpn = torch.logsumexp(lp, dim=1)
        self.log_resp = lp - lpn[:, None]
        return float(lpn.sum().item()) / self.n

    def mstep_log(self, reg):
        r = self.log_resp.exp()
        nk = r.sum(dim=0) + 10 * np.finfo(np.float64).eps
        means = r.T @ self.X / nk[:, None]
        if self.ct == "diag":
            cov = r.T @ (self.X * self.X) / nk[:, None] - means ** 2 + reg
        else:
            cov = torch.empty((self.k, self.d, self.d), dtype=torch.float64, device=self.X.device)
            for c in range(self.k):
                diff = self.X - means[c]
                cov[c] = (r[:, c] * diff.T) @ diff / nk[c]
                cov[c].diagonal().add_(reg)
        return nk.cpu().numpy(), means.cpu().numpy(), cov.cpu().numpy()


def iteration(B, p, cov):
    B.estep(p)
    return gmm._Params(*B.mstep_log(1e-6), cov)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "gmm_bench.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    for row in (int(v) for v in args.rows.split(",")):
        n, d, k, cov, what = ROWS[row]
        Xc, lab = blobs(n, d, k, row)
        X = Xc.to(dev)
        B, T = gmm._Device(X, k, cov), TorchSide(X, k, cov)
        p0 = gmm._Params(*B.mstep(B.one_hot(lab), False, 1e-6), cov)
        # bytes one iteration has to move at least: X once per step, the [n][k] table written and read
        nbytes = 2 * n * d * 4 + 2 * n * k * 8
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        sides = {"kernels": lambda: iteration(B, p0, cov), "torch_f64": lambda: iteration(T, p0, cov), "copy": lambda: dst.copy_(src)}
        if what == "fit":
            sides["kernels"] = lambda: gmm.gmm(X, k, covariance_type=cov, init_params=lab, max_iter=20, tol=0.0)
            fit_p = [p0]

            def torch_fit():
                p = p0
                for _ in range(20):
                    p = iteration(T, p, cov)
                fit_p[0] = p
            sides["torch_f64"] = torch_fit
        for f in sides.values():
            f()                                         # warm-up
        ms = {name: [] for name in sides}
        for _ in range(args.reps):
            for name, f in sides.items():
                ms[name].append(timed(f))
        rec = dict(row=row, n=n, d=d, k=k, covariance_type=cov, measured=what + (" (20 iterations, given start)" if what == "fit" else ""),
                   bytes_copied=nbytes, reps=args.reps, **{name + "_ms": statistics.median(v) for name, v in ms.items()})
        if what == "fit" and not args.no_sklearn:
            try:
                import warnings
                from sklearn.mixture import GaussianMixture
                X64 = Xc.numpy().astype(np.float64)
                t = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    GaussianMixture(k, covariance_type=cov, tol=0.0, max_iter=20, init_params="random", random_state=0).fit(X64)
                rec["sklearn_cpu_ms"] = (time.perf_counter() - t) * 1e3
                rec["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0"))
            except ImportError:
                rec["sklearn_cpu_ms"] = None
        rec["met"] = bool(rec["kernels_ms"] < rec["torch_f64_ms"])
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del B, T, X, src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=results), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
