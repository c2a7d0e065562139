"""Two-stage dimension reduction (2SDR) and MPCA of an image stack, on the GPU (utils_ralib.py MPCA / TwoSDR).

    python -m cryo_ralib_amd.sdr STACK OUT.npz --p0 25 --q0 25 --r 50 [--params FILE] [--mpca] [--max_iter 30] [--tol 1e-7]

The contract (utils_ralib.py:436-564): Y = arr - mean over the stack, X_i image i of Y (p x q).  SA = sum X_i^T X_i; then per
iteration B = top-q0 eigenvectors of SA, SB = sum (X_i B)(X_i B)^T, A = top-p0 eigenvectors of SB, SA = sum (A^T X_i)^T (A^T X_i),
and from the second iteration on the loop stops when (E_k - E_{k-1}) / n < tol (signed), E_k = sum ||A_k^T X_i B_k||_F^2 = the sum
of the top p0 eigenvalues of that iteration's SB.  MPCA returns U (U_i = vec(A^T X_i B), (a, b) -> a q0 + b), A, B, mean;
2SDR also G = top-r eigenvectors of C = sum u_i u_i^T and factors U G.

The Grams, the projection and the factors run in the HIP kernels behind ra_sdr_* (csrc/ralign_sdr.h); the loop and the eigen
solves (numpy.linalg.eigh in float64, descending) run here.  backend="numpy" runs the same loop with float64 numpy products: it
is the CPU checker.  Eigenvector signs follow one convention: in every column the entry of largest magnitude is positive (the
first such entry on ties).  The reference's ARPACK eigs / svds pick signs at random, so every comparison with it is sign-invariant.

Domain: 1 <= p, q <= 256; 1 <= p0 <= min(p, 64); 1 <= q0 <= min(q, 64); p0 q0 <= 2048; 1 <= r <= min(256, p0 q0 - 1, n - 1).
ARPACK (the reference) additionally needs p0 < p - 1 and q0 < q - 1; eigh has no such limit.
"""
import argparse
import sys

import numpy as np

from . import _common
from ._common import Launcher, ptr


class SdrError(ValueError):
    """an input outside the supported domain, or a malformed params file"""


class SdrResult:
    """factors [n][r] (2SDR) or [n][p0 q0] (MPCA), G [p0 q0][r] (2SDR only, else None), A [p][p0], B [q][q0] (float64), mean
    [p][q] (float32), iterations (loop passes run), energies (E_k per pass, float64)"""

    def __init__(self, factors, G, A, B, mean, iterations, energies):
        self.factors, self.G, self.A, self.B, self.mean = factors, G, A, B, mean
        self.iterations, self.energies = iterations, energies


def check_domain(n, p, q, p0, q0, r=None, max_iter=30):
    """raise SdrError unless (n, p, q, p0, q0[, r]) is inside the supported domain"""
    def need(ok, msg):
        if not ok:
            raise SdrError(msg)
    for name, v in (("n", n), ("p", p), ("q", q), ("p0", p0), ("q0", q0), ("max_iter", max_iter)) + ((("r", r),) if r is not None else ()):
        need(isinstance(v, (int, np.integer)), "%s must be an integer, got %r" % (name, v))
    need(n >= 1, "need at least one image, got n = %d" % n)
    need(1 <= p <= 256 and 1 <= q <= 256, "images must be p x q with 1 <= p, q <= 256, got %d x %d" % (p, q))
    need(1 <= p0 <= min(p, 64), "need 1 <= p0 <= min(p, 64) = %d, got p0 = %d" % (min(p, 64), p0))
    need(1 <= q0 <= min(q, 64), "need 1 <= q0 <= min(q, 64) = %d, got q0 = %d" % (min(q, 64), q0))
    need(p0 * q0 <= 2048, "need p0 q0 <= 2048, got %d" % (p0 * q0))
    need(max_iter >= 1, "need max_iter >= 1, got %d" % max_iter)
    if r is not None:
        rmax = min(256, p0 * q0 - 1, n - 1)
        need(1 <= r <= rmax, "need 1 <= r <= min(256, p0 q0 - 1, n - 1) = %d, got r = %d" % (rmax, r))


def fix_signs(V):
    """flip columns of V so that the entry of largest magnitude of each is positive (the first such entry on ties)"""
    V = np.array(V, np.float64, copy=True)
    if V.size == 0:
        return V
    idx = np.argmax(np.abs(V), axis=0)
    s = np.sign(V[idx, np.arange(V.shape[1])])
    s[s == 0] = 1.0
    return V * s


def top_eig(S, k):
    """(eigenvalues, eigenvectors) of the k largest eigenvalues of the symmetric matrix S, descending, signs fixed"""
    w, V = np.linalg.eigh(np.asarray(S, np.float64))
    order = np.argsort(w, kind="stable")[::-1][:k]
    return w[order], fix_signs(V[:, order])


def _loop(n, p0, q0, max_iter, tol, gram0, gram1, gram2):
    """the MPCA alternation; returns A, B, energies.  The last pass's SA is never used, so it is not computed."""
    SA = gram0()
    energies = []
    A = B = None
    for k in range(max_iter):
        _, B = top_eig(SA, q0)
        w, A = top_eig(gram1(B), p0)
        energies.append(float(np.sum(w)))
        if k > 0 and (energies[-1] - energies[-2]) / n < tol:
            break
        if k + 1 < max_iter:
            SA = gram2(A)
    return A, B, energies


# ---- CPU checker (float64 numpy)

def _numpy_run(images, p0, q0, r, max_iter, tol):
    arr = np.asarray(images, np.float32)
    n, p, q = arr.shape
    mean = arr.astype(np.float64).mean(axis=0).astype(np.float32)
    X = (arr - mean).astype(np.float64)                      # centred in fp32, as the device does
    g0 = lambda: X.reshape(n * p, q).T @ X.reshape(n * p, q)

    def g1(B):
        T = (X @ B).transpose(1, 0, 2).reshape(p, -1)
        return T @ T.T

    def g2(A):
        S = np.einsum("ra,irc->iac", A, X).reshape(-1, q)
        return S.T @ S
    A, B, energies = _loop(n, p0, q0, max_iter, tol, g0, g1, g2)
    U = np.einsum("ra,irc,cb->iab", A, X, B).reshape(n, p0 * q0)
    if r is None:
        return SdrResult(U, None, A, B, mean, len(energies), energies)
    _, G = top_eig(U.T @ U, r)
    return SdrResult(U @ G, G, A, B, mean, len(energies), energies)


# ---- device

class _Device:
    """thin launcher of the ra_sdr_* entries on the current stream of the images' device"""

    def __init__(self, images):
        L = Launcher(images)
        self.torch, self.api, self.lib, self.dev, self.stream, self.call = L.torch, L.api, L.lib, L.dev, L.stream, L.call
        self.x = images
        self.n, self.p, self.q = (int(s) for s in images.shape)

    def _f32(self, M):
        return self.torch.from_numpy(np.ascontiguousarray(M, np.float32)).to(self.dev)

    def mean(self):
        m = self.torch.empty((self.p, self.q), dtype=self.torch.float32, device=self.dev)
        self.call("ra_sdr_mean", ptr(self.x), self.n, self.p, self.q, ptr(m))
        return m

    def gram(self, x, n, p, q, mean, form, P=None):
        d = p if form == 1 else q
        g = self.torch.empty((d, d), dtype=self.torch.float64, device=self.dev)
        Pd = self._f32(P) if P is not None else None
        self.call("ra_sdr_gram", ptr(x), n, p, q, ptr(mean), form, ptr(Pd), 0 if P is None else int(P.shape[1]), ptr(g))
        return g.cpu().numpy()

    def project(self, mean, A, B):
        p0, q0 = A.shape[1], B.shape[1]
        U = self.torch.empty((self.n, p0 * q0), dtype=self.torch.float32, device=self.dev)
        Ad, Bd = self._f32(A), self._f32(B)
        self.call("ra_sdr_project", ptr(self.x), self.n, self.p, self.q, ptr(mean), ptr(Ad), p0, ptr(Bd), q0, ptr(U))
        return U

    def factors(self, U, G):
        n, m = (int(s) for s in U.shape)
        r = G.shape[1]
        F = self.torch.empty((n, r), dtype=self.torch.float32, device=self.dev)
        Gd = self._f32(G)
        self.call("ra_sdr_factors", ptr(U), n, m, ptr(Gd), r, ptr(F))
        return F


def _device_run(images, p0, q0, r, max_iter, tol):
    D = _Device(images)
    n, p, q = D.n, D.p, D.q
    with D.torch.cuda.device(D.dev):
        mean = D.mean()
        A, B, energies = _loop(n, p0, q0, max_iter, tol,
                               lambda: D.gram(D.x, n, p, q, mean, 0),
                               lambda B: D.gram(D.x, n, p, q, mean, 1, B),
                               lambda A: D.gram(D.x, n, p, q, mean, 2, A))
        U = D.project(mean, A, B)
        mean_np = mean.cpu().numpy()
        if r is None:
            return SdrResult(U.cpu().numpy(), None, A, B, mean_np, len(energies), energies)
        _, G = top_eig(D.gram(U, n, 1, p0 * q0, None, 0), r)
        F = D.factors(U, G)
        return SdrResult(F.cpu().numpy(), G, A, B, mean_np, len(energies), energies)


def _run(images, p0, q0, r, max_iter, tol, backend):
    if backend == "device":
        import torch
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32 and images.is_contiguous()):
            raise SdrError("backend 'device' takes a contiguous float32 CUDA tensor [n][p][q]")
    elif backend != "numpy":
        raise SdrError("backend is 'device' or 'numpy', got %r" % (backend,))
    if images.ndim != 3:
        raise SdrError("images are [n][p][q], got shape %s" % (tuple(images.shape),))
    n, p, q = (int(s) for s in images.shape)
    check_domain(n, p, q, p0, q0, r, max_iter)
    if backend == "numpy":
        if not isinstance(images, np.ndarray):
            images = images.detach().cpu().numpy()
        return _numpy_run(images, p0, q0, r, max_iter, tol)
    return _device_run(images, p0, q0, r, max_iter, tol)


def two_sdr(images, p0, q0, r, max_iter=30, tol=1e-7, backend="device"):
    """TwoSDR(arr, p0, q0, r): SdrResult with factors [n][r] and G [p0 q0][r]"""
    return _run(images, p0, q0, r, max_iter, tol, backend)


def mpca(images, p0, q0, max_iter=30, tol=1e-7, backend="device"):
    """MPCA(arr, p0, q0): SdrResult with factors = U [n][p0 q0] and G None"""
    return _run(images, p0, q0, None, max_iter, tol, backend)


# ---- command line

def read_params(path, n):
    """[n][4] (alpha, sx, sy, mirror) from a params.txt (idx angle_psi shift_x shift_y mirror class, rows in any order) or an
    initial2Dparams.txt (alpha sx sy mirror, in stack order)"""
    return _common.read_params(path, n, SdrError)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.sdr")
    ap.add_argument("stack", help=".hdf, .mrcs or .npy stack")
    ap.add_argument("output", help="OUT.npz")
    ap.add_argument("--p0", type=int, default=25); ap.add_argument("--q0", type=int, default=25); ap.add_argument("--r", type=int, default=50)
    ap.add_argument("--params", default=None, help="params.txt or initial2Dparams.txt: rot_shift2D every image first")
    ap.add_argument("--mpca", action="store_true", help="MPCA only (factors = U, no second stage)")
    ap.add_argument("--max_iter", type=int, default=30); ap.add_argument("--tol", type=float, default=1e-7)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    _common.require_gpu("no GPU visible: the reduction has no CPU path outside backend='numpy'")
    import torch
    from . import api, stackio
    data = np.ascontiguousarray(stackio.read_stack(args.stack), np.float32)
    if data.ndim != 3:
        raise SystemExit("%s: not a stack of 2-D images" % args.stack)
    n, p, q = data.shape
    try:
        check_domain(n, p, q, args.p0, args.q0, None if args.mpca else args.r, args.max_iter)
        prm = read_params(args.params, n) if args.params else None
    except (SdrError, OSError) as e:
        raise SystemExit("error: %s" % e)
    if prm is not None and p != q:
        raise SystemExit("error: --params needs square images, got %d x %d" % (p, q))
    dev = torch.device("cuda", args.device)
    m = args.p0 * args.q0
    need = data.nbytes * (2 if prm is not None else 1) + n * m * 4 * 2 + (64 << 20)
    free, _ = torch.cuda.mem_get_info(dev)
    if need > free:
        raise SystemExit("error: the stack needs about %.2f GB on the device, %.2f GB are free; the reduction does not chunk"
                         % (need / 1e9, free / 1e9))
    x = _common.to_device(data, args.device)
    with torch.cuda.device(dev):
        if prm is not None:
            x = api.rot_shift2d(x, prm)
        res = (mpca(x, args.p0, args.q0, args.max_iter, args.tol) if args.mpca
               else two_sdr(x, args.p0, args.q0, args.r, args.max_iter, args.tol))
    np.savez(args.output, factors=res.factors, G=res.G if res.G is not None else np.zeros((m, 0)), A=res.A, B=res.B,
             mean=res.mean, iterations=np.int64(res.iterations), energies=np.asarray(res.energies, np.float64),
             p0=np.int64(args.p0), q0=np.int64(args.q0), r=np.int64(0 if args.mpca else args.r))
    print("%s: %d images %d x %d, %d iterations, factors %s" % (args.output, n, p, q, res.iterations, res.factors.shape))
    return 0


if __name__ == "__main__":
    sys.exit(main())
