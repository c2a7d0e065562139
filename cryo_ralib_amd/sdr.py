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

Applying a fitted model (what the reference returns G, A, B and the mean for).  A model is (mean [p][q] f32, A [p][p0], B [q][q0],
G [m][r] or None) with m = p0 q0; A, B and G are float64 on the host and rounded to float32 once when they go to the device.
    transform(x)     U = vec(A^T (x - mean) B); f = U G (2SDR) or f = U (MPCA, G is None): the launches of the fit itself
                     (ra_sdr_project, ra_sdr_factors), so the factors of the fitted stack come out bit for bit.
    reconstruct(f)   c = G f (MPCA: c = f), C = reshape(c, p0, q0) with (a, b) -> a q0 + b, x^ = mean + A C B^T rounded to float32
                     once; add_mean=False leaves the mean out.  One kernel, ra_sdr_reconstruct: c, C and C B^T stay in LDS.
    denoise(x)       reconstruct(transform(x)); residuals=True adds resid_i = sum over pixels of (x_i - x^_i)^2, x^_i the float32
                     value written, the difference and the sum in double in an order fixed by (p, q).
    eigenimages      image j is reconstruct(e_j, add_mean=False), j < r (MPCA: j < m).
x^ depends on the subspaces only (the column signs of A, B and G cancel), so it compares with the reference without alignment.
Domain: the fit's p, q, p0, q0; 1 <= r <= min(256, m); n >= 0 (n == 0 gives empty results).  The numpy backend computes in float64
and returns the input's precision: a float32 stack is centred in float32, as the device does, and x^ rounded once; float64 images
and factors stay float64 throughout (x^ unrounded: what the device is held against).

    python -m cryo_ralib_amd.sdr STACK OUT.npz ... [--denoised OUT_STACK] [--residuals] [--eigenimages FILE [--n_eig K]]
    python -m cryo_ralib_amd.sdr STACK OUT.npz --model MODEL.npz [--batch 4096] [--params FILE] [--denoised ...] ...
--model applies the model of an earlier OUT.npz instead of fitting one, reading the stack --batch images at a time.
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


# ---- applying a fitted model

class SdrModel:
    """mean [p][q] float32, A [p][p0], B [q][q0] and G [p0 q0][r] (None: MPCA) float64; width is the length of a factor row"""

    def __init__(self, mean, A, B, G=None):
        self.mean = np.ascontiguousarray(mean, np.float32)
        self.A, self.B = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(B, np.float64)
        self.G = None if G is None else np.ascontiguousarray(G, np.float64)
        if self.mean.ndim != 2 or self.A.ndim != 2 or self.B.ndim != 2 or (self.G is not None and self.G.ndim != 2):
            raise SdrError("a model is mean [p][q], A [p][p0], B [q][q0] and G [p0 q0][r] or None")
        self.p, self.q = self.mean.shape
        self.p0, self.q0 = self.A.shape[1], self.B.shape[1]
        if self.A.shape[0] != self.p or self.B.shape[0] != self.q:
            raise SdrError("A has %d rows and B %d, the mean is %d x %d" % (self.A.shape[0], self.B.shape[0], self.p, self.q))
        check_domain(1, self.p, self.q, self.p0, self.q0)
        self.m = self.p0 * self.q0
        if self.G is not None and not (self.G.shape[0] == self.m and 1 <= self.G.shape[1] <= min(256, self.m)):
            raise SdrError("G must be [%d][r] with 1 <= r <= %d, got %s" % (self.m, min(256, self.m), self.G.shape))
        self.width = self.m if self.G is None else self.G.shape[1]

    @classmethod
    def from_result(cls, res):
        return cls(res.mean, res.A, res.B, res.G)

    @classmethod
    def load(cls, path):
        """from a file written by save() or by the tool (OUT.npz); a G with zero columns means MPCA"""
        with np.load(path) as z:
            missing = [k for k in ("mean", "A", "B", "G") if k not in z.files]
            if missing:
                raise SdrError("%s holds no %s: not a model" % (path, ", ".join(missing)))
            return cls(z["mean"], z["A"], z["B"], z["G"] if z["G"].shape[-1] else None)

    def arrays(self):
        """the model's part of an OUT.npz"""
        return dict(G=self.G if self.G is not None else np.zeros((self.m, 0)), A=self.A, B=self.B, mean=self.mean,
                    p0=np.int64(self.p0), q0=np.int64(self.q0), r=np.int64(0 if self.G is None else self.width))

    def save(self, path):
        np.savez(path, **self.arrays())


def _checked(x, tail, backend, what):
    """x [n] + tail as the backend takes it: a contiguous float32 CUDA tensor, or a float32 / float64 numpy copy"""
    if backend == "device":
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise SdrError("backend 'device' takes %s as a contiguous float32 CUDA tensor" % what)
    elif backend == "numpy":
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        x = np.array(x, np.float64 if x.dtype == np.float64 else np.float32)
    else:
        raise SdrError("backend is 'device' or 'numpy', got %r" % (backend,))
    if x.ndim != 1 + len(tail) or tuple(x.shape[1:]) != tail:
        raise SdrError("%s are [n]%s, got shape %s" % (what, "".join("[%d]" % t for t in tail), tuple(x.shape)))
    return x


def _checked_out(out, x, shape):
    if out is not None and not (type(out) is type(x) and out.dtype == x.dtype and tuple(out.shape) == shape
                                and (isinstance(out, np.ndarray) or (out.device == x.device and out.is_contiguous()))):
        raise SdrError("out must be a contiguous [%d][%d][%d] array of the input's kind, type and device" % shape)


def _numpy_transform(x, model):
    X = (x - model.mean.astype(x.dtype)).astype(np.float64)
    U = np.einsum("ra,irc,cb->iab", model.A, X, model.B).reshape(x.shape[0], model.m)
    return U if model.G is None else U @ model.G


def _numpy_reconstruct(f, model, add_mean):
    c = f.astype(np.float64) if model.G is None else f.astype(np.float64) @ model.G.T
    xh = np.matmul(np.matmul(model.A, c.reshape(-1, model.p0, model.q0)), model.B.T)
    return xh + model.mean.astype(np.float64) if add_mean else xh


def _device_transform(x, model):
    if x.shape[0] == 0:
        return x.new_empty((0, model.width))
    D = _Device(x)
    with D.torch.cuda.device(D.dev):
        U = D.project(D._f32(model.mean), model.A, model.B)
        return U if model.G is None else D.factors(U, model.G)


def _device_reconstruct(f, model, add_mean, out, images=None):
    """x^ [n][p][q] of the factors f; with the images also resid [n] float64 (else None)"""
    n = int(f.shape[0])
    if out is None:
        out = f.new_empty((n, model.p, model.q))
    D = _Device(out)
    resid = D.torch.empty(n, dtype=D.torch.float64, device=D.dev) if images is not None else None
    with D.torch.cuda.device(D.dev):
        G, A, B = (D._f32(M) if M is not None else None for M in (model.G, model.A, model.B))
        mean = D._f32(model.mean) if add_mean else None
        D.call("ra_sdr_reconstruct", ptr(f), n, model.width, ptr(G), model.p0, model.q0, ptr(A), model.p, ptr(B), model.q,
               ptr(mean), ptr(images), ptr(out), ptr(resid))
    return out, resid


def transform(images, model, backend="device"):
    """factors [n][model.width] of images [n][p][q] (float64 from the numpy backend)"""
    x = _checked(images, (model.p, model.q), backend, "images")
    return _device_transform(x, model) if backend == "device" else _numpy_transform(x, model)


def reconstruct(factors, model, add_mean=True, out=None, backend="device"):
    """x^ [n][p][q] of factors [n][model.width], written to out if one is given"""
    f = _checked(factors, (model.width,), backend, "factors")
    _checked_out(out, f, (int(f.shape[0]), model.p, model.q))
    if backend == "device":
        return _device_reconstruct(f, model, add_mean, out)[0]
    xh = _numpy_reconstruct(f, model, add_mean).astype(f.dtype)
    if out is None:
        return xh
    out[...] = xh
    return out


def denoise(images, model, residuals=False, out=None, backend="device"):
    """reconstruct(transform(images)); with residuals=True (x^, resid [n] float64)"""
    x = _checked(images, (model.p, model.q), backend, "images")
    _checked_out(out, x, tuple(int(s) for s in x.shape))
    if backend == "device":
        xh, resid = _device_reconstruct(_device_transform(x, model), model, True, out, x if residuals else None)
    else:
        xh = _numpy_reconstruct(_numpy_transform(x, model), model, True)
        resid = ((x.astype(np.float64) - xh.astype(np.float32)) ** 2).sum(axis=(1, 2)) if residuals else None
        if out is not None:
            out[...] = xh
            xh = out
        else:
            xh = xh.astype(x.dtype)
    return (xh, resid) if residuals else xh


def eigenimages(model, count=None, backend="device"):
    """the first count (default: all model.width) basis images [count][p][q]: reconstruct(e_j, add_mean=False)"""
    count = model.width if count is None else count
    if not (_common.is_int(count) and 1 <= count <= model.width):
        raise SdrError("count must be an integer in 1 .. %d, got %r" % (model.width, count))
    E = np.eye(count, model.width, dtype=np.float32 if backend == "device" else np.float64)
    if backend == "device":
        import torch
        E = torch.from_numpy(E).to(torch.device("cuda", torch.cuda.current_device()))
    return reconstruct(E, model, add_mean=False, backend=backend)


# ---- command line

def read_params(path, n):
    """[n][4] (alpha, sx, sy, mirror) from a params.txt (idx angle_psi shift_x shift_y mirror class, rows in any order) or an
    initial2Dparams.txt (alpha sx sy mirror, in stack order)"""
    return _common.read_params(path, n, SdrError)


def _apply(batches, model, denoised, residuals):
    """the model on device batches [b][p][q]: factors [n][width], and as asked the denoised stack (else None) and
    {"resid", "resid_rel"} (else {}), on the host.  resid_rel = resid / sum (x - mean)^2, 0 / 0 -> 0"""
    F, X, R, E = [], [], [], []
    for x in batches:
        f = _device_transform(x, model)
        F.append(f.cpu().numpy())
        if denoised or residuals:
            xh, resid = _device_reconstruct(f, model, True, None, x if residuals else None)
            if denoised:
                X.append(xh.cpu().numpy())
            if residuals:
                R.append(resid.cpu().numpy())
                E.append(((x - x.new_tensor(model.mean)).double() ** 2).sum(dim=(1, 2)).cpu().numpy())
    extra = {}
    if residuals:
        resid, energy = np.concatenate(R), np.concatenate(E)
        extra = dict(resid=resid, resid_rel=np.divide(resid, energy, out=np.zeros_like(resid), where=energy != 0))
    return np.concatenate(F), np.concatenate(X) if denoised else None, extra


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.sdr")
    ap.add_argument("stack", help=".hdf, .mrcs or .npy stack")
    ap.add_argument("output", help="OUT.npz")
    ap.add_argument("--p0", type=int, default=None, help="default 25"); ap.add_argument("--q0", type=int, default=None, help="default 25")
    ap.add_argument("--r", type=int, default=None, help="default 50")
    ap.add_argument("--params", default=None, help="params.txt or initial2Dparams.txt: rot_shift2D every image first")
    ap.add_argument("--mpca", action="store_true", help="MPCA only (factors = U, no second stage)")
    ap.add_argument("--max_iter", type=int, default=None, help="default 30"); ap.add_argument("--tol", type=float, default=None, help="default 1e-7")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--denoised", default=None, help="OUT_STACK.{hdf,mrcs,npy}: the denoised (with --params: aligned) stack")
    ap.add_argument("--residuals", action="store_true", help="resid and resid_rel per image in OUT.npz")
    ap.add_argument("--eigenimages", default=None, help="FILE.{hdf,mrcs,npy}: the basis images")
    ap.add_argument("--n_eig", type=int, default=None, help="write the first K basis images (default: all)")
    ap.add_argument("--model", default=None, help="MODEL.npz (an earlier OUT.npz): apply its model instead of fitting one")
    ap.add_argument("--batch", type=int, default=None, help="with --model: images read and processed at a time (default 4096)")
    args = ap.parse_args(argv)
    fit_options = [o for o in ("p0", "q0", "r", "max_iter", "tol") if getattr(args, o) is not None] + (["mpca"] if args.mpca else [])
    if args.model and fit_options:
        ap.error("--model brings the fit with it: drop --" + ", --".join(fit_options))
    if args.n_eig is not None and not args.eigenimages:
        ap.error("--n_eig needs --eigenimages")
    if args.batch is not None and (not args.model or args.batch < 1):
        ap.error("--batch needs --model and a positive count")
    from . import stackio
    model = None
    if args.model:
        try:
            model = SdrModel.load(args.model)
            n, (p, q) = stackio.stack_size(args.stack), stackio.read_stack(args.stack, 0, 1).shape[1:]
        except (ValueError, OSError) as e:
            raise SystemExit("error: %s" % e)
        if (p, q) != (model.p, model.q):
            ap.error("%s holds a model of %d x %d images, the stack's are %d x %d" % (args.model, model.p, model.q, p, q))
    p0, q0, r, max_iter, tol = (d if v is None else v for v, d in ((args.p0, 25), (args.q0, 25), (args.r, 50), (args.max_iter, 30),
                                                                 (args.tol, 1e-7)))
    _common.require_gpu("no GPU visible: the reduction has no CPU path outside backend='numpy'")
    import torch
    from . import api
    dev = torch.device("cuda", args.device)
    if model is None:
        data = np.ascontiguousarray(stackio.read_stack(args.stack), np.float32)
        if data.ndim != 3:
            raise SystemExit("%s: not a stack of 2-D images" % args.stack)
        n, p, q = data.shape
    try:
        if model is None:
            check_domain(n, p, q, p0, q0, None if args.mpca else r, max_iter)
        prm = read_params(args.params, n) if args.params else None
    except (SdrError, OSError) as e:
        raise SystemExit("error: %s" % e)
    if prm is not None and p != q:
        raise SystemExit("error: --params needs square images, got %d x %d" % (p, q))

    def aligned(x, first):
        return api.rot_shift2d(x, prm[first:first + x.shape[0]]) if prm is not None else x

    if model is None:
        m = p0 * q0
        need = data.nbytes * (2 if prm is not None else 1) + n * m * 4 * 2 + (64 << 20)
        free, _ = torch.cuda.mem_get_info(dev)
        if need > free:
            raise SystemExit("error: the stack needs about %.2f GB on the device, %.2f GB are free; the reduction does not chunk"
                             % (need / 1e9, free / 1e9))
        x = _common.to_device(data, args.device)
        with torch.cuda.device(dev):
            x = aligned(x, 0)
            res = mpca(x, p0, q0, max_iter, tol) if args.mpca else two_sdr(x, p0, q0, r, max_iter, tol)
        out = dict(factors=res.factors, G=res.G if res.G is not None else np.zeros((m, 0)), A=res.A, B=res.B,
                   mean=res.mean, iterations=np.int64(res.iterations), energies=np.asarray(res.energies, np.float64),
                   p0=np.int64(p0), q0=np.int64(q0), r=np.int64(0 if args.mpca else r))
        summary = "%d iterations, factors %s" % (res.iterations, res.factors.shape)
        model, batches = SdrModel.from_result(res), [x]
    else:
        step = args.batch or 4096
        batches = (aligned(_common.to_device(stackio.read_stack(args.stack, f, min(n, f + step)), args.device), f) for f in range(0, n, step))
        out, summary = model.arrays(), "model %s" % args.model
    with torch.cuda.device(dev):
        if args.model or args.denoised or args.residuals:
            factors, denoised, extra = _apply(batches, model, bool(args.denoised), args.residuals)
            out.update(extra)
            if args.model:
                out["factors"] = factors
                summary += ", factors %s" % (factors.shape,)
            if args.denoised:
                stackio.write_stack(args.denoised, denoised)
                summary += ", denoised -> %s" % args.denoised
            if args.residuals:
                for key in ("resid", "resid_rel"):
                    summary += ", %s 50/90/99 %% %s" % (key, " ".join("%.4g" % v for v in np.quantile(out[key], (0.5, 0.9, 0.99))))
        if args.eigenimages:
            try:
                stackio.write_stack(args.eigenimages, eigenimages(model, args.n_eig).cpu().numpy())
            except SdrError as e:
                raise SystemExit("error: %s" % e)
            summary += ", eigenimages -> %s" % args.eigenimages
    np.savez(args.output, **out)
    print("%s: %d images %d x %d, %s" % (args.output, n, p, q, summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
