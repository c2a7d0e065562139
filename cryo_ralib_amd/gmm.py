"""Gaussian mixture of factors X [n][d] on the GPU (scikit-learn 1.7 GaussianMixture, covariance_type "full" and "diag").

    python -m cryo_ralib_amd.gmm IN OUT.npz --k K [--cov full|diag] [--key factors] [--init kmeans|random|LABELS.npy] [--n_init N]
                                 [--max_iter 100] [--tol 1e-3] [--reg_covar 1e-6] [--seed S] [--backend device|numpy]
                                 [--sweep K1,K2,...|LO:HI[:STEP]] [--truth FILE] [--min_proba P]
                                 [--stack STACK --params PARAMS --ou R --averages REFS.{hdf,mrcs,npy}]

IN is the OUT.npz of the sdr tool (--key factors) or of the tsne tool (--key embedding), or an [n][d] .npy.  OUT.npz holds the
model (weights, means, covariances, precisions_cholesky), labels, proba_max (the largest posterior of each particle),
log_likelihood (per sample), lower_bound, n_iter, converged, bic, aic and the options used.  --sweep fits every k of the list,
prints the table k / lower bound / iterations / BIC / AIC, stores it as sweep (and best_k: the least BIC, the smaller k on ties)
and writes the result of best_k, or of --k if given.  --min_proba P adds the mask keep = proba_max >= P and prints per class its
size and how many are kept; the class averages (--averages, as the kmeans tool's) are of the labels as they are.

The contract is sklearn's GaussianMixture(n_components, covariance_type, tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
init_params, random_state) on float64 data:
  Initialisation: rs = check_random_state(random_state).  "kmeans": the one-hot of the labels of kmeans(X, k, init="k-means++",
  n_init=1, max_iter=300, tol=1e-4, random_state=rs) (the RandomState instance is passed on); "random": rs.uniform(size=(n, k)),
  rows normalised; an int array [n] with values 0 .. k - 1: the one-hot of given labels (this project's extension).  Then one
  M-step.  With n_init > 1 every run draws from the same rs in turn.
  M-step: nk = sum_i r_ic + 10 eps, w = nk / sum nk, mu_c = sum_i r_ic x_i / nk_c; full: Sigma_c = sum_i r_ic (x_i - mu_c)
  (x_i - mu_c)^T / nk_c + reg_covar I, PC_c = (L_c^-1)^T with L_c the lower Cholesky factor; diag: sum_i r_ic x_i^2 / nk_c -
  mu_c^2 + reg_covar, PC_c = 1 / sqrt(Sigma_c).  A covariance that is not positive definite raises ValueError with sklearn's text.
  E-step: m_ic = |(x_i - mu_c)^T PC_c|^2 (diag: sum_t ((x_it - mu_ct) PC_ct)^2), log p_ic = -(d log 2 pi + m_ic) / 2 +
  log det PC_c + log w_c, log_prob_norm_i = logsumexp_c log p_ic, log_resp = log p - log_prob_norm; the lower bound is the mean of
  log_prob_norm.
  Loop: for it = 1 .. max_iter: E-step, M-step, change = lb - prev; converged when |change| < tol.  The run of the largest lower
  bound is kept (>, or the first), its parameters restored, and one final E-step gives labels = argmax_c log_resp (first index on
  ties).  A kept run that did not converge warns with sklearn's ConvergenceWarning text.
  Scores: score_samples = log_prob_norm, predict_proba = exp(log_resp), bic = -2 sum log_prob_norm + P log n, aic = -2 sum
  log_prob_norm + 2 P with P = k d (d + 1) / 2 + k d + k - 1 (full) or 2 k d + k - 1 (diag).
Not built: covariance_type "tied" and "spherical", init_params "k-means++" and "random_from_data", weights_init / means_init /
precisions_init, warm_start, BayesianGaussianMixture, sampling, multi-GPU.

Every n x k x d (diag) and n x k x d^2 (full) sum runs in the float64 HIP kernels behind ra_gmm_estep / ra_gmm_mstep
(csrc/ralign_gmm.h; the full E-step and covariance scatter on v_mfma_f64_16x16x4_f64).  The k Cholesky factors, log-determinants and
offsets are float64 numpy on the host; the host reads one double (the lower bound) and the k parameter sets per iteration.
backend="numpy" runs the same loop in float64 numpy: it is the CPU checker.

Domain: 1 <= k <= 256, k <= n <= 4194304, n k <= 2^28, 1 <= d <= 256 (full) or 2048 (diag), max_iter >= 1, n_init >= 1, tol >= 0,
reg_covar >= 0, finite input.  Anything else raises GmmError before anything is launched.
"""
import argparse
import sys
import warnings

import numpy as np

from . import _common
from . import kmeans as _km
from ._common import Launcher, is_int, is_real, ptr
from .kmeans import ConvergenceWarning, check_random_state

MAX_N, MAX_K, MAX_D_FULL, MAX_D_DIAG, MAX_NK = 4194304, 256, 256, 2048, 1 << 28
COV_TYPES = {"full": 0, "diag": 1}          # RA_GMM_FULL, RA_GMM_DIAG
ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
               "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale "
               "the input data.")
NOT_CONVERGED = ("Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or "
                 "check for degenerate data.")


class GmmError(ValueError):
    """an input outside the supported domain"""


class GmmResult:
    """weights [k], means [k][d], covariances and precisions_cholesky (full [k][d][d], diag [k][d]): float64; covariance_type;
    converged, n_iter, lower_bound and lower_bounds (the kept run's history); labels int32 [n]; init_labels (int32 [n], None for
    init_params="random"); log_prob float64 [n] (score_samples of the fitted data) and proba_max float64 [n]"""

    def __init__(self, covariance_type, weights, means, covariances, precisions_cholesky, converged, n_iter, lower_bound, lower_bounds,
                 labels, init_labels, log_prob, proba_max):
        self.covariance_type, self.weights, self.means, self.covariances = covariance_type, weights, means, covariances
        self.precisions_cholesky, self.converged, self.n_iter, self.lower_bound = precisions_cholesky, converged, n_iter, lower_bound
        self.lower_bounds, self.labels, self.init_labels, self.log_prob, self.proba_max = lower_bounds, labels, init_labels, log_prob, proba_max


def check_domain(n, d, n_components, covariance_type="full", max_iter=100, tol=1e-3, reg_covar=1e-6, n_init=1):
    """raise GmmError unless the shape and parameters are inside the supported domain"""
    def need(ok, msg):
        if not ok:
            raise GmmError(msg)
    need(covariance_type in COV_TYPES, "covariance_type is 'full' or 'diag', got %r" % (covariance_type,))
    for name, v in (("n", n), ("d", d), ("n_components", n_components), ("max_iter", max_iter), ("n_init", n_init)):
        need(is_int(v), "%s must be an integer, got %r" % (name, v))
    need(1 <= n_components <= MAX_K, "need 1 <= n_components <= %d, got %d" % (MAX_K, n_components))
    need(n_components <= n <= MAX_N, "need n_components = %d <= n <= %d points, got %d" % (n_components, MAX_N, n))
    need(n * n_components <= MAX_NK, "need n * n_components <= 2^28, got %d x %d" % (n, n_components))
    dmax = MAX_D_FULL if covariance_type == "full" else MAX_D_DIAG
    need(1 <= d <= dmax, "need 1 <= d <= %d features (%s), got %d" % (dmax, covariance_type, d))
    need(max_iter >= 1, "need max_iter >= 1, got %d" % max_iter)
    need(n_init >= 1, "need n_init >= 1, got %d" % n_init)
    need(is_real(tol) and tol >= 0, "need a finite tol >= 0, got %r" % (tol,))
    need(is_real(reg_covar) and reg_covar >= 0, "need a finite reg_covar >= 0, got %r" % (reg_covar,))


def n_parameters(model):
    """free parameters of the mixture (sklearn's _n_parameters)"""
    k, d = model.means.shape
    cov = k * d * (d + 1) // 2 if model.covariance_type == "full" else k * d
    return int(cov + k * d + k - 1)


# ---- host arithmetic shared by both backends (float64 numpy)

def precision_cholesky(cov, covariance_type):
    """PC_c = (L_c^-1)^T (full: upper triangular [k][d][d]) or 1 / sqrt(Sigma_c) (diag); ValueError with sklearn's text when a
    covariance is not positive definite"""
    cov = np.asarray(cov, np.float64)
    if covariance_type == "diag":
        if np.any(np.less_equal(cov, 0.0)) or not np.all(np.isfinite(cov)):
            raise ValueError(ILL_DEFINED)
        return 1.0 / np.sqrt(cov)
    if not np.all(np.isfinite(cov)):
        raise ValueError(ILL_DEFINED)
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError(ILL_DEFINED)
    k, d, _ = L.shape
    Y = np.zeros((k, d, d))                  # L^-1 by forward substitution, a row at a time for all components
    for i in range(d):
        r = -np.matmul(L[:, i:i + 1, :i], Y[:, :i, :])[:, 0, :]
        r[:, i] += 1.0
        Y[:, i, :] = r / L[:, i, i, None]
    return np.ascontiguousarray(np.transpose(Y, (0, 2, 1))) + 0.0


def log_det_cholesky(pc, covariance_type):
    if covariance_type == "diag":
        return np.sum(np.log(pc), axis=1)
    return np.sum(np.log(np.diagonal(pc, axis1=1, axis2=2)), axis=1)


def offsets(weights, pc, covariance_type):
    """[k] log w_c + log det PC_c - d / 2 log 2 pi"""
    d = pc.shape[1]
    return np.log(weights) + log_det_cholesky(pc, covariance_type) - 0.5 * d * np.log(2.0 * np.pi)


class _Params:
    def __init__(self, nk, means, cov, covariance_type):
        self.weights = nk / nk.sum()
        self.means, self.cov = means, cov
        self.pc = precision_cholesky(cov, covariance_type)
        self.offset = offsets(self.weights, self.pc, covariance_type)


# ---- CPU checker (float64 numpy)

class _Numpy:
    """the E- and M-step in float64 numpy"""

    def __init__(self, X, k, covariance_type):
        self.X = np.asarray(X, np.float64)
        self.n, self.d = self.X.shape
        self.k, self.ct = k, covariance_type
        self.log_resp = self.log_prob = self.labels = None

    def kmeans_labels(self, k, rs):
        return _km.kmeans(self.X, k, init="k-means++", n_init=1, max_iter=300, tol=1e-4, random_state=rs, backend="numpy").labels

    def log_p(self, p):
        lp = np.empty((self.n, self.k))
        for c in range(self.k):
            diff = self.X - p.means[c]
            y = diff @ p.pc[c] if self.ct == "full" else diff * p.pc[c]
            lp[:, c] = p.offset[c] - 0.5 * np.sum(y * y, axis=1)
        return lp

    def estep(self, p):
        lp = self.log_p(p)
        mx = np.max(lp, axis=1)
        self.log_prob = mx + np.log(np.sum(np.exp(lp - mx[:, None]), axis=1))
        self.labels = np.argmax(lp, axis=1).astype(np.int32)
        self.log_resp = lp - self.log_prob[:, None]
        return float(np.sum(self.log_prob) / self.n)

    def mstep(self, resp, log_domain, reg):
        X, d = self.X, self.d
        r = np.exp(resp) if log_domain else np.asarray(resp, np.float64)
        nk = r.sum(axis=0) + 10 * np.finfo(np.float64).eps
        means = r.T @ X / nk[:, None]
        if self.ct == "diag":
            return nk, means, r.T @ (X * X) / nk[:, None] - means ** 2 + reg
        cov = np.empty((self.k, d, d))
        for c in range(self.k):
            diff = X - means[c]
            cov[c] = (r[:, c] * diff.T) @ diff / nk[c]
            cov[c].flat[::d + 1] += reg
        return nk, means, cov

    def mstep_log(self, reg):
        return self.mstep(self.log_resp, True, reg)

    def one_hot(self, labels):
        r = np.zeros((self.n, self.k))
        r[np.arange(self.n), labels] = 1.0
        return r

    def resp_from(self, r):
        return r

    def labels_numpy(self):
        return self.labels.astype(np.int32)

    def log_prob_numpy(self):
        return self.log_prob

    def log_resp_numpy(self):
        return self.log_resp

    def log_resp_max(self):
        return np.max(self.log_resp, axis=1)


# ---- device

class _Device:
    """thin launcher of ra_gmm_estep / ra_gmm_mstep on the current stream of X's device"""

    def __init__(self, X, k, covariance_type):
        L = Launcher(X)
        torch = L.torch
        self.torch, self.api, self.lib, self.dev, self.stream, self.call = torch, L.api, L.lib, L.dev, L.stream, L.call
        self.X = X
        self.n, self.d = (int(s) for s in X.shape)
        self.k, self.ct, self.ctype = k, covariance_type, COV_TYPES[covariance_type]
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.log_resp = torch.empty((self.n, k), **f64)
        self.log_prob = torch.empty(self.n, **f64)
        self.labels = torch.empty(self.n, dtype=torch.int32, device=self.dev)
        self.sum = torch.empty(1, **f64)
        self.nk = torch.empty(k, **f64)
        self.means = torch.empty((k, self.d), **f64)
        self.cov = torch.empty((k, self.d, self.d) if covariance_type == "full" else (k, self.d), **f64)

    def kmeans_labels(self, k, rs):
        return _km.kmeans(self.X, k, init="k-means++", n_init=1, max_iter=300, tol=1e-4, random_state=rs, backend="device").labels

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(self.dev)

    def estep(self, p):
        means, pc, off = self._up(p.means), self._up(p.pc), self._up(p.offset)
        self.call("ra_gmm_estep", ptr(self.X), self.n, self.d, self.k, self.ctype, ptr(means), ptr(pc), ptr(off), ptr(self.log_resp),
                  ptr(self.log_prob), ptr(self.labels), ptr(self.sum))
        return float(self.sum.item()) / self.n

    def mstep(self, resp, log_domain, reg):
        self.call("ra_gmm_mstep", ptr(self.X), self.n, self.d, self.k, self.ctype, ptr(resp), int(bool(log_domain)), float(reg),
                  ptr(self.nk), ptr(self.means), ptr(self.cov))
        return self.nk.cpu().numpy(), self.means.cpu().numpy(), self.cov.cpu().numpy()

    def mstep_log(self, reg):
        return self.mstep(self.log_resp, True, reg)

    def one_hot(self, labels):
        torch = self.torch
        r = torch.zeros((self.n, self.k), dtype=torch.float64, device=self.dev)
        idx = torch.from_numpy(np.ascontiguousarray(labels, np.int64)).to(self.dev)
        r.scatter_(1, idx[:, None], 1.0)
        return r

    def resp_from(self, r):
        return self._up(r)

    def labels_numpy(self):
        return self.labels.cpu().numpy().astype(np.int32)

    def log_prob_numpy(self):
        return self.log_prob.cpu().numpy()

    def log_resp_numpy(self):
        return self.log_resp.cpu().numpy()

    def log_resp_max(self):
        return self.log_resp.max(dim=1).values.cpu().numpy()


# ---- the loop (sklearn BaseMixture.fit_predict)

def _fit(B, k, covariance_type, tol, reg_covar, max_iter, n_init, init, random_state):
    rs = check_random_state(random_state)
    best = None
    for _ in range(n_init):
        init_labels = None
        if isinstance(init, str) and init == "kmeans":
            init_labels = np.asarray(B.kmeans_labels(k, rs), np.int32)
            resp = B.one_hot(init_labels)
        elif isinstance(init, str):
            r = rs.uniform(size=(B.n, k))
            r /= r.sum(axis=1)[:, np.newaxis]
            resp = B.resp_from(r)
        else:
            init_labels = init.astype(np.int32)
            resp = B.one_hot(init_labels)
        p = _Params(*B.mstep(resp, False, reg_covar), covariance_type)
        del resp
        lb, hist, converged, it = -np.inf, [], False, 0
        for it in range(1, max_iter + 1):
            prev = lb
            lb = B.estep(p)
            p = _Params(*B.mstep_log(reg_covar), covariance_type)
            hist.append(lb)
            if abs(lb - prev) < tol:
                converged = True
                break
        if best is None or lb > best[1]:
            best = (p, lb, it, converged, hist, init_labels)
    p, lb, it, converged, hist, init_labels = best
    if not converged:
        warnings.warn(NOT_CONVERGED, ConvergenceWarning, stacklevel=3)
    B.estep(p)
    return GmmResult(covariance_type, p.weights, p.means, p.cov, p.pc, bool(converged), int(it), float(lb), np.asarray(hist, np.float64),
                     B.labels_numpy(), init_labels, B.log_prob_numpy(), np.exp(B.log_resp_max()))


def _resolve_init(init, n, k):
    if isinstance(init, str):
        if init not in ("kmeans", "random"):
            raise GmmError("init_params is 'kmeans', 'random' or an int array [n] of labels, got %r" % (init,))
        return init
    lab = init.detach().cpu().numpy() if hasattr(init, "detach") else np.asarray(init)
    if lab.shape != (n,) or not np.issubdtype(lab.dtype, np.integer):
        raise GmmError("init labels are [%d] integers, got %s %s" % (n, lab.dtype, lab.shape))
    if lab.min() < 0 or lab.max() >= k:
        raise GmmError("init labels are integers in 0 .. n_components - 1 = %d, got %d .. %d" % (k - 1, lab.min(), lab.max()))
    return lab.astype(np.int64)


def _backend(X, k, covariance_type, backend):
    return _Numpy(X, k, covariance_type) if backend == "numpy" else _Device(X, k, covariance_type)


def gmm(X, n_components, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params="kmeans",
        random_state=None, backend="device"):
    """Gaussian mixture of X [n][d] (a contiguous float32 CUDA tensor; a numpy array is copied to the device): GmmResult"""
    X = _common.as_input(X, backend, GmmError)
    n, d = (int(s) for s in X.shape)
    check_domain(n, d, n_components, covariance_type, max_iter, tol, reg_covar, n_init)
    init = _resolve_init(init_params, n, n_components)
    _common.check_random_state(random_state, GmmError)
    _common.check_finite(X, backend, GmmError)
    if backend == "numpy":
        return _fit(_Numpy(X, n_components, covariance_type), n_components, covariance_type, tol, reg_covar, max_iter, n_init, init, random_state)
    import torch
    with torch.cuda.device(X.device):
        return _fit(_Device(X, n_components, covariance_type), n_components, covariance_type, tol, reg_covar, max_iter, n_init, init,
                    random_state)


# ---- evaluation of a fitted model: one E-step

class _Model:
    def __init__(self, model):
        self.means = np.ascontiguousarray(model.means, np.float64)
        self.pc = np.ascontiguousarray(model.precisions_cholesky, np.float64)
        self.offset = offsets(np.asarray(model.weights, np.float64), self.pc, model.covariance_type)


def _evaluate(X, model, backend):
    X = _common.as_input(X, backend, GmmError)
    n, d = (int(s) for s in X.shape)
    k = int(model.means.shape[0])
    if model.means.shape != (k, d):
        raise GmmError("the model has %d features, X has %d" % (model.means.shape[1], d))
    check_domain(n, d, k, model.covariance_type)
    _common.check_finite(X, backend, GmmError)
    if backend == "numpy":
        B = _Numpy(X, k, model.covariance_type)
        B.estep(_Model(model))
        return B
    import torch
    with torch.cuda.device(X.device):
        B = _Device(X, k, model.covariance_type)
        B.estep(_Model(model))
        return B


def predict(X, model, backend="device"):
    """labels int32 [n]: argmax_c of the posterior, the first index on ties"""
    return _evaluate(X, model, backend).labels_numpy()


def predict_proba(X, model, backend="device"):
    """posterior probabilities float64 [n][k] = exp(log_resp)"""
    return np.exp(_evaluate(X, model, backend).log_resp_numpy())


def score_samples(X, model, backend="device"):
    """log-likelihood of every sample float64 [n] = log_prob_norm"""
    return _evaluate(X, model, backend).log_prob_numpy()


def score(X, model, backend="device"):
    """mean log-likelihood"""
    lp = score_samples(X, model, backend)
    return float(np.sum(lp) / lp.size)


def _ic(log_prob, model, penalty):
    return float(-2.0 * np.sum(log_prob) + n_parameters(model) * penalty)


def bic(X, model, backend="device"):
    """Bayesian information criterion: -2 sum log_prob_norm + P log n"""
    lp = score_samples(X, model, backend)
    return _ic(lp, model, np.log(lp.size))


def aic(X, model, backend="device"):
    """Akaike information criterion: -2 sum log_prob_norm + 2 P"""
    return _ic(score_samples(X, model, backend), model, 2.0)


# ---- sweep over k

class SweepRow:
    """one k of a sweep: k, lower_bound, n_iter, converged, bic, aic, labels int32 [n] and the model (GmmResult)"""

    def __init__(self, k, fit):
        self.k, self.model, self.labels = int(k), fit, fit.labels
        self.lower_bound, self.n_iter, self.converged = fit.lower_bound, fit.n_iter, fit.converged
        self.bic, self.aic = _ic(fit.log_prob, fit, np.log(fit.log_prob.size)), _ic(fit.log_prob, fit, 2.0)


class SweepResult:
    """rows (one SweepRow per k, in the order of ks) and best_k: the k of the least BIC, the smaller k on ties"""

    def __init__(self, rows):
        self.rows = rows
        best = rows[0]
        for r in rows[1:]:
            if r.bic < best.bic or (r.bic == best.bic and r.k < best.k):
                best = r
        self.best_k = best.k

    def row(self, k):
        return next(r for r in self.rows if r.k == k)

    def table(self):
        """float64 [len(ks)][6]: k, lower_bound, n_iter, converged, bic, aic"""
        return np.array([[r.k, r.lower_bound, r.n_iter, r.converged, r.bic, r.aic] for r in self.rows], np.float64).reshape(-1, 6)


def sweep(X, ks, backend="device", **gmm_kwargs):
    """gmm(X, k, **gmm_kwargs) with its BIC and AIC for every k of ks on one device copy of X: SweepResult(rows, best_k)"""
    ks = [int(v) for v in ks]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 1:
        raise GmmError("a sweep needs increasing k >= 1, got %r" % (ks,))
    X = _common.as_input(X, backend, GmmError)
    n, d = (int(s) for s in X.shape)
    for k in ks:
        check_domain(n, d, k, gmm_kwargs.get("covariance_type", "full"))
    return SweepResult([SweepRow(k, gmm(X, k, backend=backend, **gmm_kwargs)) for k in ks])


# ---- command line

def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.gmm")
    _common.add_cluster_arguments(ap, ("input", "output"), "factors", False)
    ap.add_argument("--k", type=int, default=None, help="number of components (optional with --sweep)")
    ap.add_argument("--cov", default="full", choices=("full", "diag"), help="covariance_type")
    _common.add_cluster_arguments(ap, ("--key",), "factors", False)
    ap.add_argument("--init", default="kmeans", help="kmeans, random or an int [n] .npy of labels")
    ap.add_argument("--n_init", type=int, default=1)
    ap.add_argument("--max_iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--reg_covar", type=float, default=1e-6)
    ap.add_argument("--seed", type=int, default=None, help="random_state")
    _common.add_cluster_arguments(ap, ("--backend",), "factors", False)
    ap.add_argument("--sweep", default=None, help="K1,K2,... or LO:HI[:STEP]: a mixture with BIC and AIC for every k; the result "
                    "written is that of --k if given, else of the least BIC")
    _common.add_cluster_arguments(ap, ("--truth",), "factors", False)
    ap.add_argument("--min_proba", type=float, default=None, help="P in (0, 1]: the mask keep = proba_max >= P in OUT.npz")
    _common.add_cluster_arguments(ap, ("--stack", "--params", "--ou", "--averages", "--device"), "factors", False)
    args = ap.parse_args(argv)
    ks = None
    if args.k is None and args.sweep is None:
        ap.error("one of --k and --sweep is needed")
    if args.min_proba is not None and not (0.0 < args.min_proba <= 1.0):
        ap.error("--min_proba is in (0, 1], got %r" % (args.min_proba,))
    if args.sweep is not None:
        try:
            ks = _km.parse_sweep(args.sweep)
        except _km.KMeansError as e:
            ap.error(str(e))
    try:
        X = _km.read_input(args.input, args.key)
        n, d = X.shape
        init = args.init if args.init in ("kmeans", "random") else np.load(args.init)
        for kk in (ks or []) + ([args.k] if args.k is not None else []):
            check_domain(n, d, kk, args.cov, args.max_iter, args.tol, args.reg_covar, args.n_init)
            _resolve_init(init, n, kk)
        truth = _km.read_truth(args.truth, n) if args.truth else None
    except (GmmError, _km.KMeansError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    _common.check_averages_arguments(ap, args, usage=False)
    if args.backend == "device" or args.averages:
        _common.require_gpu(_common.NO_GPU)
    kw = dict(covariance_type=args.cov, tol=args.tol, reg_covar=args.reg_covar, max_iter=args.max_iter, n_init=args.n_init,
              init_params=init, random_state=args.seed)
    swept = None
    try:
        Xb = _common.to_device(X, args.device) if args.backend == "device" else X
        if ks:
            swept = sweep(Xb, ks, backend=args.backend, **kw)
            if args.k is None:
                args.k = swept.best_k
        res = swept.row(args.k).model if swept is not None and args.k in ks else gmm(Xb, args.k, backend=args.backend, **kw)
    except ValueError as e:
        raise SystemExit("error: %s" % e)
    row = SweepRow(args.k, res)
    out = dict(weights=res.weights, means=res.means, covariances=res.covariances, precisions_cholesky=res.precisions_cholesky,
               labels=res.labels, proba_max=res.proba_max, log_likelihood=res.log_prob, lower_bound=np.float64(res.lower_bound),
               lower_bounds=res.lower_bounds, n_iter=np.int64(res.n_iter), converged=np.bool_(res.converged), bic=np.float64(row.bic),
               aic=np.float64(row.aic), k=np.int64(args.k), cov=np.str_(args.cov), init=np.str_(args.init), n_init=np.int64(args.n_init),
               max_iter=np.int64(args.max_iter), tol=np.float64(args.tol), reg_covar=np.float64(args.reg_covar),
               seed=np.int64(-1 if args.seed is None else args.seed), backend=np.str_(args.backend))
    msg = "%s: %d points x %d, k = %d (%s), %d iterations%s, lower bound %.6g, BIC %.6g, AIC %.6g" % (
        args.output, n, d, args.k, args.cov, res.n_iter, "" if res.converged else " (not converged)", res.lower_bound, row.bic, row.aic)
    if truth is not None:
        msg += _common.truth_scores(out, truth, res.labels)
    if args.min_proba is not None:
        keep = res.proba_max >= args.min_proba
        out["keep"], out["min_proba"] = keep, np.float64(args.min_proba)
        for c in range(args.k):
            sel = res.labels == c
            print("class %3d: %7d members, %7d kept" % (c, int(sel.sum()), int((sel & keep).sum())))
    if args.averages:
        msg += _common.write_averages(args, n, res.labels, args.k, None, GmmError)
    if swept is not None:
        out["sweep"], out["best_k"] = swept.table(), np.int64(swept.best_k)
        print("%5s %14s %7s %10s %14s %14s" % ("k", "lower bound", "n_iter", "converged", "BIC", "AIC"))
        for r in swept.rows:
            print("%5d %14.6g %7d %10s %14.6g %14.6g%s" % (r.k, r.lower_bound, r.n_iter, r.converged, r.bic, r.aic,
                                                          "  <- best" if r.k == swept.best_k else ""))
    np.savez(args.output, **out)
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
