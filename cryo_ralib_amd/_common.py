"""What the analysis modules (sdr, tsne, kmeans, gmm, dbscan, hdbscan, wiener) and the engine-less wrappers of api.py share: the
argument predicates, the input rules, the file readers, the launcher of the ra_* entries and the tails of the command lines.  Every
function that can refuse an input takes the calling module's exception class as `error`, so each module raises its own class with
one text.  Nothing here imports a feature module at module level; torch is imported where a device is touched.
"""
import ctypes
import math
import numbers

import numpy as np


# ---- argument predicates

def is_int(v):
    return isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, bool)


def is_real(v):
    return isinstance(v, (numbers.Real, np.number)) and not isinstance(v, bool) and math.isfinite(v)


def check_random_state(seed, error):
    """sklearn.utils.check_random_state"""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if is_int(seed):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise error("random_state is None, an integer or a numpy RandomState, got %r" % (seed,))


# ---- inputs

def as_input(X, backend, error, numpy_on_device=True, numpy_dtype=None):
    """X [n][d] as the backend takes it.  "device": a contiguous float32 CUDA tensor; a numpy array is copied to the current device
    unless numpy_on_device is False.  "numpy": a numpy array (a tensor is copied to the host), cast to numpy_dtype if one is
    given; a module that gives one also has the rank of a numpy array checked before it is copied to the device."""
    if backend == "device":
        import torch
        if numpy_on_device and isinstance(X, np.ndarray):
            if numpy_dtype is not None and X.ndim != 2:
                raise error("X is [n][d], got shape %s" % (X.shape,))
            X = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
        if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.is_contiguous()):
            raise error("backend 'device' takes a contiguous float32 CUDA tensor [n][d]"
                        + (" (or a numpy array, copied)" if numpy_on_device else ""))
        if X.ndim != 2:
            raise error("X is [n][d], got shape %s" % (tuple(X.shape),))
        return X
    if backend != "numpy":
        raise error("backend is 'device' or 'numpy', got %r" % (backend,))
    if not isinstance(X, np.ndarray) and hasattr(X, "detach"):
        X = X.detach().cpu().numpy()
    X = np.asarray(X)
    if X.ndim != 2:
        raise error("X is [n][d], got shape %s" % (X.shape,))
    return X if numpy_dtype is None else np.asarray(X, numpy_dtype)


def host_finite(A, step=1 << 16):
    """whether the numpy array A [n][...] holds finite values only, read a block of rows at a time"""
    return all(bool(np.all(np.isfinite(A[s:s + step]))) for s in range(0, A.shape[0], step))


def check_finite(X, backend, error):
    ok = bool(X.isfinite().all().item()) if backend == "device" else bool(np.all(np.isfinite(X)))
    if not ok:
        raise error("X holds NaN or infinite values")


# ---- rule 2's float64 reference of the DBSCAN and HDBSCAN checkers

def row_chunks(n):
    ch = max(1, (1 << 22) // n)
    return [(s, min(n, s + ch)) for s in range(0, n, ch)]


def d2_rows(X, s0, s1):
    """D2 [s1 - s0][n] of rule 2: differences in float64, the features in order, multiply and add unfused"""
    D = np.zeros((s1 - s0, X.shape[0]))
    for t in range(X.shape[1]):
        df = X[s0:s1, t, None] - X[None, :, t]
        D += df * df
    return D


# ---- files

def read_input(path, key, error):
    """[n][d] float32 from an .npz (key) or an .npy"""
    try:
        if path.endswith(".npz"):
            with np.load(path) as z:
                if key not in z.files:
                    raise error("%s has no array %r (it holds %s)" % (path, key, ", ".join(z.files)))
                X = z[key]
        else:
            X = np.load(path)
    except (OSError, ValueError) as e:
        raise error("%s: %s" % (path, e))
    X = np.ascontiguousarray(X, np.float32)
    if X.ndim != 2:
        raise error("%s: need an [n][d] array, got shape %s" % (path, X.shape))
    return X


def read_truth(path, n, error):
    """[n] int classes from an int .npy or a params.txt (idx angle_psi shift_x shift_y mirror class, rows in any order)"""
    try:
        if path.endswith(".npy"):
            y = np.load(path)
            if y.shape != (n,) or not np.issubdtype(y.dtype, np.integer):
                raise error("%s: need [%d] integers, got %s %s" % (path, n, y.dtype, y.shape))
            return y.astype(np.int64)
        rows = np.loadtxt(path, ndmin=2, dtype=np.float64)
    except (OSError, ValueError) as e:
        raise error("%s: %s" % (path, e))
    if rows.shape != (n, 6):
        raise error("%s: need %d rows of 6 columns (params.txt), got %s" % (path, n, rows.shape))
    idx = rows[:, 0].astype(np.int64)
    if not np.array_equal(np.sort(idx), np.arange(n)):
        raise error("%s: the idx column is not a permutation of 0 .. %d" % (path, n - 1))
    y = np.empty(n, np.int64)
    y[idx] = rows[:, 5].astype(np.int64)
    return y


def read_params(path, n, error):
    """[n][4] (alpha, sx, sy, mirror) from a params.txt (idx angle_psi shift_x shift_y mirror class, rows in any order) or an
    initial2Dparams.txt (alpha sx sy mirror, in stack order)"""
    try:
        rows = np.loadtxt(path, ndmin=2, dtype=np.float64)
    except ValueError as e:
        raise error("%s: not a params file (%s)" % (path, e))
    if rows.shape[0] != n:
        raise error("%s has %d rows, the stack %d images" % (path, rows.shape[0], n))
    if rows.shape[1] == 4:
        return rows
    if rows.shape[1] == 6:
        idx = rows[:, 0].astype(np.int64)
        if not np.array_equal(np.sort(idx), np.arange(n)) or not np.array_equal(idx, rows[:, 0]):
            raise error("%s: the idx column is not a permutation of 0 .. %d" % (path, n - 1))
        out = np.empty((n, 4))
        out[idx] = rows[:, 1:5]
        return out
    raise error("%s: rows of %d columns; expected 6 (params.txt) or 4 (initial2Dparams.txt)" % (path, rows.shape[1]))


# ---- device calls

def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Launcher:
    """torch, api, lib (libralign_hip.so), dev and stream (the current stream of dev) for a device or a tensor's device;
    call(name, *args) runs the entry lib.name(*args, stream) and raises api.EngineError unless it returns 0"""

    def __init__(self, where):
        import torch
        from . import api
        self.torch, self.api, self.lib = torch, api, api.load_library()
        self.dev = where.device if isinstance(where, torch.Tensor) else where
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def call(self, name, *args):
        self.api._check(getattr(self.lib, name)(*args, self.stream), name)


# ---- command line of the clustering tools

NO_GPU = "no GPU visible: use --backend numpy for the CPU checker (--averages needs the GPU)"


def add_cluster_arguments(ap, names, key_default, noise):
    """adds the options `names` that the clustering tools share, in that order (a tool's usage line lists its own options between
    them).  key_default: "factors" or "embedding"; noise: the tool labels noise, which --truth and --averages leave out"""
    first, second = ("sdr", "tsne") if key_default == "factors" else ("tsne", "sdr")
    shared = {
        "input": dict(help="OUT.npz of the %s or %s tool, or an [n][d] .npy" % (first, second)),
        "output": dict(help="OUT.npz"),
        "--key": dict(default=key_default, help="array of an .npz input (default %s; %s for the %s tool)" % (
            key_default, "embedding" if key_default == "factors" else "factors", second)),
        "--backend": dict(default="device", choices=("device", "numpy")),
        "--truth": dict(default=None, help="int .npy or params.txt: purity, c_purity and contingency "
                        + ("over the non-noise points" if noise else "in OUT.npz")),
        "--stack": dict(default=None, help="stack for --averages (.hdf, .mrcs or .npy)"),
        "--params": dict(default=None, help="params.txt or initial2Dparams.txt of the stack"),
        "--ou": dict(type=int, default=None, help="outer radius of the averages' mask"),
        "--averages": dict(default=None, help="REFS.{hdf,mrcs,npy}: the " + ("class averages of the non-noise particles" if noise
                                                                           else "k class averages")),
        "--device": dict(type=int, default=0),
    }
    for name in names:
        ap.add_argument(name, **shared[name])


def check_averages_arguments(ap, args, usage=True):
    """--averages without --stack, --params and --ou: a usage error, or with usage=False the tools' "error: ..." exit"""
    if args.averages and not (args.stack and args.params and args.ou):
        if usage:
            ap.error("--averages needs --stack, --params and --ou")
        raise SystemExit("error: --averages needs --stack, --params and --ou")


def require_gpu(message):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(message)


def to_device(X, index):
    import torch
    return torch.from_numpy(X).to(torch.device("cuda", index))


def truth_scores(out, truth, labels, keep=None):
    """purity, c_purity and contingency of the labels (of the points of the mask `keep`, if given) into out; returns their part of
    the summary line.  With nothing kept the scores are NaN and the matrix is [0][0]"""
    from . import kmeans
    if keep is not None:
        truth, labels = truth[keep], labels[keep]
    if labels.size:
        out["purity"], out["c_purity"] = np.float64(kmeans.purity_score(truth, labels)), np.float64(kmeans.c_purity_score(truth, labels))
        out["contingency"] = kmeans.contingency_matrix(truth, labels)
    else:
        out["purity"], out["c_purity"], out["contingency"] = np.float64(np.nan), np.float64(np.nan), np.zeros((0, 0), np.int64)
    return ", purity %.4f, c_purity %.4f" % (out["purity"], out["c_purity"])


def write_averages(args, n, labels, k, keep, error, max_k=None):
    """--averages: the k class averages (kmeans.class_averages) of --stack by --params, of the particles of the mask `keep` if
    given, written to args.averages; returns their part of the summary line.  max_k: the most clusters a tool may bring"""
    from . import kmeans, sdr, stackio
    try:
        if max_k is not None and not 1 <= k <= max_k:
            raise error("--averages takes 1 to %d clusters, got %d" % (max_k, k))
        stack = np.ascontiguousarray(stackio.read_stack(args.stack), np.float32)
        if stack.ndim != 3 or stack.shape[0] != n:
            raise error("%s: need a stack of %d images, got shape %s" % (args.stack, n, stack.shape))
        prm = sdr.read_params(args.params, n)
        if keep is not None:
            stack, prm, labels = stack[keep], prm[keep], labels[keep]
        refs = kmeans.class_averages(stack, prm, labels, k, args.ou, device=args.device)
    except (ValueError, OSError) as e:
        raise SystemExit("error: %s" % e)
    stackio.write_stack(args.averages, refs)
    return ", averages -> %s" % args.averages
